"""Greedy conditional-variance selection of the inducing patches (--inducing-init greedy), what needs no GPU: the NumPy reference of
tests/greedy_ref.py on a hand-worked case, the flag and its errors, what ModelBuilder.spec() hands to ``kernels.greedy_variance`` for every
layer, the untouched default path, the host fill rule, and the declaration of the C entry."""
import numpy as np
import pytest

import greedy_ref as gr


# ---- 1. the reference -----------------------------------------------------------------------------------------------------------------------
def _hand_case():
    """Six points on a line, RBF with variance 4 and lengthscale 1.  a = sqrt(2 ln 2) makes k(0, a) = variance / 2 = 2, b = sqrt(2 ln 4) makes
    k(200, 200 + b) = variance / 4 = 1; points 100 apart have k = 4 exp(-5000) = 0 exactly.  By hand, with a floor of 1e-9:
      pick 0: all residuals 4, lowest index 0.  c_0 = [2, 1, 0, 0, 0, 0]                       d = [0, 3, 4, 4, 4, 4]        trace 19
      pick 1: index 2 (first of the 4s); its copy, index 3, goes to 0                          d = [0, 3, 0, 0, 4, 4]        trace 11
      pick 2: index 4; c_2[5] = 1 / 2                                                          d = [0, 3, 0, 0, 0, 3.75]     trace 6.75
      pick 3: index 5                                                                          d = [0, 3, 0, 0, 0, 0]        trace 3
      pick 4: index 1                                                                          d = 0                         trace 0
      pick 5: nothing above the floor: n_greedy = 5."""
    a, b = np.sqrt(2.0 * np.log(2.0)), np.sqrt(2.0 * np.log(4.0))
    return np.array([[0.0], [a], [100.0], [100.0], [200.0], [200.0 + b]])


def test_reference_on_a_hand_worked_case():
    out = gr.greedy_variance_ref(_hand_case(), 6, "rbf", 4.0, 1.0, min_variance=1e-9)
    assert out["n_greedy"] == 5
    assert out["rows"].tolist() == [0, 2, 4, 5, 1, -1]
    np.testing.assert_allclose(out["trace"], [19.0, 11.0, 6.75, 3.0, 0.0, 0.0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["pivots"], [4.0, 4.0, 4.0, 3.75, 3.0], rtol=0, atol=1e-12)
    assert np.all(out["residual"] <= 1e-12)
    assert np.all(out["factor"][5] == 0.0)
    np.testing.assert_allclose(out["factor"][0], [2.0, 1.0, 0, 0, 0, 0], rtol=0, atol=1e-14)


@pytest.mark.parametrize("kind,p1,p2", [("rbf", 3.0, 0.0), ("matern32", 3.0, 0.0), ("matern52", 3.0, 0.0), ("acos", 1.0, 1.0)])
def test_reference_factor_reproduces_the_selected_gram(kind, p1, p2):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((40, 9))
    out = gr.greedy_variance_ref(X, 12, kind, 5.0, p1, p2)
    rows = out["rows"]
    assert out["n_greedy"] == 12 and len(set(rows.tolist())) == 12
    L = out["factor"][:, rows].T                 # L[s, t] = c_t[rows[s]]: row s of the factor of K(X[rows])
    assert np.all(np.triu(L, 1) == 0.0) and np.all(np.diag(L) > 0)
    K = gr.gram(X[rows], kind, 5.0, p1, p2)
    np.fill_diagonal(K, gr.kdiag(kind, 5.0))    # where the residual starts (the Matern k(x, x) = k(r = 1e-6) sits 1.5e-12 below)
    np.testing.assert_allclose(L @ L.T, K, rtol=0, atol=5e-13 * 5.0)
    # the whole factor: the Nystrom approximation, exact on the selected rows and columns, and the trace is what it leaves of the diagonal
    Q = out["factor"].T @ out["factor"]
    want = gr.gram(X, kind, 5.0, p1, p2)[rows]
    want[np.arange(12), rows] = gr.kdiag(kind, 5.0)
    np.testing.assert_allclose(Q[rows], want, rtol=0, atol=5e-12)
    assert abs(out["trace"][-1] - (40 * gr.kdiag(kind, 5.0) - np.trace(Q))) <= 1e-11
    assert np.all(np.diff(out["trace"]) < 0)


def test_reference_with_ard_is_the_scaled_rbf():
    rng = np.random.default_rng(4)
    X, ls = rng.standard_normal((30, 5)), rng.uniform(0.5, 1.5, 5)
    a = gr.greedy_variance_ref(X, 8, "rbf", 5.0, ard=ls)
    b = gr.greedy_variance_ref(X / ls, 8, "rbf", 5.0, 1.0)
    assert a["rows"].tolist() == b["rows"].tolist()
    np.testing.assert_allclose(a["trace"], b["trace"], rtol=1e-13)


# ---- 2. the flag ----------------------------------------------------------------------------------------------------------------------------
def test_flag_table_and_parser(tmp_path):
    from deepcgp_amd.arguments import FLAGS, default_parser, parse_inducing_init
    from deepcgp_amd.utils import toml_lines
    row = [f for f in FLAGS if f[0] == "--inducing-init"]
    assert len(row) == 1 and row[0][1] is str and row[0][2] == "kmeans" and "kmeans" in row[0][3] and "greedy" in row[0][3]
    base = ['--name', 't']
    assert parse_inducing_init(default_parser().parse_args(base)) == "kmeans"
    assert parse_inducing_init(default_parser().parse_args(base + ['--inducing-init', 'greedy'])) == "greedy"
    with pytest.raises(ValueError, match="--inducing-init"):
        parse_inducing_init(default_parser().parse_args(base + ['--inducing-init', 'lloyd']))

    class Old(object):      # a namespace from before the flag
        pass
    assert parse_inducing_init(Old()) == "kmeans"
    assert 'inducing_init = "greedy"' in toml_lines(vars(default_parser().parse_args(base + ['--inducing-init', 'greedy'])))


# ---- 3. ModelBuilder.spec() -------------------------------------------------------------------------------------------------------------------
ARCH = ['--name', 't', '-M', '4,5,6', '--feature-maps', '2,3', '--filter-sizes', '3,3,2', '--strides', '1,1,1']


def _images():
    return np.random.default_rng(0).standard_normal((12, 9, 9, 1))


def _spec(monkeypatch, extra, model_path=None):
    """spec() with ``kernels.greedy_variance`` replaced by a recorder that returns the first k candidates."""
    from deepcgp_amd import kernels
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder
    calls = []

    def fake(points, k, base_kernel, min_variance=kernels.JITTER, return_info=False):
        calls.append((np.array(points), k, base_kernel, min_variance))
        info = {"rows": np.arange(k), "n_greedy": k, "trace": np.zeros(k), "residual": np.zeros(len(points))}
        return (np.array(points[:k]), info) if return_info else np.array(points[:k])
    monkeypatch.setattr(kernels, "greedy_variance", fake)
    fl = default_parser().parse_args(ARCH + extra)
    np.random.seed(11)
    spec = ModelBuilder(fl, _images(), np.zeros((12, 1)), model_path).spec()
    return spec, calls


def test_greedy_builder_passes_every_layer_its_kernel(monkeypatch):
    from deepcgp_amd.kernels import JITTER, RBF
    spec, calls = _spec(monkeypatch, ['--inducing-init', 'greedy'])
    assert [(c[0].shape, c[1]) for c in calls] == [((400, 9), 4), ((500, 18), 5), ((600, 12), 6)]      # 100 M candidates of f f C elements each
    for (_, _, bk, floor), L in zip(calls, (9, 18, 12)):
        assert type(bk) is RBF and not bk.ARD and bk.input_dim == L and bk._describe() == [0.0, 5.0, 5.0, 0.0] and floor == JITTER
    assert [c["Z"].shape for c in spec["convs"]] == [(4, 9), (5, 18)] and spec["head"]["Z"].shape == (6, 12)
    for c, call in zip(spec["convs"] + [spec["head"]], calls):
        assert np.array_equal(c["Z"], call[0][:call[1]])


def test_greedy_builder_draws_the_candidates_kmeans_would(monkeypatch):
    from deepcgp_amd.models import draw_patches
    _, calls = _spec(monkeypatch, ['--inducing-init', 'greedy'])
    np.random.seed(11)
    assert np.array_equal(calls[0][0], draw_patches(_images(), 400, 3))


def test_greedy_builder_with_ard(monkeypatch):
    from deepcgp_amd.kernels import RBF
    _, calls = _spec(monkeypatch, ['--inducing-init', 'greedy', '--ard'])
    for (_, _, bk, _), L in zip(calls[:2], (9, 18)):
        assert type(bk) is RBF and bk.ARD and bk.variance == 5.0 and np.array_equal(bk.lengthscales, np.full(L, 5.0))
    assert type(calls[2][2]) is RBF and not calls[2][2].ARD                       # the patch head keeps its scalar RBF


def test_greedy_builder_with_matern52_and_acos(monkeypatch):
    from deepcgp_amd.kernels import ArcCosine, Matern52, RBF
    _, calls = _spec(monkeypatch, ['--inducing-init', 'greedy', '--base-kernel', 'matern52'])
    for (_, _, bk, _), L in zip(calls[:2], (9, 18)):
        assert type(bk) is Matern52 and bk.input_dim == L and bk._describe() == [3.0, 5.0, 5.0, 0.0]
    assert type(calls[2][2]) is RBF
    _, calls = _spec(monkeypatch, ['--inducing-init', 'greedy', '--base-kernel', 'acos'])
    for (_, _, bk, _), L in zip(calls[:2], (9, 18)):
        assert type(bk) is ArcCosine and bk.input_dim == L and bk._describe() == [1.0, 1.0, 1.0, 1.0]      # what build_layers_from_spec builds
    assert type(calls[2][2]) is RBF


def test_greedy_builder_with_a_dense_head(monkeypatch):
    from deepcgp_amd.kernels import RBF
    import sklearn.cluster

    def no_sklearn(*a, **k):
        raise AssertionError("sklearn's k-means was called on the greedy path")
    monkeypatch.setattr(sklearn.cluster, "KMeans", no_sklearn)
    spec, calls = _spec(monkeypatch, ['--inducing-init', 'greedy', '--last-kernel', 'rbf'])
    pts, k, bk, _ = calls[2]
    D = 5 * 5 * 3                                        # 9 -> 7 -> 5 pixels a side, 3 maps: the flattened features
    assert pts.shape == (12, D) and k == 6               # all 12 initialisation rows: fewer than 100 M
    assert type(bk) is RBF and bk.ARD and bk.input_dim == D and bk.variance == 5.0 and np.array_equal(bk.lengthscales, np.full(D, 5.0))
    assert spec["head"]["Z"].shape == (6, D)


def test_greedy_builder_samples_a_large_dense_candidate_set(monkeypatch):
    from deepcgp_amd import kernels
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder
    seen = []

    def fake(points, k, base_kernel, min_variance=kernels.JITTER, return_info=False):
        seen.append(np.array(points))
        return np.array(points[:k]), {"rows": np.arange(k), "n_greedy": k, "trace": np.zeros(k), "residual": np.zeros(len(points))}
    monkeypatch.setattr(kernels, "greedy_variance", fake)
    X = np.random.default_rng(1).standard_normal((150, 4, 4, 1))
    fl = default_parser().parse_args(['--name', 't', '-M', '1', '--feature-maps', '', '--filter-sizes', '2', '--strides', '1', '--last-kernel', 'rbf',
                                      '--inducing-init', 'greedy'])
    ModelBuilder(fl, X, np.zeros((150, 1))).spec()
    flat = X.reshape(150, 16)
    assert seen[0].shape == (100, 16)                    # 100 M of the 150 rows ...
    assert len({r.tobytes() for r in seen[0]}) == 100 and all(any(np.array_equal(r, f) for f in flat) for r in seen[0][:5])      # ... distinct rows of them


def test_greedy_builder_leaves_a_checkpoints_Z_alone(monkeypatch, tmp_path):
    rng = np.random.default_rng(5)
    Z0 = rng.standard_normal((4, 9))
    path = str(tmp_path / "ckpt.npy")
    np.save(path, {"DGP/layers/0/feature/Z": Z0, "DGP/layers/1/conv_kernel/base_kernel/variance": np.array(2.5),
                   "DGP/layers/1/conv_kernel/base_kernel/lengthscales": np.array(1.5), "DGP/layers/2/kern/base_kernel/variance": np.array(3.0),
                   "global_step": 7})
    spec, calls = _spec(monkeypatch, ['--inducing-init', 'greedy', '--load-model', path], model_path=path)
    assert np.array_equal(spec["convs"][0]["Z"], Z0)
    assert [c[1] for c in calls] == [5, 6]               # layer 0 is not selected for
    assert calls[0][2]._describe() == [0.0, 2.5, 1.5, 0.0]      # kernel parameters but no Z: selected under the checkpoint's kernel
    assert calls[1][2]._describe() == [0.0, 3.0, 5.0, 0.0]


def test_greedy_builder_reports_a_stall(monkeypatch, capsys):
    from deepcgp_amd import kernels
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder

    def fake(points, k, base_kernel, min_variance=kernels.JITTER, return_info=False):
        return np.array(points[:k]), {"rows": np.arange(k), "n_greedy": k - 1 if k == 5 else k, "trace": np.zeros(k), "residual": np.zeros(len(points))}
    monkeypatch.setattr(kernels, "greedy_variance", fake)
    ModelBuilder(default_parser().parse_args(ARCH + ['--inducing-init', 'greedy']), _images(), np.zeros((12, 1))).spec()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "greedy" in ln]
    assert len(lines) == 1 and "layer 1" in lines[0] and "4 of M = 5" in lines[0] and "0.001" in lines[0]


def test_default_flag_takes_todays_path(monkeypatch):
    """kmeans: from_images is called with exactly three positional arguments and nothing else, greedy_variance never."""
    import deepcgp_amd.models as M
    from deepcgp_amd import kernels
    seen = []

    def three(cls, imgs, m, f):         # a fourth argument or a keyword would be a TypeError
        seen.append((imgs.shape, m, f))
        return cls(np.zeros((m, f * f * imgs.shape[3])))
    monkeypatch.setattr(M.PatchInducingFeatures, "from_images", classmethod(three))
    spec, calls = _spec(monkeypatch, [])
    assert calls == []
    assert [(s[1], s[2]) for s in seen] == [(4, 3), (5, 3), (6, 2)]
    spec, calls = _spec(monkeypatch, ['--inducing-init', 'kmeans'])
    assert calls == [] and len(seen) == 6
    with pytest.raises(ValueError, match="--inducing-init"):
        _spec(monkeypatch, ['--inducing-init', 'nope'])


def test_from_images_methods():
    from deepcgp_amd.kernels import PatchInducingFeatures, RBF
    with pytest.raises(ValueError, match="base_kernel"):
        PatchInducingFeatures.from_images(_images(), 4, 3, method="greedy")
    with pytest.raises(ValueError, match="method"):
        PatchInducingFeatures.from_images(_images(), 4, 3, method="lloyd", base_kernel=RBF(9))


# ---- 4. the host side of the selection ----------------------------------------------------------------------------------------------------------
def test_fill_rule():
    from deepcgp_amd.kernels import _greedy_fill
    #                   0    1    2    3    4    5    6    7
    resid = np.array([0.0, 3e-4, 0.0, 5e-4, 3e-4, 0.0, 5e-4, 1e-5])
    rows = np.array([2, 0, -1, -1, -1, -1], np.int32)                   # two greedy picks (their residual is 0), then the stall
    assert _greedy_fill(rows, 2, resid, 6).tolist() == [2, 0, 3, 6, 1, 4]      # decreasing residual, ties to the lower index; never 5 (exactly 0)
    assert _greedy_fill(rows, 2, resid, 7).tolist() == [2, 0, 3, 6, 1, 4, 7]
    with pytest.raises(ValueError, match="only 7 usable"):
        _greedy_fill(rows, 2, resid, 8)
    assert _greedy_fill(np.array([4, 1, 3]), 3, resid, 3).tolist() == [4, 1, 3]      # no stall: the picks as they are
    # a pick is never taken twice, whatever its residual says
    assert _greedy_fill(np.array([3, -1, -1]), 1, resid, 3).tolist() == [3, 6, 1]


def test_greedy_variance_argument_errors():
    from deepcgp_amd.kernels import greedy_variance, RBF
    with pytest.raises(ValueError, match="k = 5 rows of n = 4"):
        greedy_variance(np.zeros((4, 3)), 5, RBF(3))
    with pytest.raises(ValueError, match="k = 0"):
        greedy_variance(np.zeros((4, 3)), 0, RBF(3))
    with pytest.raises(ValueError, match="length 3"):
        greedy_variance(np.zeros((4, 2)), 2, RBF(3))
    with pytest.raises(TypeError, match="base_kernel"):
        greedy_variance(np.zeros((4, 3)), 2, type("K", (), {"input_dim": 3})())


def test_entry_is_declared():
    from deepcgp_amd import device as dev
    assert "dcgp_greedy_variance" in dev.declared_symbols()
    assert "dcgp_greedy_variance" in dev._SIGS and len(dev._SIGS["dcgp_greedy_variance"]) == 16

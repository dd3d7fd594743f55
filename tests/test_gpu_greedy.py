"""GPU: dcgp_greedy_variance (csrc/greedy.hip) against the NumPy reference of tests/greedy_ref.py, its determinism, the stall on duplicate
candidates with the host fill, its argument errors, and ModelBuilder under --inducing-init greedy.

Tolerance: the operator tolerance of this suite, 1e-9 relative to the tensor's scale (tests/test_gpu_ops.py).  The selected ROWS must be equal,
which only means something where the reference's own choice is not a coin toss: every parity case first asserts, on the reference alone,
that every pivot is at least 1e-2 variance (nothing then amplifies fp64 rounding beyond the tolerance) and that at every pick the largest
residual leads the second largest distinct one by at least 1e-8 variance (seven orders above the rounding of either side).

The shapes are the smallest at which the kernel can go wrong: a single row; n below, at and just past a workgroup's 256 columns; k no multiple
of the projection's four chains; d shorter and longer than a wave.  They run a handful of workgroups: a launch of more workgroups than the chip
has CUs is not covered here.  The ``greedy_wgs`` switch makes a lane take several columns, the path of n > 256 * 1024."""
import ctypes as C

import numpy as np
import pytest

import greedy_ref as gr

pytestmark = pytest.mark.gpu

RTOL = 1e-9
VARIANCE = 5.0
SHAPES = [(1, 3, 1), (64, 9, 8), (257, 25, 32), (517, 27, 33), (300, 490, 24)]
KERNELS = ["rbf", "rbf_ard", "matern32", "matern52", "acos"]


def close(a, b, scale, name):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err = np.max(np.abs(a - b)) / scale if a.size else 0.0
    print("%s: max err / scale %.3e" % (name, err))
    assert err <= RTOL, "%s: max rel err %.3e > %.1e" % (name, err, RTOL)


def make_kernel(kern, d, rng):
    """(device kernel object, the reference's keyword arguments)."""
    from deepcgp_amd.kernels import RBF, ArcCosine, Matern32, Matern52
    ls = float(np.sqrt(d))
    if kern == "rbf":
        return RBF(d, VARIANCE, ls), dict(kind="rbf", variance=VARIANCE, p1=ls)
    if kern == "rbf_ard":
        ard = ls * rng.uniform(0.5, 1.5, d)
        return RBF(d, VARIANCE, ard, ARD=True), dict(kind="rbf", variance=VARIANCE, ard=ard)
    if kern == "matern32":
        return Matern32(d, VARIANCE, ls), dict(kind="matern32", variance=VARIANCE, p1=ls)
    if kern == "matern52":
        return Matern52(d, VARIANCE, ls), dict(kind="matern52", variance=VARIANCE, p1=ls)
    return ArcCosine(d, 0, VARIANCE, 1.0, 1.0), dict(kind="acos", variance=VARIANCE, p1=1.0, p2=1.0)


_CASES = {}


def case(n, d, k, kern):
    """Inputs, kernel and the reference's result of one parity case: computed once, shared, never changed."""
    key = (n, d, k, kern)
    if key not in _CASES:
        rng = np.random.default_rng(n)
        X = rng.standard_normal((n, d))
        bk, kw = make_kernel(kern, d, rng)
        ref = gr.greedy_variance_ref(X, k, min_variance=0.0, **kw)
        for v in (X, *ref.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CASES[key] = (X, bk, kw, ref)
    return _CASES[key]


def check_precondition(ref, k):
    assert ref["n_greedy"] == k
    print("smallest pivot %.3e variance, smallest gap %.3e variance" % (ref["pivots"].min() / VARIANCE, ref["gaps"].min() / VARIANCE))
    assert ref["pivots"].min() >= 1e-2 * VARIANCE
    assert ref["gaps"].min() >= 1e-8 * VARIANCE


def check_against_reference(out, ref, n, k):
    assert out["n_greedy"] == k
    assert out["rows"].tolist() == ref["rows"].tolist()
    close(out["trace"], ref["trace"], n * VARIANCE, "trace")
    close(out["residual"], ref["residual"], VARIANCE, "residual")
    close(out["factor"], ref["factor"], np.sqrt(VARIANCE), "factor")
    L = out["factor"][:, out["rows"]].T              # L[s, t] = c_t[rows[s]]
    assert np.all(np.triu(L, 1) == 0.0) and np.all(np.diag(L) > 0.0)


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_parity(ctx, n, d, k, kern):
    from deepcgp_amd.kernels import greedy_variance_device
    X, bk, _, ref = case(n, d, k, kern)
    check_precondition(ref, k)
    out = greedy_variance_device(X, k, bk, min_variance=0.0, factor=True)
    check_against_reference(out, ref, n, k)


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_factor_reproduces_the_device_gram(ctx, n, d, k, kern):
    """L L^T against the device's own ``base_kernel._gram(Z, 0)``, at the operator tolerance, every entry, the diagonal included.  The residual
    starts at the Gram matrix's own diagonal: ``variance`` for the stationary kernels (their k(x, x) is variance to 1.5e-12), the constant
    variance (1 - acos(1 - 1e-15) / pi) for the ArcCosine -- started from Kdiag = variance its factor reproduced a diagonal 1.423e-8 of the scale
    above the device Gram's, on every shape."""
    from deepcgp_amd.kernels import greedy_variance_device
    X, bk, _, ref = case(n, d, k, kern)
    check_precondition(ref, k)
    out = greedy_variance_device(X, k, bk, min_variance=0.0, factor=True)
    assert out["rows"].tolist() == ref["rows"].tolist()
    L = out["factor"][:, out["rows"]].T
    close(L @ L.T, bk._gram(X[out["rows"]], 0.0), VARIANCE, "L L^T vs the device Gram")


@pytest.mark.parametrize("kern", ["rbf", "acos"])
def test_several_columns_a_lane(ctx, kern):
    """n = 517 on two workgroups: every lane takes two columns, the second round's tail is empty for most of them."""
    from deepcgp_amd.kernels import greedy_variance_device
    n, d, k = 517, 27, 33
    X, bk, _, ref = case(n, d, k, kern)
    with ctx.options(greedy_wgs=2):
        out = greedy_variance_device(X, k, bk, min_variance=0.0, factor=True)
    check_against_reference(out, ref, n, k)


def test_two_calls_give_the_same_bits(ctx):
    from deepcgp_amd.kernels import greedy_variance_device
    X, bk, _, _ = case(517, 27, 33, "matern52")
    a = greedy_variance_device(X, 33, bk, min_variance=0.0, factor=True)
    b = greedy_variance_device(X, 33, bk, min_variance=0.0, factor=True)
    for key in ("rows", "trace", "residual", "factor"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["n_greedy"] == b["n_greedy"] == 33


def test_k_equals_n_selects_every_row_once(ctx):
    from deepcgp_amd.kernels import greedy_variance_device
    X, bk, kw, _ = case(64, 9, 8, "rbf")
    out = greedy_variance_device(X, 64, bk, min_variance=0.0, factor=True)
    assert out["n_greedy"] == 64 and sorted(out["rows"].tolist()) == list(range(64))
    assert np.all(out["residual"] == 0.0) and out["trace"][-1] == 0.0
    assert np.all(np.diff(out["trace"]) < 0.0)


def _duplicates():
    from deepcgp_amd.kernels import RBF
    rng = np.random.default_rng(40)
    base = rng.standard_normal((10, 9))
    X = np.repeat(base, 4, axis=0)[rng.permutation(40)]
    return X, RBF(9, VARIANCE, 3.0), dict(kind="rbf", variance=VARIANCE, p1=3.0)


def test_stall_on_duplicates_and_the_host_fill(ctx):
    from deepcgp_amd.kernels import JITTER, greedy_variance, greedy_variance_device
    X, bk, kw = _duplicates()
    ref = gr.greedy_variance_ref(X, 16, min_variance=JITTER, **kw)
    assert ref["n_greedy"] == 10
    out = greedy_variance_device(X, 16, bk, factor=True)            # the default floor
    assert out["n_greedy"] == 10
    assert out["rows"][:10].tolist() == ref["rows"][:10].tolist()
    assert np.all(out["rows"][10:] == -1)
    assert np.all(out["residual"] < JITTER)
    picked = X[out["rows"][:10]]
    assert len({r.tobytes() for r in picked}) == 10                 # no selected row is a copy of another
    assert np.all(out["trace"][10:] == out["trace"][9]) and np.all(out["factor"][10:] == 0.0)
    close(out["trace"], ref["trace"], 40 * VARIANCE, "trace")
    # the host fill: the rest by residual (what rounding leaves of a copy's: ~1e-15), 16 distinct indices, the same on a second call
    Z1, info1 = greedy_variance(X, 16, bk, return_info=True)
    Z2, info2 = greedy_variance(X, 16, bk, return_info=True)
    print("residuals of the fill:", info1["residual"][info1["rows"][10:]])
    assert info1["n_greedy"] == 10 and len(set(info1["rows"].tolist())) == 16 and info1["rows"][:10].tolist() == out["rows"][:10].tolist()
    assert info1["rows"].tolist() == info2["rows"].tolist() and Z1.tobytes() == Z2.tobytes()
    assert np.array_equal(Z1, X[info1["rows"]])
    filled = info1["rows"][10:]
    assert np.all(info1["residual"][filled] > 0.0) and np.all(np.diff(info1["residual"][filled]) <= 0.0)
    with pytest.raises(ValueError, match="k = 45 rows of n = 40"):
        greedy_variance(X, 45, bk)


def test_a_floor_above_the_variance_selects_nothing(ctx):
    from deepcgp_amd.kernels import greedy_variance_device
    X, bk, _, _ = case(64, 9, 8, "rbf")
    out = greedy_variance_device(X, 8, bk, min_variance=VARIANCE, factor=True)
    assert out["n_greedy"] == 0 and np.all(out["rows"] == -1)
    assert np.all(out["residual"] == VARIANCE) and np.all(out["trace"] == 64 * VARIANCE) and np.all(out["factor"] == 0.0)


def test_candidates_that_are_not_finite_are_an_error(ctx):
    from deepcgp_amd import device as dev
    from deepcgp_amd.kernels import greedy_variance_device
    X, bk, _, _ = case(64, 9, 8, "rbf")
    bad = X.copy()
    bad[17, 3] = np.nan
    with pytest.raises(dev.DcgpError, match="non-finite residual at pivot 0") as e:
        greedy_variance_device(bad, 8, bk)
    assert e.value.code == dev.ERR_ARG


def test_argument_errors(ctx):
    """Every DCGP_ERR_ARG case by its message; nothing is launched (the outputs keep the bytes they had)."""
    from deepcgp_amd import device as dev
    L = dev.lib()
    n, d, k = 16, 4, 3
    X = ctx.to_device(np.random.default_rng(0).standard_normal((n, d)))
    rows, trace, resid = ctx.to_device(np.full(k, 7, np.int32), np.int32), ctx.to_device(np.full(k, 7.0)), ctx.to_device(np.full(n, 7.0))
    ls_ok, ls_bad = ctx.to_device(np.ones(d)), ctx.to_device(np.array([1.0, 0.0, 1.0, 1.0]))
    ng = C.c_int(-5)

    def call(X=X.ptr, n=n, d=d, k=k, kind=0, variance=1.0, p1=1.0, p2=0.0, ard=None, floor=0.0, rows=rows.ptr, trace=trace.ptr, resid=resid.ptr,
             ng=C.byref(ng)):
        return L.dcgp_greedy_variance(ctx.handle, X, n, d, k, kind, variance, p1, p2, ard, floor, rows, trace, resid, None, ng)
    cases = [
        (dict(X=None), "X is NULL"), (dict(rows=None), "rows_out is NULL"), (dict(trace=None), "trace_out is NULL"),
        (dict(resid=None), "residual_out is NULL"), (dict(ng=None), "n_greedy_out is NULL"),
        (dict(k=0), "k = 0"), (dict(k=n + 1), "k = 17 exceeds n = 16"), (dict(k=4097, n=5000), "k = 4097"), (dict(d=0), "d = 0"),
        (dict(d=4097), "d = 4097"), (dict(n=0), "n = 0"), (dict(n=2 ** 31), "n = 2147483648"),
        (dict(kind=4), "unknown kernel_type 4"), (dict(kind=-1), "unknown kernel_type -1"),
        (dict(kind=2, ard=ls_ok.ptr), "ard_lengthscales go with kernel_type 0"), (dict(kind=1, ard=ls_ok.ptr), "ard_lengthscales go with kernel_type 0"),
        (dict(variance=0.0), "variance must be positive"), (dict(variance=-1.0), "variance must be positive"),
        (dict(p1=0.0), "p1 (lengthscale) must be positive"), (dict(kind=3, p1=-2.0), "p1 (lengthscale) must be positive"),
        (dict(kind=1, p1=0.0), "p1 (weight variance) must be positive"), (dict(kind=1, p2=-1.0), "p2 (bias variance) must not be negative"),
        (dict(ard=ls_bad.ptr), "ard_lengthscales[1] must be positive"),
        (dict(floor=-1e-3), "min_variance must not be negative"),
    ]
    for kw, msg in cases:
        assert call(**kw) == dev.ERR_ARG, kw
        got = L.dcgp_last_error(ctx.handle).decode()
        assert got.startswith("greedy_variance: ") and msg in got, (kw, got)
        with pytest.raises(dev.DcgpError):
            ctx._check(dev.ERR_ARG)
    assert L.dcgp_greedy_variance(None, X.ptr, n, d, k, 0, 1.0, 1.0, 0.0, None, 0.0, rows.ptr, trace.ptr, resid.ptr, None, C.byref(ng)) == dev.ERR_ARG
    assert np.all(rows.numpy() == 7) and np.all(trace.numpy() == 7.0) and np.all(resid.numpy() == 7.0) and ng.value == -5
    assert call() == dev.DCGP_OK and ng.value == 3 and sorted(set(rows.numpy().tolist())) == sorted(rows.numpy().tolist())


def test_the_call_keeps_no_workspace(ctx):
    """Scratch is allocated and freed inside the call: a ctx of its own holds no workspace behind it."""
    from deepcgp_amd import device as dev
    from deepcgp_amd import kernels
    X, bk, _, ref = case(257, 25, 32, "rbf")
    fresh = dev.Context(ctx.device)
    old = dev._default_ctx
    dev._default_ctx = fresh
    try:
        out = kernels.greedy_variance_device(X, 32, bk, min_variance=0.0)
        assert fresh.workspace_bytes() == (0, 0)
    finally:
        dev._default_ctx = old
        fresh.close()
    assert out["rows"].tolist() == ref["rows"].tolist() and out["factor"] is None


# ---- ModelBuilder under --inducing-init greedy ----------------------------------------------------------------------------------------------
ARCH = ['--name', 'g', '-M', '16,16', '--feature-maps', '2', '--filter-sizes', '3,3', '--strides', '1,1', '--batch-size', '16', '--num-samples', '2']


def _digits():
    from sklearn.datasets import load_digits
    dg = load_digits()
    X = (dg.data[:64] / 16.0).reshape(64, 8, 8, 1)
    return X, dg.target[:64].reshape(-1, 1).astype(np.float64)


def _is_row_of(Z, cand):
    pool = {r.tobytes() for r in np.ascontiguousarray(cand)}
    return all(z.tobytes() in pool for z in np.ascontiguousarray(Z))


@pytest.mark.parametrize("extra", [[], ['--base-kernel', 'acos'], ['--ard'], ['--last-kernel', 'rbf']], ids=["rbf", "acos", "ard", "dense_head"])
def test_builder(ctx, extra, tmp_path):
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder, draw_patches, identity_conv, save_model_parameters
    X, Y = _digits()
    fl = default_parser().parse_args(ARCH + ['--inducing-init', 'greedy'] + extra)
    np.random.seed(3)
    builder = ModelBuilder(fl, X, Y)
    model = builder.build()
    try:
        # replay the generator: every Z row is one of the candidates it was selected from
        np.random.seed(3)
        cand0 = draw_patches(X, 1600, 3)
        assert _is_row_of(model.layers[0].feature.Z, cand0)
        feats = identity_conv(X, 3, 1, 2, 1)
        cand1 = feats.reshape(64, -1) if '--last-kernel' in extra else draw_patches(feats, 1600, 3)
        assert _is_row_of(model.layers[1].feature.Z, cand1)
        assert model.layers[0].feature.Z.shape == (16, 9) and model.layers[1].feature.Z.shape[0] == 16
        elbo = model.compute_log_likelihood(X[:16].reshape(16, -1), Y[:16], seed=1)
        assert np.isfinite(elbo)
        # save / --load-model: Z comes back bit for bit and nothing is selected again
        path = str(tmp_path / "g.npy")
        saved = save_model_parameters(model, path)
        Zs = [np.array(l.feature.Z) for l in model.layers]
        assert all(np.array_equal(saved["DGP/layers/%d/feature/Z" % i], Z) for i, Z in enumerate(Zs))
        assert np.isfinite(model.train_step(X[:16].reshape(16, -1), Y[:16], 1e-3, seed=2))      # one Adam step runs
    finally:
        model.close()
    from deepcgp_amd import kernels
    fl2 = default_parser().parse_args(ARCH + ['--inducing-init', 'greedy', '--load-model', path] + extra)
    real = kernels.greedy_variance

    def never(*a, **k):
        raise AssertionError("a layer whose Z the checkpoint holds was selected for")
    kernels.greedy_variance = never
    try:
        spec = ModelBuilder(fl2, X, Y, path).spec()
    finally:
        kernels.greedy_variance = real
    for got, want in zip([c["Z"] for c in spec["convs"]] + [spec["head"]["Z"]], Zs):
        assert np.asarray(got).tobytes() == want.tobytes()


def test_default_flag_gives_the_parents_Z(ctx):
    """Without the flag the builder's Z is ``_cluster_patches`` called directly from the same generator state."""
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.kernels import _cluster_patches
    from deepcgp_amd.models import ModelBuilder, identity_conv
    X, Y = _digits()
    np.random.seed(3)
    spec = ModelBuilder(default_parser().parse_args(ARCH), X, Y).spec()
    np.random.seed(3)
    Z0 = _cluster_patches(X, 16, 3)
    Z1 = _cluster_patches(identity_conv(X, 3, 1, 2, 1), 16, 3)
    assert spec["convs"][0]["Z"].tobytes() == Z0.tobytes() and spec["head"]["Z"].tobytes() == Z1.tobytes()

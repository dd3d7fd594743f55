"""Per-dimension (ARD) lengthscales on the conv layers' RBF base kernel, what needs no GPU: the --ard flag and its errors, options.toml,
ModelBuilder.spec() and build_layers_from_spec producing ARD layers, the checkpoint's broadcast and refusal, the declared operator entry,
what keeps raising (Matern / ArcCosine ARD, ARD on a patch head), and the liveness of the torch reference on every case tests/test_gpu_ard.py
runs -- with the conv layers' ``lengthscales`` vectors among live_specs' median and capped groups (tests/ard_ref.py)."""
import functools

import numpy as np
import pytest

import ard_ref as ar
import live_specs as ls
import torch_ref as tr


class _NoPrior:
    """ConvLayer without its prior factorisation (the only device call of its constructor when q_sqrt is given)."""

    def __enter__(self):
        from deepcgp_amd.layers import ConvLayer
        self.cls, self.real = ConvLayer, ConvLayer._build_prior_cholesky
        ConvLayer._build_prior_cholesky = lambda self: None
        return self

    def __exit__(self, *exc):
        self.cls._build_prior_cholesky = self.real


def _flags(*extra):
    from deepcgp_amd.arguments import default_parser
    return default_parser().parse_args(["--name", "t", "-M", "5,6,7", "--feature-maps", "4,2", "--filter-sizes", "3,3,3", "--strides", "1,1,1",
                                        "--num-samples", "2", "--batch-size", "4"] + list(extra))


def _builder(monkeypatch, *extra, path=None):
    from deepcgp_amd import kernels
    from deepcgp_amd.models import ModelBuilder
    monkeypatch.setattr(kernels, "kmeans", lambda sample, k, **kw: np.array(sample[:k]))      # (Lloyd's iterations run on the device)
    X = np.random.default_rng(0).standard_normal((30, 10, 10, 1))
    return ModelBuilder(_flags(*extra), X, np.zeros((30, 1)), model_path=path)


def _fill(spec):
    for l in spec["convs"] + [spec["head"]]:
        l["q_mu"] = np.zeros((l["M"], l["R"]))
        l["q_sqrt"] = np.tile(np.eye(l["M"]), (l["R"], 1, 1))
    return spec


# ---- the flag -----------------------------------------------------------------------------------------------------------------------------
def test_flag_default_spec_and_errors(monkeypatch):
    from deepcgp_amd.arguments import default_parser
    assert default_parser().parse_args(["--name", "x"]).ard is False
    assert _flags("--ard").ard is True
    np.random.seed(0)
    plain = _builder(monkeypatch).spec()
    assert all(c["ls"] == 5.0 and isinstance(c["ls"], float) for c in plain["convs"])
    np.random.seed(0)
    spec = _builder(monkeypatch, "--ard").spec()
    # the reference's initial value, broadcast: L = f f C per layer; the head keeps its scalar
    assert [np.shape(c["ls"]) for c in spec["convs"]] == [(9,), (36,)] and all(np.all(c["ls"] == 5.0) for c in spec["convs"])
    assert spec["head"]["ls"] == 5.0 and all(c["variance"] == 5.0 for c in spec["convs"])
    for a, b in zip(plain["convs"] + [plain["head"]], spec["convs"] + [spec["head"]]):      # nothing else moves
        assert np.array_equal(a["Z"], b["Z"])
    for base in ("acos", "matern32", "matern52"):
        with pytest.raises(ValueError, match="--ard.*--base-kernel"):
            _builder(monkeypatch, "--ard", "--base-kernel", base).spec()


def test_options_toml_records_the_flag(tmp_path):
    from deepcgp_amd import utils
    for i, (extra, want) in enumerate(((("--ard",), "ard = true"), ((), "ard = false"))):
        log = utils.Log(str(tmp_path), "run%d" % i, [])
        log.write_flags(_flags(*extra))
        log.close()
        assert want in (tmp_path / ("run%d" % i) / "options.toml").read_text().splitlines()


# ---- layers, parameters, checkpoints ----------------------------------------------------------------------------------------------------------
def test_builders_make_ard_layers_and_the_checkpoint_round_trip(monkeypatch, tmp_path):
    from deepcgp_amd.kernels import RBF
    from deepcgp_amd.models import build_from_spec, build_layers_from_spec, read_checkpoint, save_model_parameters
    np.random.seed(0)
    spec = _fill(_builder(monkeypatch, "--ard").spec())
    vec = 3.0 + np.arange(9.0)
    spec["convs"][0]["ls"] = vec
    with _NoPrior():
        model = build_from_spec(spec, np.zeros((4, 100)), np.zeros((4, 1), np.int64))
        scalar_layers = build_layers_from_spec(_fill(_builder(monkeypatch).spec()))
    k0, k1 = model.layers[0].base_kernel, model.layers[1].base_kernel
    assert type(k0) is RBF and k0.ARD and np.array_equal(k0.lengthscales, vec) and k0._describe() == [0.0, 5.0, 1.0, 0.0]
    assert k1.ARD and k1.lengthscales.shape == (36,) and not model.layers[2].kern.base_kernel.ARD
    assert not scalar_layers[0].base_kernel.ARD and scalar_layers[0].base_kernel.lengthscales == 5.0
    # gpflow's key, an [L] array
    path = str(tmp_path / "ckpt.npy")
    saved = save_model_parameters(model, path, global_step=3)
    assert np.array_equal(saved["DGP/layers/0/conv_kernel/base_kernel/lengthscales"], vec)
    step, rec = read_checkpoint(path, 3)
    assert step == 3 and np.array_equal(rec[0]["ls"], vec) and rec[1]["ls"].shape == (36,)
    np.random.seed(0)
    back = _builder(monkeypatch, "--ard", "--load-model", "ckpt", path=path).spec()
    assert np.array_equal(back["convs"][0]["ls"], vec) and np.shape(back["head"]["ls"]) == ()
    # a vector checkpoint without --ard is refused, naming the flag
    with pytest.raises(ValueError, match="--ard"):
        _builder(monkeypatch, "--load-model", "ckpt", path=path).spec()
    # a scalar checkpoint under --ard broadcasts
    raw = np.load(path, allow_pickle=True).item()
    raw["DGP/layers/0/conv_kernel/base_kernel/lengthscales"] = np.array(2.5)
    raw["DGP/layers/1/conv_kernel/base_kernel/lengthscales"] = np.array(1.5)
    np.save(path, raw)
    np.random.seed(0)
    back = _builder(monkeypatch, "--ard", "--load-model", "ckpt", path=path).spec()
    assert np.array_equal(back["convs"][0]["ls"], np.full(9, 2.5)) and np.array_equal(back["convs"][1]["ls"], np.full(36, 1.5))
    np.random.seed(0)
    assert _builder(monkeypatch, "--load-model", "ckpt", path=path).spec()["convs"][0]["ls"] == 2.5
    # a vector of another length is refused
    raw["DGP/layers/0/conv_kernel/base_kernel/lengthscales"] = np.ones(7)
    np.save(path, raw)
    with pytest.raises(ValueError, match="--ard"):
        _builder(monkeypatch, "--ard", "--load-model", "ckpt", path=path).spec()
    # the parameter's setter keeps the vector
    p = [p for p in model.parameters if p.pathname == "DGP/layers/0/conv_kernel/base_kernel/lengthscales"][0]
    p.assign(2.0 * vec)
    assert np.array_equal(model.layers[0].base_kernel.lengthscales, 2.0 * vec)
    # gradient / optimiser groups name the vector
    groups = {key: shape for key, _, _, shape in model._optimizer_groups()}
    assert groups["layers/0/ard_lengthscales"] == (9,) and groups["layers/1/ard_lengthscales"] == (36,) and "layers/2/ard_lengthscales" not in groups


def test_what_keeps_raising():
    from deepcgp_amd.kernels import AdditivePatchKernel, ArcCosine, ConvKernel, Matern32, Matern52, RBF
    from deepcgp_amd.views import FullView
    for cls in (Matern32, Matern52):
        with pytest.raises(NotImplementedError):
            cls(4, ARD=True)
    with pytest.raises(TypeError):
        ArcCosine(4, order=0, weight_variances=np.ones(4))
    view = FullView((7, 6, 2), 3, 2, 2)
    for cls in (ConvKernel, AdditivePatchKernel):
        with pytest.raises(NotImplementedError):
            cls(RBF(view.patch_length, 1.0, np.ones(view.patch_length), ARD=True), view).patch_mean(np.zeros((4, view.patch_length)), np.zeros((3, 84)),
                                                                                                   np.zeros((4, 2)))
    with pytest.raises(ValueError):
        RBF(9, 1.0, np.ones(8), ARD=True)                       # a wrong count
    with pytest.raises(ValueError):
        RBF(3, 1.0, [1.0, -1.0, 1.0], ARD=True)


def test_the_operator_entry_is_declared():
    import os
    import re
    from deepcgp_amd import device as dev
    assert "dcgp_kuf_patches_rbf_ard" in dev.declared_symbols()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dcgp.h")).read()
    assert re.search(r"int dcgp_kuf_patches_rbf_ard\(", header)


# ---- the references are live on every case the GPU tests use ------------------------------------------------------------------------------------
def test_ard_case_recipe():
    spec, X, Y, zs = ar.ard_case("small3_M20")
    plain = ls.make_case("small3_M20")[0]
    rng = np.random.default_rng(11)
    for c, p in zip(spec["convs"], plain["convs"]):
        L = c["f"] * c["f"] * c["C"]
        assert np.array_equal(c["ls"], p["ls"] * (0.8 + 0.4 * rng.random(L))) and np.array_equal(c["Z"], p["Z"])
    assert spec["head"]["ls"] == plain["head"]["ls"]
    assert set(ar.MEDIAN_GROUPS) == set(ls.MEDIAN_GROUPS) | {"lengthscales"} and set(ar.CAPPED_GROUPS) == set(ls.CAPPED_GROUPS) | {"lengthscales"}


@pytest.mark.parametrize("case", ar.CASES)
def test_reference_gradients_are_live(case):
    pytest.importorskip("torch")
    import matern_ref as mr
    spec, X, Y, zs = ar.ard_case(case)
    want = tr.reference(spec, X, Y, zs)["want"]
    for li, c in enumerate(spec["convs"]):
        assert want[li]["lengthscales"].shape == (c["f"] * c["f"] * c["C"],)
    ar.assert_live(case, want)


@pytest.mark.parametrize("cid", ar.COMPOSE_CASES)
def test_composed_reference_gradients_are_live(cid):
    pytest.importorskip("torch")
    import compose_cases as cc
    import compose_ref as cr
    spec, X, Y, zs, lik = cc.make_case(cc.BY_ID[cid])
    ar.ardify(spec)
    want = cr.reference(spec, X, Y, zs, lik)["want"]
    assert all(np.ndim(want[li]["lengthscales"]) == 1 for li in range(len(spec["convs"])))
    ar.assert_live(cid, want)


@pytest.mark.parametrize("name", ar.MIXING_CASES)
def test_mixing_reference_gradients_are_live(name):
    pytest.importorskip("torch")
    import mixing_ref as mx
    spec, X, Y, zs = mx.make_case(name)
    ar.ardify(spec)
    want = tr.reference(spec, X, Y, zs)["want"]
    assert all(np.ndim(want[li]["lengthscales"]) == 1 for li in range(len(spec["convs"])))
    ar.assert_live(name, want)

"""Mixed conv layers without a GPU: ``ConvLayer(..., mixing=W)``'s attributes and errors, ``mixing_matrix``, the flags --latent-gps /
--freeze-mixing through ModelBuilder.spec() with their errors, options.toml, the spec and checkpoint key round trip, the NumPy mirror of
csrc/mix.hip (tests/mixing_ref.py) against central differences, the two torch layer loops against each other, and the liveness of every case
tests/test_gpu_mixing.py uses, from the torch reference alone."""
import numpy as np
import pytest

import live_specs as ls
import mixing_ref as R
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


def _layer(mf=None, G=3, mixing=None, view=None):
    from deepcgp_amd.kernels import RBF, PatchInducingFeatures
    from deepcgp_amd.layers import ConvLayer
    from deepcgp_amd.views import FullView
    view = view or FullView((8, 8), 3, 2, 1)
    rng = np.random.default_rng(0)
    with _NoPrior():
        return ConvLayer(RBF(view.patch_length, 1.0, 1.0), mf, PatchInducingFeatures(rng.standard_normal((6, view.patch_length))), view,
                         gp_count=G, q_mu=np.zeros((6, G)), q_sqrt=np.tile(np.eye(6), (G, 1, 1)), mixing=mixing)


# ---- 1. the layer and mixing_matrix -----------------------------------------------------------------------------------------------------
def test_conv_layer_attributes_and_errors():
    from deepcgp_amd.mean_functions import Conv2dMean, LinearConv2dMean
    W = np.arange(15.0).reshape(3, 5)
    l = _layer(G=3, mixing=W)
    assert (l.gp_count, l.feature_maps_out, l.num_outputs, l.num_latent_outputs) == (3, 5, 36 * 5, 36 * 3) and np.array_equal(l.mixing, W)
    assert l.mixing is not W                                            # a copy
    u = _layer(G=3)
    assert (u.feature_maps_out, u.num_outputs, u.num_latent_outputs, u.mixing) == (3, 108, 108, None)
    for bad in (np.zeros((4, 5)), np.zeros(3), np.zeros((3, 0)), np.zeros((3, 5, 1))):
        with pytest.raises(ValueError, match="mixing"):
            _layer(G=3, mixing=bad)
    # the mean function lives on the R maps
    lin = LinearConv2dMean(3, 2, 5)
    assert _layer(lin, G=3, mixing=W).filter_mean is lin
    with pytest.raises(ValueError, match="does not match"):
        _layer(LinearConv2dMean(3, 2, 3), G=3, mixing=W)
    c = _layer(Conv2dMean(3, 2, 5), G=3, mixing=W)
    assert c.centre_mean and not c.identity_mean and c.generic_mean is None and c.filter_mean is None
    c = _layer(Conv2dMean(3, 2, 3), G=3)
    assert c.identity_mean and not c.centre_mean
    with pytest.raises(NotImplementedError, match="mixing"):
        l.conditional_ND(np.zeros((2, 128)), full_cov=True)
    with pytest.raises(ValueError, match="108"):                        # z is P * G per row
        l.sample_from_conditional(np.zeros((1, 2, 128)), z=np.zeros((1, 2, 180)))


def test_mixing_matrix():
    from deepcgp_amd.layers import mixing_matrix
    assert np.array_equal(mixing_matrix("identity", 4, 4), np.eye(4))
    with pytest.raises(ValueError, match="G == R"):
        mixing_matrix("identity", 3, 4)
    a, b, c = mixing_matrix("random", 3, 10, seed=2), mixing_matrix("random", 3, 10, seed=2), mixing_matrix("random", 3, 10, seed=3)
    assert a.shape == (3, 10) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(a, np.random.RandomState(2).standard_normal((3, 10)) / np.sqrt(3))
    assert np.array_equal(mixing_matrix("random", 3, 10), mixing_matrix("random", 3, 10, seed=0))
    for G in (2, 8):      # a map's variance is about a latent's: sum_g W[g, r]^2 ~ 1 (chi^2_G / G over 4000 maps: 5 standard errors)
        s = (mixing_matrix("random", G, 4000, seed=1) ** 2).sum(0)
        assert abs(s.mean() - 1.0) <= 5 * np.sqrt(2.0 / G / 4000), (G, s.mean())
    W = np.arange(6.0).reshape(2, 3)
    got = mixing_matrix(W, 2, 3)
    assert np.array_equal(got, W) and got is not W
    for bad in (lambda: mixing_matrix(W, 3, 2), lambda: mixing_matrix("ones", 2, 2), lambda: mixing_matrix("random", 0, 2)):
        with pytest.raises(ValueError, match="mixing_matrix"):
            bad()


# ---- 2. flags -> spec, options.toml, the checkpoint key ------------------------------------------------------------------------------------
def _flags(*extra):
    from deepcgp_amd.arguments import default_parser
    return default_parser().parse_args(["--name", "t", "-M", "5,6,7", "--feature-maps", "4,2", "--filter-sizes", "3,3,3", "--strides", "1,1,1",
                                        "--paddings", "1,1,0", "--num-samples", "2", "--batch-size", "4"] + list(extra))


def _builder(monkeypatch, *extra, path=None):
    from deepcgp_amd import kernels
    from deepcgp_amd.models import ModelBuilder
    monkeypatch.setattr(kernels, "kmeans", lambda sample, k, **kw: np.array(sample[:k]))      # (Lloyd's iterations run on the device)
    X = np.random.default_rng(0).standard_normal((30, 10, 10, 1))
    return ModelBuilder(_flags(*extra), X, np.zeros((30, 1)), model_path=path)


def test_flags_to_spec_and_their_errors(monkeypatch):
    from deepcgp_amd.arguments import default_parser, parse_latent_gps
    from deepcgp_amd.layers import mixing_matrix
    d = default_parser().parse_args(["--name", "x"])
    assert d.latent_gps == "" and d.freeze_mixing is False
    assert parse_latent_gps(d, 2) == [0, 0] and parse_latent_gps(_flags("--latent-gps", "3,0"), 2) == [3, 0]
    np.random.seed(0)
    plain = _builder(monkeypatch).spec()
    assert all("mix_W" not in c for c in plain["convs"]) and [c["R"] for c in plain["convs"]] == [4, 2]
    np.random.seed(0)
    spec = _builder(monkeypatch, "--latent-gps", "3,0").spec()
    c0, c1 = spec["convs"]
    assert c0["R"] == 3 and np.array_equal(c0["mix_W"], mixing_matrix("random", 3, 4, seed=0)) and c0["mix_trainable"] is True
    assert "mix_W" not in c1 and c1["R"] == 2 and c1["C"] == 4 and spec["head"]["C"] == 2
    for a, b in zip(plain["convs"] + [plain["head"]], spec["convs"] + [spec["head"]]):      # the initialisation images are what they were
        assert np.array_equal(a["Z"], b["Z"])
    np.random.seed(0)
    spec = _builder(monkeypatch, "--latent-gps", "3,5", "--freeze-mixing", "--identity-mean", "--mean-filter", "channels").spec()
    assert np.array_equal(spec["convs"][1]["mix_W"], mixing_matrix("random", 5, 2, seed=1)) and spec["convs"][1]["mix_trainable"] is False
    assert spec["convs"][0]["mean_filter"].shape == (3, 3, 1, 4) and spec["convs"][1]["mean_filter"].shape == (3, 3, 4, 2)
    for text in ("3", "3,3,3", "3,-1", "3,x", "1.5,2"):
        with pytest.raises(ValueError, match="--latent-gps"):
            _builder(monkeypatch, "--latent-gps", text).spec()


def test_options_toml_records_both_flags(tmp_path):
    from deepcgp_amd import utils
    for i, (extra, want) in enumerate(((("--latent-gps", "3,3", "--freeze-mixing"), ('latent_gps = "3,3"', "freeze_mixing = true")),
                                       ((), ('latent_gps = ""', "freeze_mixing = false")))):
        log = utils.Log(str(tmp_path), "run%d" % i, [])
        log.write_flags(_flags(*extra))
        log.close()
        lines = (tmp_path / ("run%d" % i) / "options.toml").read_text().splitlines()
        for w in want:
            assert w in lines, lines


def test_spec_and_checkpoint_key_round_trip(monkeypatch, tmp_path):
    """spec -> layers -> save_model_parameters -> read_checkpoint -> ModelBuilder.spec(): the same W; a checkpoint without the key builds the
    initial one."""
    from deepcgp_amd.layers import mixing_matrix
    from deepcgp_amd.models import CHECKPOINT_FIELDS, build_from_spec, read_checkpoint, save_model_parameters
    assert ("mixing/W", "mix_W") in CHECKPOINT_FIELDS
    np.random.seed(0)
    spec = _builder(monkeypatch, "--latent-gps", "3,0").spec()
    W = np.random.default_rng(3).standard_normal((3, 4))
    spec["convs"][0]["mix_W"] = W
    for l in spec["convs"] + [spec["head"]]:
        l["q_mu"] = np.zeros((l["M"], l["R"]))
        l["q_sqrt"] = np.tile(np.eye(l["M"]), (l["R"], 1, 1))
    spec["head"]["w"] = np.ones(64)
    with _NoPrior():
        model = build_from_spec(spec, np.zeros((4, 100)), np.zeros((4, 1), np.int64))
    l0, l1 = model.layers[:2]
    assert np.array_equal(l0.mixing, W) and l0.mixing_trainable is True and l0.feature_maps_out == 4 and l1.mixing is None
    names = [p.pathname for p in model.parameters]
    assert "DGP/layers/0/mixing/W" in names and "DGP/layers/1/mixing/W" not in names
    path = str(tmp_path / "ckpt.npy")
    save_model_parameters(model, path, global_step=5)
    step, rec = read_checkpoint(path, 3)
    assert step == 5 and np.array_equal(rec[0]["mix_W"], W) and "mix_W" not in rec[1] and "mix_W" not in rec[2]
    np.random.seed(0)
    back = _builder(monkeypatch, "--latent-gps", "3,0", "--load-model", "ckpt", path=path).spec()
    assert np.array_equal(back["convs"][0]["mix_W"], W)
    raw = np.load(path, allow_pickle=True).item()
    del raw["DGP/layers/0/mixing/W"]                       # such as the reference's
    np.save(path, raw)
    np.random.seed(0)
    back = _builder(monkeypatch, "--latent-gps", "3,0", "--load-model", "ckpt", path=path).spec()
    assert np.array_equal(back["convs"][0]["mix_W"], mixing_matrix("random", 3, 4, seed=0))
    # the setter of the parameter keeps the shape
    p = [p for p in model.parameters if p.pathname.endswith("mixing/W")][0]
    p.assign(np.arange(12.0))
    assert l0.mixing.shape == (3, 4) and l0.mixing[2, 3] == 11.0
    with pytest.raises(ValueError, match="mix_W"):
        from deepcgp_amd.models import build_layers_from_spec
        spec["convs"][0]["mix_W"] = np.zeros((2, 4))
        build_layers_from_spec(spec)


# ---- 3. the NumPy mirror ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,G,Rm", [(70, 3, 5), (33, 4, 2), (40, 1, 3), (1100, 3, 3)])
def test_mirror_backward_against_central_differences(K, G, Rm):
    """L = sum(sample * A) + sum(mean * B) + sum(var * C): d L / d u = mirror_backward_latent(W, A); d L / d W through the sample =
    mirror_backward_w(u, A).  Central differences with h = 1e-5 on a bilinear / quadratic form: error ~ h^2 |third derivative| = 0 here, so the
    bound is rounding, 1e-8 relative."""
    rng = np.random.default_rng(K)
    W, u, gm, gv = rng.standard_normal((G, Rm)), rng.standard_normal((K, G)), rng.standard_normal((K, G)), rng.random((K, G))
    A = rng.standard_normal((K, Rm))
    s, m, v = R.mirror_forward(W, u, gm, gv)
    assert np.allclose(s, u @ W, rtol=1e-13, atol=1e-13) and np.allclose(m, gm @ W, rtol=1e-13, atol=1e-13) and np.allclose(v, gv @ (W * W), rtol=1e-13, atol=1e-13)
    assert R.mirror_forward(W, None, gm, None)[0] is None and R.mirror_forward(W, None, gm, None)[2] is None
    loss = lambda W_, u_: float((R.mirror_forward(W_, u_, None, None)[0] * A).sum())      # noqa: E731
    gu, gW = R.mirror_backward_latent(W, A), R.mirror_backward_w(u, A)
    assert np.allclose(gW, u.T @ A, rtol=1e-12, atol=1e-12)
    h = 1e-5
    for (i, j) in [(0, 0), (K // 2, G - 1), (K - 1, 0)]:
        d = np.zeros_like(u)
        d[i, j] = h
        fd = (loss(W, u + d) - loss(W, u - d)) / (2 * h)
        assert abs(fd - gu[i, j]) <= 1e-8 * max(1.0, abs(gu[i, j])), (i, j, fd, gu[i, j])
    for (g, r) in [(0, 0), (G - 1, Rm - 1)]:
        d = np.zeros_like(W)
        d[g, r] = h
        fd = (loss(W + d, u) - loss(W - d, u)) / (2 * h)
        assert abs(fd - gW[g, r]) <= 1e-8 * max(1.0, abs(gW[g, r])), (g, r, fd, gW[g, r])
    assert R.w_plan(216) == (7, 32) and R.w_plan(525) == (17, 32) and R.w_plan(40000) == (625, 64)


def test_the_two_torch_loops_agree_on_an_unmixed_layer():
    """torch_ref.forward's mixed branch with W = I against its unmixed branch on the same spec without the mixing: ELBO parts to 1e-13."""
    torch = pytest.importorskip("torch")
    for name in ("a_3_3", "pad_lin"):
        spec, X, Y, zs = R.make_case(name, **({"G": 5} if name == "pad_lin" else {}))
        G = spec["convs"][0]["R"]
        eye = R.with_mixing(spec, [np.eye(G)])
        plain = R.copy.deepcopy(eye)
        del plain["convs"][0]["mix_W"]
        with torch.no_grad():
            a, b = tr.forward(eye, X, Y, zs), tr.forward(plain, X, Y, zs)
        for k in ("elbo", "kl"):
            assert abs(a[k].item() - b[k].item()) <= 1e-13 * abs(b[k].item()), (name, k)
        assert torch.allclose(a["F"][0], b["F"][0], rtol=1e-13, atol=1e-13)


# ---- 4. liveness of the GPU file's cases, from the torch reference alone --------------------------------------------------------------------
def gpu_cases():
    """(id, make_case arguments) of every case tests/test_gpu_mixing.py runs."""
    out = [(name, dict(name=name)) for name in R.CASES]
    out += [("%s_%s" % (name, base), dict(name=name, base=base)) for name, bases in R.BASES.items() for base in bases]
    return out


@pytest.mark.parametrize("cid,kw", gpu_cases(), ids=[c for c, _ in gpu_cases()])
def test_gpu_cases_are_live(cid, kw):
    pytest.importorskip("torch")
    spec, X, Y, zs = R.make_case(**kw)
    t = tr.reference(spec, X, Y, zs)
    elbo, want = t["parts"][0], t["want"]
    mixed = [li for li, c in enumerate(spec["convs"]) if c.get("mix_W") is not None]
    assert mixed
    for li in mixed:
        top = np.abs(want[li]["mixing"]).max()
        print("%s layer %d |gW|max %.3e" % (cid, li, top))
        assert top >= ls.LIVE_MAX, (cid, li, top)
    ls.assert_live(cid, want)
    other = tr.reference(R.reseeded(spec), X, Y, zs)["parts"][0]
    rel = abs(other - elbo) / abs(elbo)
    print("%s ELBO %.9g, with the next seed's W %.9g: %.3e" % (cid, elbo, other, rel))
    assert rel > 1e-3, (cid, elbo, other)

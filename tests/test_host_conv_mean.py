"""The linear convolutional mean function without a GPU: the NumPy reference (tests/conv_mean_ref.py) against torch's conv2d and its autograd,
the named filters, how ConvLayer classifies a ``LinearConv2dMean``, the flags --mean-filter / --train-mean through ModelBuilder.spec() with
their errors, options.toml, the checkpoint key, the initialisation images of a ``channels`` model, and the two gradient references of
tests/test_gpu_conv_mean.py against each other."""
import argparse

import numpy as np
import pytest

import conv_mean_ref as R
import torch_ref as tr


# ---- 1. the reference itself --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,C,f,s,Rm", [(9, 7, 3, 4, 2, 3), (8, 8, 1, 3, 1, 17)])
def test_reference_matches_torch_conv2d_and_its_autograd(H, W, C, f, s, Rm):
    """output, dX and dW at 1e-12 (relative to the largest entry)"""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(H * 100 + Rm)
    N = 3
    X, Wf = rng.standard_normal((N, H, W, C)), rng.standard_normal((f, f, C, Rm))
    Ho, Wo = (H - f) // s + 1, (W - f) // s + 1
    g = rng.standard_normal((N, Ho * Wo * Rm))
    m = R.RefConvMean(Wf, s)
    out = m(X)
    dX = m.backward(X, g)
    dW = m.filter_grad()
    Xt = torch.tensor(X, dtype=torch.float64, requires_grad=True)
    Wt = torch.tensor(Wf, dtype=torch.float64, requires_grad=True)
    # NHWC x [f, f, Cin, Cout] -> NCHW x [Cout, Cin, f, f]; the result back to N x (P Cout), patch-major
    y = torch.nn.functional.conv2d(Xt.permute(0, 3, 1, 2), Wt.permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1).reshape(N, -1)
    gx, gw = torch.autograd.grad((y * torch.tensor(g)).sum(), [Xt, Wt])
    for what, a, b in (("out", out, y.detach().numpy()), ("dX", dX, gx.numpy()), ("dW", dW, gw.numpy())):
        err = np.abs(a - b).max() / np.abs(b).max()
        print("%s %.3e" % (what, err))
        assert a.shape == b.shape and err <= 1e-12, (what, err)
    assert out.shape == (N, Ho * Wo * Rm)
    m.backward(X, g)                                     # two recorded calls: the sum
    assert np.allclose(m.filter_grad(), 2.0 * dW, rtol=1e-14, atol=0.0)
    m.reset()
    assert not m.filter_grad().any()


def test_named_filters():
    from deepcgp_amd.mean_functions import Conv2dMean, IdentityConv2dMean, LinearConv2dMean, conv_mean_filter
    assert np.array_equal(conv_mean_filter("centre0", 5, 3, 4), Conv2dMean(5, 3, 4).conv_filter)
    assert np.array_equal(conv_mean_filter("sum", 5, 3, 4), IdentityConv2dMean(5, 3, 4).conv_filter)
    for Cin, Cout in ((3, 4), (4, 3), (2, 2)):
        W = conv_mean_filter("channels", 3, Cin, Cout)
        assert W.shape == (3, 3, Cin, Cout) and W.sum() == min(Cin, Cout)
        assert all(W[1, 1, c, c] == 1.0 for c in range(min(Cin, Cout)))
    for kind in ("centre0", "channels", "sum"):
        with pytest.raises(ValueError, match="odd"):
            conv_mean_filter(kind, 4, 1, 1)
    with pytest.raises(ValueError, match="expected one of"):
        conv_mean_filter("identity", 3, 1, 1)
    m = LinearConv2dMean(3, 2, 2)
    assert np.array_equal(m.conv_filter, conv_mean_filter("channels", 3, 2, 2)) and m.trainable is False and m.stride == 1
    m.set_trainable(True)
    assert m.trainable is True
    W = np.arange(4 * 4 * 3 * 2, dtype=np.float64).reshape(4, 4, 3, 2)
    assert np.array_equal(LinearConv2dMean(4, 3, 2, stride=2, filter=W, trainable=True).conv_filter, W)      # an array may have an even f
    with pytest.raises(ValueError, match="array"):
        LinearConv2dMean(3, 3, 2, filter=W)
    with pytest.raises(ValueError, match="odd"):
        LinearConv2dMean(4, 3, 2, filter="channels")


def test_conv_layer_classifies_a_linear_mean():
    """``filter_mean`` is the object, ``identity_mean`` False and ``generic_mean`` None; another geometry than the view's raises at construction."""
    from deepcgp_amd.kernels import RBF, PatchInducingFeatures
    from deepcgp_amd.layers import ConvLayer
    from deepcgp_amd.mean_functions import Conv2dMean, LinearConv2dMean
    from deepcgp_amd.views import FullView

    class Stub(ConvLayer):           # the classification needs no device: skip the prior factorisation
        def _build_prior_cholesky(self):
            pass
    rng = np.random.default_rng(0)
    view = FullView((9, 9), 5, 3, 2)
    mk = lambda mf: Stub(RBF(view.patch_length, 1.0, 1.0), mf, PatchInducingFeatures(rng.standard_normal((6, view.patch_length))),   # noqa: E731
                         view, gp_count=4, q_mu=np.zeros((6, 4)), q_sqrt=np.tile(np.eye(6), (4, 1, 1)))
    lin = LinearConv2dMean(5, 3, 4, stride=2, filter="centre0")
    layer = mk(lin)
    assert layer.filter_mean is lin and not layer.identity_mean and layer.generic_mean is None
    assert mk(Conv2dMean(5, 3, 4, stride=2)).filter_mean is None and mk(None).filter_mean is None
    for bad in (LinearConv2dMean(3, 3, 4, stride=2), LinearConv2dMean(5, 3, 4, stride=1), LinearConv2dMean(5, 2, 4, stride=2),
                LinearConv2dMean(5, 3, 3, stride=2)):
        with pytest.raises(ValueError, match="does not match"):
            mk(bad)


# ---- 2. flags -> spec ---------------------------------------------------------------------------------------------------------------
def _flags(*extra):
    from deepcgp_amd.arguments import default_parser
    return default_parser().parse_args(["--name", "t", "-M", "5,6,7", "--feature-maps", "2,2", "--filter-sizes", "3,3,3", "--strides", "1,1,1",
                                        "--paddings", "1,1,0", "--num-samples", "2", "--batch-size", "4"] + list(extra))


def _builder(monkeypatch, *extra, X=None):
    from deepcgp_amd import kernels
    from deepcgp_amd.models import ModelBuilder
    monkeypatch.setattr(kernels, "kmeans", lambda sample, k, **kw: np.array(sample[:k]))      # (Lloyd's iterations run on the device)
    X = np.random.default_rng(0).standard_normal((30, 10, 10, 1)) if X is None else X
    return ModelBuilder(_flags(*extra), X, np.zeros((X.shape[0], 1)))


def test_flags_to_spec_and_their_errors(monkeypatch):
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.mean_functions import conv_mean_filter
    d = default_parser().parse_args(["--name", "x"])
    assert d.mean_filter == "centre0" and d.train_mean is False
    # the defaults: the objects and the device path of before
    assert _builder(monkeypatch).mean_flags() == (None, False)
    assert _builder(monkeypatch, "--identity-mean").mean_flags() == ("conv2d", False)
    np.random.seed(0)
    spec = _builder(monkeypatch, "--identity-mean").spec()
    assert all(c["mean_function"] == "conv2d" and "mean_filter" not in c for c in spec["convs"])
    np.random.seed(0)
    assert all(c["mean_function"] is None and "mean_filter" not in c for c in _builder(monkeypatch).spec()["convs"])
    # a LinearConv2dMean: any other filter, and centre0 itself once it is trained
    for extra, kind, train in ((("--mean-filter", "channels"), "channels", False), (("--mean-filter", "sum", "--train-mean"), "sum", True),
                               (("--train-mean",), "centre0", True)):
        b = _builder(monkeypatch, "--identity-mean", *extra)
        assert b.mean_flags() == (kind, train)
        np.random.seed(0)
        spec = b.spec()
        for c in spec["convs"]:
            assert c["mean_function"] is None and c["mean_trainable"] is train
            assert np.array_equal(c["mean_filter"], conv_mean_filter(kind, c["f"], c["C"], c["R"]))
    for extra, flag in ((("--mean-filter", "channels"), "--mean-filter"), (("--mean-filter", "sum", "--train-mean"), "--mean-filter"),
                        (("--train-mean",), "--train-mean"), (("--identity-mean", "--mean-filter", "identity"), "--mean-filter")):
        with pytest.raises(ValueError, match=flag):
            _builder(monkeypatch, *extra).spec()
    from deepcgp_amd.models import ModelBuilder
    even = default_parser().parse_args(["--name", "t", "-M", "5,6", "--feature-maps", "2", "--filter-sizes", "4,3", "--strides", "1,1",
                                        "--identity-mean", "--mean-filter", "channels"])
    with pytest.raises(ValueError, match="odd"):
        ModelBuilder(even, np.zeros((30, 10, 10, 1)), np.zeros((30, 1))).spec()


def test_initialisation_images_of_a_channels_model(monkeypatch):
    """10 x 10 x 1 -> f3 s1 p1 R2 -> f3 s1 p1 R2 -> head.  Behind layer 0 the images are (x, 0): channel 0 skipped to map 0, nothing into map 1
    -- not identity_conv's (x, x); so layer 1's inducing patches are zero in channel 1, and the head's as well."""
    from deepcgp_amd import models
    seen = []
    real = models.filter_conv
    monkeypatch.setattr(models, "filter_conv", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    X = np.random.default_rng(1).standard_normal((30, 10, 10, 1)) + 3.0
    np.random.seed(0)
    spec = _builder(monkeypatch, "--identity-mean", "--mean-filter", "channels", X=X).spec()
    assert [s.shape for s in seen] == [(30, 10, 10, 2), (30, 10, 10, 2)]
    assert not seen[0][..., 1].any() and seen[0][..., 0].any()
    for imgs in seen:                                         # every image of map 0 is one of the training images (stride 1, padding 1: same size)
        assert all(any(np.array_equal(im[..., 0], x[..., 0]) for x in X) for im in imgs[:5])
    Z1 = spec["convs"][1]["Z"].reshape(-1, 3, 3, 2)
    assert not Z1[..., 1].any() and Z1[..., 0].any()
    assert not spec["head"]["Z"].reshape(-1, 3, 3, 2)[..., 1].any()
    # the same draw as identity_conv makes: centre0 keeps identity_conv (the sum filter), whose two maps are equal
    np.random.seed(0)
    spec0 = _builder(monkeypatch, "--identity-mean", X=X).spec()
    Z1 = spec0["convs"][1]["Z"].reshape(-1, 3, 3, 2)
    assert np.array_equal(Z1[..., 0], Z1[..., 1]) and np.array_equal(spec0["convs"][0]["Z"], spec["convs"][0]["Z"])


def test_filter_conv_is_the_reference_convolution():
    from deepcgp_amd.models import filter_conv
    rng = np.random.default_rng(2)
    X, W = rng.standard_normal((5, 9, 7, 3)), rng.standard_normal((4, 4, 3, 2))
    np.random.seed(4)
    pick = np.random.choice(np.arange(5), size=5)
    np.random.seed(4)
    got = filter_conv(X, W, 2)
    want = R.RefConvMean(W, 2)(X[pick]).reshape(5, 3, 2, 2)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def test_options_toml_records_both_flags(tmp_path):
    from deepcgp_amd import utils
    for i, (extra, want) in enumerate(((("--identity-mean", "--mean-filter", "channels", "--train-mean"), ('mean_filter = "channels"', "train_mean = true")),
                                       ((), ('mean_filter = "centre0"', "train_mean = false")))):
        log = utils.Log(str(tmp_path), "run%d" % i, [])
        log.write_flags(_flags(*extra))
        log.close()
        lines = (tmp_path / ("run%d" % i) / "options.toml").read_text().splitlines()
        for w in want:
            assert w in lines, lines
        try:
            import tomli
        except ImportError:
            continue
        back = argparse.Namespace(**tomli.loads("\n".join(lines)))
        assert (back.mean_filter, back.train_mean) == (_flags(*extra).mean_filter, _flags(*extra).train_mean)


def test_checkpoint_key_through_read_checkpoint(tmp_path):
    from deepcgp_amd.models import CHECKPOINT_FIELDS, read_checkpoint
    assert ("mean_function/conv_filter", "mean_filter") in CHECKPOINT_FIELDS
    W0, W1 = np.arange(18.0).reshape(3, 3, 1, 2), np.arange(36.0).reshape(3, 3, 2, 2)
    raw = {"DGP/layers/0/mean_function/conv_filter": W0, "DGP/layers/1/mean_function/conv_filter": W1, "DGP/layers/0/q_mu": np.zeros((5, 2)),
           "DGP/layers/2/q_mu": np.zeros((7, 10)), "global_step": 12}
    path = str(tmp_path / "ckpt.npy")
    np.save(path, raw)
    step, rec = read_checkpoint(path, 3)
    assert step == 12 and np.array_equal(rec[0]["mean_filter"], W0) and np.array_equal(rec[1]["mean_filter"], W1) and "mean_filter" not in rec[2]


def test_model_builder_takes_the_checkpoints_filter(monkeypatch, tmp_path):
    from deepcgp_amd.models import ModelBuilder
    W0 = np.random.default_rng(5).standard_normal((3, 3, 1, 2))
    path = str(tmp_path / "ckpt.npy")
    np.save(path, {"DGP/layers/0/mean_function/conv_filter": W0, "DGP/layers/2/kern/base_kernel/variance": np.array(4.0), "global_step": 3})
    b = _builder(monkeypatch, "--identity-mean", "--mean-filter", "channels", "--train-mean", "--load-model", "ckpt")
    b = ModelBuilder(b.flags, b.X_train, b.Y_train, model_path=path)
    np.random.seed(0)
    spec = b.spec()
    assert np.array_equal(spec["convs"][0]["mean_filter"], W0) and b.global_step == 3
    assert spec["convs"][1]["mean_filter"].sum() == 2.0                      # (not in the checkpoint: the named filter)


# ---- 3. the two gradient references ---------------------------------------------------------------------------------------------------
def test_oracle_gradient_with_filter_grad_matches_torch_autograd():
    """On the unpadded two-layer stack: oracle.grad.elbo_and_grad (unmodified, RefConvMean attached) plus filter_grad() against autograd of the
    torch forward with the mean as a leaf -- every group, the bound of tests/test_oracle_autograd.py."""
    pytest.importorskip("torch")
    spec, X, Y, zs = R.make_case("valid2")
    e_o, g_o = R.oracle_gradient(spec, X, Y, zs)
    t = tr.reference(spec, X, Y, zs)
    e_t, g_t = t["parts"][0], t["want"]
    assert abs(e_t - e_o) <= 1e-10 * abs(e_o)
    for li, groups in enumerate(g_t):
        assert set(groups) == set(g_o[li]), (li, sorted(groups), sorted(g_o[li]))
        for name, want in groups.items():
            got = np.asarray(g_o[li][name], np.float64)
            got = np.tril(got) if name == "q_sqrt" else got
            err = np.abs(got - want).max()
            print("L%d %-14s %.3e (|want|max %.3e)" % (li, name, err, np.abs(want).max()))
            assert err <= 1e-9 * max(1.0, np.abs(want).max()), (li, name, err)
    assert all("mean_filter" in g for g in g_t[:-1]) and np.abs(g_t[0]["mean_filter"]).max() > 1e-3


@pytest.mark.parametrize("name", ["ch_res", "even_s2"])
def test_oracle_forward_with_the_mean_matches_the_torch_forward(name):
    torch = pytest.importorskip("torch")
    spec, X, Y, zs = R.make_case(name)
    ref, _ = R.oracle_model(spec, X, Y)
    with torch.no_grad():
        out = tr.forward(spec, X, Y, zs)
    got = (ref.compute_log_likelihood(X, Y, zs=zs), ref.data_term(X, Y, zs=zs), ref.KL())
    want = (out["elbo"].item(), out["data"].sum().item(), out["kl"].item())
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-9 * abs(w), (name, got, want)
    no_mean = R.pr.oracle_model(R.without_filters(spec), X, Y).compute_log_likelihood(X, Y, zs=zs)
    assert abs(no_mean - got[0]) > 1e-3 * abs(got[0])           # the mean is live in the case

"""GPU: the Gaussian likelihood end to end (csrc/pointwise.hip) -- ELBO, gradient, optimiser slot, predictions, evaluation,
learning and checkpoints -- against the oracle's propagate with a NumPy Gaussian tail and torch autograd; plus head widths D = 1 / 3."""
import ctypes as C
import os

import numpy as np
import pytest

from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.likelihoods import Gaussian, MultiClass
from deepcgp_amd.models import AccuracyLogger, TestLogDensityLogger, build_from_spec, save_model_parameters, train
from oracle_build import oracle_model

pytestmark = pytest.mark.gpu

LOG2PI = np.log(2 * np.pi)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def make_case(case, D, white=False, N=5, S=3, seed=7):
    hwc = (10, 10, 1)
    kw = dict(S=S, num_data=300, seed=seed, white=white, conv_q_sqrt_scale=0.3, variance=2.0, ls=1.5, head_outputs=D)
    if case == "conv":
        spec = syn.make_spec(hwc, [(3, 1, 2)], (3, 1), 9, **kw)
    elif case == "head_only":
        spec = syn.make_spec(hwc, [], (3, 1), 9, **kw)
    elif case == "dense_ard":
        spec = syn.make_spec(hwc, [(3, 1, 2)], (3, 1), 9, head_kernel="rbf", **kw)
    elif case == "acos":
        spec = syn.make_spec(hwc, [(3, 1, 2)], (3, 1), 9, base_kernel="acos", **kw)
    X, Ylab = syn.make_batch(hwc, N, seed=seed)
    Y = np.random.default_rng(seed).standard_normal((N, D))
    zs = syn.make_noise(spec, N, seed=seed)
    return spec, X, Ylab, Y, zs


def numpy_elbo(spec, X, Ylab, Y, zs, s2):
    ref = oracle_model(spec, X, Ylab)
    S, N = spec["S"], X.shape[0]
    _, Fm, Fv = ref.propagate(X, S=S, zs=zs)
    m, v = Fm[-1], Fv[-1]
    ve = -0.5 * (LOG2PI + np.log(s2)) - 0.5 * (np.square(Y[None] - m) + v) / s2     # [S, N, D]
    data = ve.sum(2).mean(0).sum()
    kl = sum(l.KL() for l in ref.layers)
    return data * spec["num_data"] / N - kl, data, kl


@pytest.mark.parametrize("case,D,white", [("conv", 10, False), ("conv", 10, True), ("head_only", 3, False), ("dense_ard", 3, False),
                                          ("acos", 3, False), ("conv", 1, False), ("conv", 3, True), ("dense_ard", 1, True)])
@pytest.mark.parametrize("dedup", [False, True])
def test_elbo_vs_numpy(ctx, case, D, white, dedup):
    spec, X, Ylab, Y, zs = make_case(case, D, white)
    s2 = 0.7
    want, wdata, wkl = numpy_elbo(spec, X, Ylab, Y, zs, s2)
    model = build_from_spec(spec, X, Y, likelihood=Gaussian(s2))
    model.dedup_layer0 = dedup
    e, data, kl = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    assert abs(e - want) <= 1e-10 * abs(want), (e, want)
    assert abs(data - wdata) <= 1e-10 * abs(wdata)
    # (the KL is the RobustMax route's own; ArcCosine's K_uu factorisation is the least well conditioned of the cases: 3e-10 there)
    assert abs(kl - wkl) <= (1e-9 if case == "acos" else 1e-10) * abs(wkl)
    # the enqueue / collect halves: bit-identical to the synchronous call
    t = model.enqueue_log_likelihood(X, Y, zs=zs)
    assert model.collect_log_likelihood(t, return_parts=True) == (e, data, kl)
    model.close()


@pytest.mark.parametrize("case,D", [("conv", 1), ("conv", 3), ("dense_ard", 1), ("head_only", 3), ("dense_ard", 3)])
@pytest.mark.parametrize("dedup", [False, True])
def test_head_marginals_at_other_widths(ctx, case, D, dedup):
    """Regression heads at D = 1 and 3 through head_cond / the GEMM route / propagate / the dedup and RNG paths: the oracle's marginals."""
    spec, X, Ylab, Y, zs = make_case(case, D)
    ref = oracle_model(spec, X, Ylab)
    _, om, ov = ref.propagate(X, S=spec["S"], zs=zs)
    model = build_from_spec(spec, X, Ylab)
    model.dedup_layer0 = dedup
    _, gm, gv = model.propagate(X, S=spec["S"], zs=zs)
    for li in range(len(om)):
        assert gm[li].shape == om[li].shape
        assert rel(gm[li], om[li]) < 1e-9 and rel(gv[li], ov[li]) < 1e-9, li
    # device RNG: the same seed twice gives the same draws at these widths too
    a = model.propagate(X, S=spec["S"], seed=3)[0][-1]
    b = model.propagate(X, S=spec["S"], seed=3)[0][-1]
    assert np.array_equal(a, b) and np.all(np.isfinite(a))
    model.close()


def _spec(D):
    return syn.make_spec((10, 10, 1), [(3, 1, 2)], (3, 1), 9, S=2, num_data=100, seed=1, head_outputs=D)


def test_targets_and_parameters(ctx):
    X, lab = syn.make_batch((10, 10, 1), 4, seed=1)
    Y = np.random.default_rng(1).standard_normal((4, 3))
    m = build_from_spec(_spec(3), X, Y, likelihood=Gaussian(0.5))
    assert m.gaussian and m.Y.dtype == np.float64 and m.Y.shape == (4, 3)
    names = [p.pathname for p in m.parameters]
    assert names[0] == "DGP/likelihood/likelihood/variance" and "DGP/likelihood/likelihood/invlink/epsilon" not in names
    m.parameters[0].assign(0.25)
    assert m.likelihood.variance == 0.25
    with pytest.raises(ValueError):
        build_from_spec(_spec(3), X, Y[:, :2], likelihood=Gaussian(0.5))
    one = build_from_spec(_spec(1), X, Y[:, 0], likelihood=Gaussian(0.5))     # D = 1 accepts a flat target vector
    assert one.Y.shape == (4, 1)
    # every other likelihood keeps today's route: int32 labels
    rm = build_from_spec(_spec(10), X, lab)
    assert not rm.gaussian and rm.Y.dtype == np.int32 and isinstance(rm.likelihood, MultiClass)


def _torch_gauss_rule(m, v, yt, s2t):
    """E_q[log N(y; f, s2)] in closed form on tensors m, v, yt of one (broadcast) shape; shared with tests/compose_ref.py."""
    import torch
    return -0.5 * torch.log(2 * np.pi * s2t) - 0.5 * ((yt - m) ** 2 + v) / s2t


def _torch_gauss(spec, X, Ylab, Y, zs, s2):
    import torch
    import test_oracle_autograd as ta
    Ylab = np.asarray(Ylab) % Y.shape[1]          # (labels of the RobustMax forward the KL is recovered from)
    e_rm, leaves, m, v = ta._torch_elbo(spec, X, Ylab, zs, want_head=True)
    S, N = spec["S"], X.shape[0]
    y = torch.tensor(np.tile(np.asarray(Ylab).reshape(1, N), [S, 1]).reshape(S * N), dtype=torch.long)
    ve_rm = ta._robustmax_ve(m.reshape(S * N, -1), v.reshape(S * N, -1), y).reshape(S, N).mean(0).sum()
    kl = ve_rm * (spec["num_data"] / N) - e_rm
    s2t = torch.tensor(s2, dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(Y, dtype=torch.float64)[None]
    ve = _torch_gauss_rule(m, v, yt, s2t)
    e = ve.sum(2).mean(0).sum() * (spec["num_data"] / N) - kl
    return e, leaves, s2t


@pytest.mark.parametrize("case", ["conv", "dense_ard"])
def test_gradient_vs_torch_autograd(ctx, case):
    torch = pytest.importorskip("torch")
    spec, X, Ylab, Y, zs = make_case(case, 3, N=3, S=2, seed=11)
    s2 = 0.6
    e_t, leaves, s2t = _torch_gauss(spec, X, Ylab, Y, zs, s2)
    flat = [(li, k, t) for li, p in enumerate(leaves) for k, t in p.items()]
    grads = torch.autograd.grad(e_t, [t for _, _, t in flat] + [s2t])
    model = build_from_spec(spec, X, Y, likelihood=Gaussian(s2))
    e, g = model.compute_gradients(X, Y, zs=zs)
    assert abs(e - e_t.item()) <= 1e-10 * abs(e_t.item())
    for (li, name, _), gt in zip(flat, grads[:-1]):
        want, got = gt.numpy(), g[li][name]
        if name == "q_sqrt":
            want, got = np.tril(want), np.tril(got)
        assert np.abs(got - want).max() <= 1e-8 * max(1.0, np.abs(want).max()), (li, name)
    want = grads[-1].item()
    assert abs(g[-1]["likelihood_variance"] - want) <= 1e-8 * max(1.0, abs(want))
    # two identical calls: bitwise identical gradient blocks (the s2 slot included)
    L = dev.lib()
    blocks = []
    for _ in range(2):
        model.compute_gradients(X, Y, zs=zs, fetch=False)
        ptr, n = C.c_void_p(), C.c_size_t()
        ctx._check(L.dcgp_model_grad_block(model._model, len(model.layers) - 1, C.byref(ptr), C.byref(n)))
        host = np.empty(n.value)
        ctx._check(L.dcgp_d2h(ctx.handle, host.ctypes.data, ptr, host.nbytes))
        blocks.append(host)
    assert np.array_equal(blocks[0], blocks[1])
    assert blocks[0][-1] == g[-1]["likelihood_variance"]
    model.close()


def _params(model):
    model.pull_parameters()
    out = {}
    for li, l in enumerate(model.layers):
        head = li == len(model.layers) - 1
        kern = (l.kern.base_kernel if hasattr(l.kern, "base_kernel") else l.kern) if head else l.base_kernel
        out[(li, "Z")], out[(li, "q_mu")], out[(li, "q_sqrt")] = np.array(l.feature.Z), np.array(l.q_mu), np.array(l.q_sqrt)
        out[(li, "variance")], out[(li, "lengthscales")] = np.array(kern.variance), np.array(kern.lengthscales)
        if head and hasattr(l.kern, "patch_weights"):
            out[(li, "patch_weights")] = np.array(l.kern.patch_weights)
    out[(len(model.layers) - 1, "likelihood_variance")] = np.array(model.likelihood.variance)
    return out


POSITIVE = ("variance", "lengthscales", "likelihood_variance")


def test_train_step_equals_numpy_adam(ctx):
    spec, X, Ylab, Y, zs = make_case("conv", 3, N=4, S=2, seed=3)
    lr, b1, b2, eps = 0.01, 0.9, 0.999, 1e-8
    a = build_from_spec(spec, X, Y, likelihood=Gaussian(0.8))
    _, g = a.compute_gradients(X, Y, zs=zs)
    before = _params(a)
    b = build_from_spec(spec, X, Y, likelihood=Gaussian(0.8))
    b.train_step(X, Y, lr, zs=zs)
    after = _params(b)
    lr_t = lr * np.sqrt(1 - b2) / (1 - b1)
    for (li, name), x in before.items():
        gr = -np.asarray(g[li][name], np.float64)
        u = x
        if name in POSITIVE:
            y = x - 1e-6
            u = np.log(np.expm1(y))
            gr = gr * -np.expm1(-y)
        m, v = (1 - b1) * gr, (1 - b2) * gr * gr
        u = u - lr_t * m / (np.sqrt(v) + eps)
        want = np.log1p(np.exp(u)) + 1e-6 if name in POSITIVE else u
        assert np.allclose(after[(li, name)], want, rtol=1e-10, atol=1e-13), (li, name)
    assert after[(len(b.layers) - 1, "likelihood_variance")] > 0
    assert after[(len(b.layers) - 1, "likelihood_variance")] != 0.8
    # switched off, s2 does not move (the rest still does)
    b.set_trainable(0, "likelihood_variance", False)
    s2 = b.likelihood.variance
    b.train_step(X, Y, lr, zs=zs)
    after2 = _params(b)
    assert after2[(len(b.layers) - 1, "likelihood_variance")] == s2
    assert not np.array_equal(after2[(0, "Z")], after[(0, "Z")])
    a.close(), b.close()


@pytest.mark.parametrize("ranks", [2, 3])
def test_sharded_adam_carries_the_variance_slot(ctx, ranks):
    spec, X, Ylab, Y, zs = make_case("conv", 3, N=3, S=2, seed=4)
    res = []
    for sharded in (False, True):
        m = build_from_spec(spec, X, Y, likelihood=Gaussian(1.3))
        for _ in range(2):
            m.compute_gradients(X, Y, zs=zs, fetch=False)
            if sharded:
                m.debug_sharded_adam(ranks, 0.05)
            else:
                m.adam_step(0.05)
        res.append(_params(m))
        m.close()
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k
    assert res[0][(1, "likelihood_variance")] != 1.3


def test_sgd_and_natgrad_move_the_variance(ctx):
    spec, X, Ylab, Y, zs = make_case("conv", 3, N=3, S=2, seed=5)
    m = build_from_spec(spec, X, Y, likelihood=Gaussian(1.0))
    _, g = m.compute_gradients(X, Y, zs=zs)
    m.sgd_step(1e-3)
    m.pull_parameters()
    y = 1.0 - 1e-6
    u = np.log(np.expm1(y)) + 1e-3 * g[-1]["likelihood_variance"] * -np.expm1(-y)
    assert np.isclose(m.likelihood.variance, np.log1p(np.exp(u)) + 1e-6, rtol=1e-12)
    m.close()


def test_predictions(ctx):
    spec, X, Ylab, Y, zs = make_case("conv", 3, N=6, S=4, seed=9)
    s2 = 0.45
    model = build_from_spec(spec, X, Y, likelihood=Gaussian(s2))
    fm, fv = model.predict_f(X, 4, zs=zs)
    ym, yv = model.predict_y(X, 4, zs=zs)
    assert np.array_equal(ym, fm) and np.array_equal(yv, fv + s2)
    ld = model.predict_density(X, Y, 4, zs=zs)
    l = -0.5 * (LOG2PI + np.log(fv + s2)) - 0.5 * np.square(Y[None] - fm) / (fv + s2)
    mx = l.max(0)
    want = mx + np.log(np.exp(l - mx).sum(0)) - np.log(4)
    assert ld.shape == (6, 3) and rel(ld, want) < 1e-12
    model.close()


@pytest.mark.parametrize("batch", [1, 4, 7, 32])
def test_evaluate_equals_a_predict_density_loop(ctx, batch):
    spec, X, Ylab, Y, zs = make_case("conv", 3, N=11, S=3, seed=13)
    model = build_from_spec(spec, X, Y, likelihood=Gaussian(0.9))
    out = model.evaluate(X, Y, S=3, batch_size=batch, seed=21, per_image=True)
    loop, ym = [], []
    for i, lo in enumerate(range(0, 11, batch)):
        sl = slice(lo, lo + batch)
        loop.append(model.predict_density(X[sl], Y[sl], 3, seed=21 + i).sum(1))
        ym.append(model.predict_f(X[sl], 3, seed=21 + i)[0].mean(0))
    loop, ym = np.concatenate(loop), np.concatenate(ym)
    assert rel(out["log_density"], loop) < 1e-12
    assert rel(out["y_mean"], ym) < 1e-12
    assert abs(out["mean_log_density"] - loop.mean()) <= 1e-12 * abs(loop.mean())
    rmse = np.sqrt(np.mean(np.square(out["y_mean"] - Y)))
    assert abs(out["rmse"] - rmse) <= 1e-12 * rmse and out["n"] == 11
    assert TestLogDensityLogger(X, Y, batch_size=batch, num_samples=3)(model, seed=21) == out["mean_log_density"]
    model.close()


def test_error_paths(ctx):
    spec, X, Ylab, Y, zs = make_case("conv", 3, N=4, S=2, seed=2)
    with pytest.raises(ValueError):
        build_from_spec(spec, X, Y[:, :2], likelihood=Gaussian(1.0))
    model = build_from_spec(spec, X, Y, likelihood=Gaussian(1.0))
    with pytest.raises(ValueError):
        model.compute_log_likelihood(X, Y[:, :1], zs=zs)
    model._build()
    L = dev.lib()
    dX, dY = ctx.to_device(X), ctx.to_device(Ylab.astype(np.int32), np.int32)
    out, info = (C.c_double * 3)(), C.c_int(0)
    assert L.dcgp_elbo_forward(model._model, dX.ptr, dY.ptr, 4, 1.0, None, 0, 0, out, C.byref(info)) == dev.ERR_ARG
    assert L.dcgp_elbo_grad(model._model, dX.ptr, dY.ptr, 4, 1.0, None, 0, 0, out, C.byref(info)) == dev.ERR_ARG
    with pytest.raises(ValueError):
        AccuracyLogger(X, Y)(model)
    with pytest.raises(ValueError):
        model.predict_proba(X, 2)
    # the reverse: float targets into a RobustMax model
    rm = build_from_spec(spec, X, Ylab)
    rm._build()
    dYf = ctx.to_device(Y)
    assert L.dcgp_elbo_forward_f64y(rm._model, dX.ptr, dYf.ptr, 4, 1.0, None, 0, 0, out, C.byref(info)) == dev.ERR_ARG
    model.close(), rm.close()


def test_checkpoint_round_trip(ctx, tmp_path):
    spec, X, Ylab, Y, zs = make_case("conv", 3, N=4, S=2, seed=6)
    a = build_from_spec(spec, X, Y, likelihood=Gaussian(1.0))
    for _ in range(3):
        a.train_step(X, Y, 0.02, zs=zs)
    a.pull_parameters()
    e_a = a.compute_log_likelihood(X, Y, zs=zs)
    path = os.path.join(str(tmp_path), "ckpt.npy")
    save_model_parameters(a, path)
    params = np.load(path, allow_pickle=True).item()
    assert params["DGP/likelihood/likelihood/variance"] == a.likelihood.variance != 1.0
    b = build_from_spec(spec, X, Y, likelihood=Gaussian(1.0))
    for p in b.parameters:
        p.assign(params[p.pathname])
    b.sync_parameters()
    assert b.compute_log_likelihood(X, Y, zs=zs) == e_a
    a.close(), b.close()


def test_learns_standardised_digit_values(ctx):
    """Regression on real images: sklearn's 8 x 8 digits with the digit value standardised as the target, one ConvLayer + ConvKernel head
    built by ModelBuilder from the reference's flags (tools/digits_train.py's "conv" variant), the head cut to D = 1 and the likelihood
    swapped for Gaussian(1.0), trained by models.train (Adam)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from digits_train import VARIANTS, digits
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.dgp import DGP_Base
    from deepcgp_amd.models import ModelBuilder
    Xtr, Ytr, Xte, Yte = digits()
    mu, sd = Ytr.mean(), Ytr.std()
    ytr, yte = ((Ytr - mu) / sd)[:, None], ((Yte - mu) / sd)[:, None]
    flags = default_parser().parse_args(["--name", "digits", "--batch-size", "64", "--lr", "0.01", "--num-samples", "5"] + VARIANTS["conv"])
    np.random.seed(0)
    base = ModelBuilder(flags, Xtr, Ytr.reshape(-1, 1)).build()
    head = base.layers[-1]
    head.num_outputs, head.q_mu, head.q_sqrt = 1, np.zeros((head.num_inducing, 1)), head.q_sqrt[:1].copy()
    model = DGP_Base(base.X, ytr, Gaussian(1.0), base.layers, minibatch_size=base.minibatch_size, num_samples=base.num_samples,
                     num_data=base.num_data)
    Xte = Xte.reshape(len(Xte), -1)
    before = model.evaluate(Xte, yte, S=5)["rmse"]
    train(model, 1000, lr=0.01, lr_decay_steps=10 ** 9)
    out = model.evaluate(Xte, yte, S=5)
    print("digits regression: test RMSE %.4f (untrained %.4f), variance %.4f" % (out["rmse"], before, model.likelihood.variance))
    assert out["rmse"] < 0.5, out
    assert model.likelihood.variance < 1.0
    model.close()

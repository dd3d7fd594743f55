"""GPU: the Bernoulli (probit) likelihood end to end (csrc/pointwise.hip) -- ELBO, gradient, optimisers, predictions, evaluation, errors,
checkpoints and learning -- against the oracle's propagate with a NumPy quadrature tail (tests/bernoulli_ref.py) and torch autograd."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import bernoulli_ref as br
from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.likelihoods import Bernoulli, Gaussian, MultiClass
from deepcgp_amd.models import AccuracyLogger, TestLogDensityLogger, build_from_spec, save_model_parameters, train

pytestmark = pytest.mark.gpu


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
    X, Ylab = syn.make_batch(hwc, N, seed=seed)
    Y = (np.random.default_rng(seed).random((N, D)) < 0.5).astype(np.float64)
    zs = syn.make_noise(spec, N, seed=seed)
    return spec, X, Ylab, Y, zs


def grad_block(ctx, model, li):
    ptr, n = C.c_void_p(), C.c_size_t()
    ctx._check(dev.lib().dcgp_model_grad_block(model._model, li, C.byref(ptr), C.byref(n)))
    host = np.empty(n.value)
    ctx._check(dev.lib().dcgp_d2h(ctx.handle, host.ctypes.data, ptr, host.nbytes))
    return host


@pytest.mark.parametrize("case,D,white", [("conv", 1, False), ("conv", 3, True), ("head_only", 1, True), ("head_only", 3, False),
                                          ("dense_ard", 1, False), ("dense_ard", 3, True)])
@pytest.mark.parametrize("dedup", [False, True])
def test_elbo_vs_numpy(ctx, case, D, white, dedup):
    spec, X, Ylab, Y, zs = make_case(case, D, white)
    want, wdata, wkl = br.elbo(spec, X, Ylab, Y, zs)
    model = build_from_spec(spec, X, Y, likelihood=Bernoulli())
    model.dedup_layer0 = dedup
    e, data, kl = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    assert abs(e - want) <= 1e-10 * abs(want), (e, want)
    assert abs(data - wdata) <= 1e-10 * abs(wdata)
    assert abs(kl - wkl) <= 1e-10 * abs(wkl)
    # factor reuse mode 2: the next ELBO step reuses the parameter-only chain of this one, bit-identically
    model.set_factor_reuse(2)
    k0 = model.chain_skips
    assert model.compute_log_likelihood(X, Y, zs=zs, return_parts=True) == (e, data, kl)
    assert model.chain_skips == k0 + 1
    # the enqueue / collect halves: bit-identical to the synchronous call
    t = model.enqueue_log_likelihood(X, Y, zs=zs)
    assert model.collect_log_likelihood(t, return_parts=True) == (e, data, kl)
    model.close()


def _torch_bern_rule(m, v, Y):
    """The probit rule of tests/bernoulli_ref.py in torch, at the device's 20 Gauss-Hermite nodes: m, v [S, N, D] tensors, Y [N, D] in
    {0, 1} -> [S, N, D]; shared with tests/compose_ref.py."""
    import torch
    gx, gw = np.polynomial.hermite.hermgauss(20)
    gx, gw = torch.tensor(gx, dtype=torch.float64), torch.tensor(gw / math.sqrt(math.pi), dtype=torch.float64)
    F = m[..., None] + torch.sqrt(torch.clamp(2.0 * v, min=1e-10))[..., None] * gx
    p = torch.special.ndtr(F) * (1 - 2e-3) + 1e-3
    pos = torch.tensor(np.asarray(Y) == 1)[None, :, :, None]
    return (torch.where(pos, torch.log(p), torch.log(1 - p)) * gw).sum(-1)      # [S, N, D]


def _torch_bern(spec, X, Ylab, Y, zs):
    import torch
    import test_oracle_autograd as ta
    Ylab = np.asarray(Ylab) % Y.shape[1]          # (labels of the RobustMax forward the KL is recovered from)
    e_rm, leaves, m, v = ta._torch_elbo(spec, X, Ylab, zs, want_head=True)
    S, N = spec["S"], X.shape[0]
    y = torch.tensor(np.tile(np.asarray(Ylab).reshape(1, N), [S, 1]).reshape(S * N), dtype=torch.long)
    ve_rm = ta._robustmax_ve(m.reshape(S * N, -1), v.reshape(S * N, -1), y).reshape(S, N).mean(0).sum()
    kl = ve_rm * (spec["num_data"] / N) - e_rm
    ve = _torch_bern_rule(m, v, Y)
    return ve.sum(2).mean(0).sum() * (spec["num_data"] / N) - kl, leaves


@pytest.mark.parametrize("case", ["conv", "dense_ard"])
def test_gradient_vs_torch_autograd(ctx, case):
    torch = pytest.importorskip("torch")
    spec, X, Ylab, Y, zs = make_case(case, 3, N=3, S=2, seed=11)
    e_t, leaves = _torch_bern(spec, X, Ylab, Y, zs)
    flat = [(li, k, t) for li, p in enumerate(leaves) for k, t in p.items()]
    grads = torch.autograd.grad(e_t, [t for _, _, t in flat])
    model = build_from_spec(spec, X, Y, likelihood=Bernoulli())
    e, g = model.compute_gradients(X, Y, zs=zs)
    assert abs(e - e_t.item()) <= 1e-10 * abs(e_t.item())
    for (li, name, _), gt in zip(flat, grads):
        want, got = gt.numpy(), g[li][name]
        if name == "q_sqrt":
            want, got = np.tril(want), np.tril(got)
        assert np.abs(got - want).max() <= 1e-8 * max(1.0, np.abs(want).max()), (li, name)
    assert "likelihood_variance" not in g[-1]
    # two identical calls: bitwise identical gradient blocks, of the length the same spec has under MultiClass
    blocks = []
    for _ in range(2):
        model.compute_gradients(X, Y, zs=zs, fetch=False)
        blocks.append([grad_block(ctx, model, li) for li in range(len(model.layers))])
    rm = build_from_spec(spec, X, np.asarray(Ylab) % 3, likelihood=MultiClass(3))
    rm.compute_gradients(X, np.asarray(Ylab) % 3, zs=zs, fetch=False)
    for li in range(len(model.layers)):
        assert np.array_equal(blocks[0][li], blocks[1][li]), li
        assert blocks[0][li].size == grad_block(ctx, rm, li).size, li
    model.close(), rm.close()


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
    return out


POSITIVE = ("variance", "lengthscales")


def test_train_step_equals_numpy_adam(ctx):
    spec, X, Ylab, Y, zs = make_case("conv", 3, N=4, S=2, seed=3)
    lr, b1, b2, eps = 0.01, 0.9, 0.999, 1e-8
    a = build_from_spec(spec, X, Y, likelihood=Bernoulli())
    _, g = a.compute_gradients(X, Y, zs=zs)
    before = _params(a)
    b = build_from_spec(spec, X, Y, likelihood=Bernoulli())
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
    a.close(), b.close()


@pytest.mark.parametrize("ranks", [2, 3])
def test_sharded_adam_equals_the_full_step(ctx, ranks):
    spec, X, Ylab, Y, zs = make_case("conv", 3, N=3, S=2, seed=4)
    res = []
    for sharded in (False, True):
        m = build_from_spec(spec, X, Y, likelihood=Bernoulli())
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


@pytest.mark.parametrize("optimizer", ["SGD", "NatGrad", "Adam"])
def test_models_train_moves_the_parameters(ctx, optimizer):
    spec, X, Ylab, Y, zs = make_case("conv", 1, N=8, S=2, seed=5)
    m = build_from_spec(spec, X, Y, likelihood=Bernoulli())
    m.minibatch_size = 4
    before = _params(m)
    hist = train(m, 3, lr=0.01, optimizer=optimizer)
    after = _params(m)
    assert len(hist) == 3 and np.all(np.isfinite(hist))
    moved = [k for k in before if not np.array_equal(before[k], after[k])]
    assert (1, "q_mu") in moved and (0, "Z") in moved, moved
    assert all(np.all(np.isfinite(v)) for v in after.values())
    m.close()


def test_predictions(ctx):
    spec, X, Ylab, Y, zs = make_case("conv", 3, N=6, S=4, seed=9)
    model = build_from_spec(spec, X, Y, likelihood=Bernoulli())
    fm, fv = model.predict_f(X, 4, zs=zs)
    pm, pv = model.predict_y(X, 4, zs=zs)
    wm, wv = br.predict_mean_and_var(fm, fv)
    assert pm.shape == (4, 6, 3) and rel(pm, wm) < 1e-12 and rel(pv, wv) < 1e-12
    ld = model.predict_density(X, Y, 4, zs=zs)
    assert ld.shape == (6, 3) and rel(ld, br.predict_density(fm, fv, Y)) < 1e-12
    assert np.array_equal(model.predict_proba(X, 4, zs=zs), pm.mean(0))
    model.close()


@pytest.mark.parametrize("batch", [1, 4, 7, 32])
def test_evaluate_equals_a_predict_density_loop(ctx, batch):
    spec, X, Ylab, Y, zs = make_case("conv", 3, N=11, S=3, seed=13)
    model = build_from_spec(spec, X, Y, likelihood=Bernoulli())
    out = model.evaluate(X, Y, S=3, batch_size=batch, seed=21, per_image=True)
    loop, pm = [], []
    for i, lo in enumerate(range(0, 11, batch)):
        sl = slice(lo, lo + batch)
        loop.append(model.predict_density(X[sl], Y[sl], 3, seed=21 + i).sum(1))
        pm.append(model.predict_proba(X[sl], 3, seed=21 + i))
    loop, pm = np.concatenate(loop), np.concatenate(pm)
    assert rel(out["log_density"], loop) < 1e-12
    assert np.max(np.abs(out["p_mean"] - pm)) <= 1e-15
    assert abs(out["mean_log_density"] - loop.mean()) <= 1e-12 * abs(loop.mean())
    assert out["accuracy"] == np.mean((pm > 0.5) == (Y == 1)) and out["n"] == 11
    assert AccuracyLogger(X, Y, batch_size=batch, num_samples=3)(model, seed=21) == out["accuracy"]
    assert TestLogDensityLogger(X, Y, batch_size=batch, num_samples=3)(model, seed=21) == out["mean_log_density"]
    model.close()


def test_error_paths(ctx):
    spec, X, Ylab, Y, zs = make_case("conv", 3, N=4, S=2, seed=2)
    model = build_from_spec(spec, X, Y, likelihood=Bernoulli())
    with pytest.raises(ValueError):
        model.compute_log_likelihood(X, Y[:, :1], zs=zs)
    with pytest.raises(ValueError):
        model.compute_log_likelihood(X, Y * 2, zs=zs)
    model._build()
    L = dev.lib()
    dX, dY = ctx.to_device(X), ctx.to_device(Ylab.astype(np.int32) % 3, np.int32)
    out, info = (C.c_double * 3)(), C.c_int(0)
    # int32 entry points
    assert L.dcgp_elbo_forward(model._model, dX.ptr, dY.ptr, 4, 1.0, None, 0, 0, out, C.byref(info)) == dev.ERR_ARG
    assert L.dcgp_elbo_grad(model._model, dX.ptr, dY.ptr, 4, 1.0, None, 0, 0, out, C.byref(info)) == dev.ERR_ARG
    assert L.dcgp_model_train_step_adam(model._model, dX.ptr, dY.ptr, 4, 1.0, None, 0, 0, 0.01, 0.9, 0.999, 1e-8, 0, out,
                                        C.byref(info)) == dev.ERR_ARG
    p = ctx.empty((2 * 4, 3))
    assert L.dcgp_model_predict_y(model._model, dX.ptr, 4, 2, None, 0, p.ptr, None, C.byref(info)) == dev.ERR_ARG
    ld = ctx.empty((4,))
    assert L.dcgp_model_evaluate(model._model, dX.ptr, dY.ptr, 4, 4, 2, None, 0, ld.ptr, None, out, C.byref(info)) == dev.ERR_ARG
    # likelihood_variance is Gaussian-only
    one = np.array([0.5])
    assert L.dcgp_model_set_param(model._model, 0, b"likelihood_variance", one.ctypes.data, 1) == dev.ERR_ARG
    assert L.dcgp_model_get_param(model._model, 0, b"likelihood_variance", one.ctypes.data, 1) == dev.ERR_ARG
    assert L.dcgp_model_set_trainable(model._model, 0, b"likelihood_variance", 0) == dev.ERR_ARG
    with pytest.raises(dev.DcgpError):
        model.set_trainable(0, "likelihood_variance", False)
    # kinds beyond 2
    assert L.dcgp_model_set_likelihood(model._model, 3, 0.0) == dev.ERR_ARG
    assert L.dcgp_model_set_likelihood(model._model, -1, 0.0) == dev.ERR_ARG
    # the likelihood is fixed once a gradient was taken
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    assert L.dcgp_model_get_grad(model._model, 0, b"likelihood_variance", one.ctypes.data, 1) == dev.ERR_ARG
    assert L.dcgp_model_set_likelihood(model._model, 0, 0.0) == dev.ERR_ARG
    assert L.dcgp_model_set_likelihood(model._model, 1, 1.0) == dev.ERR_ARG
    assert L.dcgp_model_set_likelihood(model._model, 2, 0.0) == dev.DCGP_OK
    assert np.isfinite(model.compute_log_likelihood(X, Y, zs=zs))
    # float targets into a RobustMax model are still refused; a Gaussian model still works beside a Bernoulli one
    rm = build_from_spec(spec, X, Ylab % 3, likelihood=MultiClass(3))
    rm._build()
    dYf = ctx.to_device(Y)
    assert L.dcgp_elbo_forward_f64y(rm._model, dX.ptr, dYf.ptr, 4, 1.0, None, 0, 0, out, C.byref(info)) == dev.ERR_ARG
    ga = build_from_spec(spec, X, Y, likelihood=Gaussian(0.5))
    assert np.isfinite(ga.compute_log_likelihood(X, Y, zs=zs))
    model.close(), rm.close(), ga.close()


def test_checkpoint_round_trip(ctx, tmp_path):
    spec, X, Ylab, Y, zs = make_case("conv", 3, N=4, S=2, seed=6)
    a = build_from_spec(spec, X, Y, likelihood=Bernoulli())
    for _ in range(3):
        a.train_step(X, Y, 0.02, zs=zs)
    a.pull_parameters()
    e_a = a.compute_log_likelihood(X, Y, zs=zs)
    path = os.path.join(str(tmp_path), "ckpt.npy")
    save_model_parameters(a, path)
    params = np.load(path, allow_pickle=True).item()
    assert not any("likelihood" in k for k in params)
    b = build_from_spec(spec, X, Y, likelihood=Bernoulli())
    for p in b.parameters:
        p.assign(params[p.pathname])
    b.sync_parameters()
    assert b.compute_log_likelihood(X, Y, zs=zs) == e_a
    a.close(), b.close()


def test_learns_even_versus_odd_digits(ctx):
    """Binary classification on real images: sklearn's 8 x 8 digits, label 1 for an even digit, one ConvLayer + ConvKernel head built by
    ModelBuilder from the reference's flags (tools/digits_train.py's "conv" variant), the head cut to D = 1 and the likelihood swapped for
    Bernoulli(), trained by models.train (Adam, 1000 steps)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from digits_train import VARIANTS, digits
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.dgp import DGP_Base
    from deepcgp_amd.models import ModelBuilder
    Xtr, Ytr, Xte, Yte = digits()
    ytr, yte = (Ytr % 2 == 0)[:, None], (Yte % 2 == 0)[:, None]
    flags = default_parser().parse_args(["--name", "digits", "--batch-size", "64", "--lr", "0.01", "--num-samples", "5"] + VARIANTS["conv"])
    np.random.seed(0)
    base = ModelBuilder(flags, Xtr, Ytr.reshape(-1, 1)).build()
    head = base.layers[-1]
    head.num_outputs, head.q_mu, head.q_sqrt = 1, np.zeros((head.num_inducing, 1)), head.q_sqrt[:1].copy()
    model = DGP_Base(base.X, ytr, Bernoulli(), base.layers, minibatch_size=base.minibatch_size, num_samples=base.num_samples,
                     num_data=base.num_data)
    Xte = Xte.reshape(len(Xte), -1)
    before = model.evaluate(Xte, yte, S=5)
    train(model, 1000, lr=0.01, lr_decay_steps=10 ** 9)
    out = model.evaluate(Xte, yte, S=5)
    print("digits even/odd: test accuracy %.4f (untrained %.4f), mean log density %.4f (untrained %.4f)"
          % (out["accuracy"], before["accuracy"], out["mean_log_density"], before["mean_log_density"]))
    assert out["accuracy"] >= 0.93, out
    assert out["mean_log_density"] > before["mean_log_density"]
    assert AccuracyLogger(Xte, yte)(model) == out["accuracy"]
    model.close()

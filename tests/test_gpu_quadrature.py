"""GPU: the StudentT and Poisson likelihoods end to end (csrc/pointwise.hip) -- ELBO, gradient, the operator entries on a hand-made
array with the clamp branch, optimisers, predictions, evaluation, errors, checkpoints and learning -- against the oracle's propagate with
a NumPy / SciPy quadrature tail (tests/quad_ref.py) and torch autograd of the same forward written with torch.distributions."""
import ctypes as C
import os

import numpy as np
import pytest

import quad_ref as qr
from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.likelihoods import Bernoulli, Gaussian, MultiClass, Poisson, StudentT
from deepcgp_amd.models import AccuracyLogger, TestLogDensityLogger, build_from_spec, save_model_parameters, train

pytestmark = pytest.mark.gpu

LIKS = [("studentt", 0.7, 3.0), ("studentt", 0.7, 4.5), ("poisson", 1.0), ("poisson", 2.5)]
ONE_EACH = [("studentt", 0.7, 4.5), ("poisson", 2.5)]


def make_lik(tup):
    return StudentT(tup[1], tup[2]) if tup[0] == "studentt" else Poisson(binsize=tup[1])


def lik_id(tup):
    return "-".join(str(t) for t in tup)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def make_case(tup, case, D, white=False, N=5, S=3, seed=7):
    """tests/test_gpu_gaussian.py::make_case's shapes; StudentT targets standard normal with one outlier at 8.0, Poisson targets
    poisson(2.5) with at least one 0."""
    hwc = (10, 10, 1)
    kw = dict(S=S, num_data=300, seed=seed, white=white, conv_q_sqrt_scale=0.3, variance=2.0, ls=1.5, head_outputs=D)
    if case == "conv":
        spec = syn.make_spec(hwc, [(3, 1, 2)], (3, 1), 9, **kw)
    elif case == "head_only":
        spec = syn.make_spec(hwc, [], (3, 1), 9, **kw)
    elif case == "dense_ard":
        spec = syn.make_spec(hwc, [(3, 1, 2)], (3, 1), 9, head_kernel="rbf", **kw)
    X, Ylab = syn.make_batch(hwc, N, seed=seed)
    rng = np.random.default_rng(seed)
    if tup[0] == "studentt":
        Y = rng.standard_normal((N, D))
        Y[N // 2, D // 2] = 8.0
    else:
        Y = rng.poisson(2.5, (N, D)).astype(np.float64)
        Y[0, 0] = 0.0
    zs = syn.make_noise(spec, N, seed=seed)
    return spec, X, Ylab, Y, zs


def grad_block(ctx, model, li):
    ptr, n = C.c_void_p(), C.c_size_t()
    ctx._check(dev.lib().dcgp_model_grad_block(model._model, li, C.byref(ptr), C.byref(n)))
    host = np.empty(n.value)
    ctx._check(dev.lib().dcgp_d2h(ctx.handle, host.ctypes.data, ptr, host.nbytes))
    return host


# ---- 1. ELBO ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tup", LIKS, ids=lik_id)
@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("D", [1, 3, 10])
@pytest.mark.parametrize("case", ["conv", "head_only", "dense_ard"])
def test_elbo_vs_numpy(ctx, case, D, white, tup):
    spec, X, Ylab, Y, zs = make_case(tup, case, D, white)
    want, wdata, wkl = qr.elbo(tup, spec, X, Ylab, Y, zs, key=(case, D, white))     # (the oracle's marginals: once per spec)
    model = build_from_spec(spec, X, Y, likelihood=make_lik(tup))
    for dedup in (False, True):
        model.dedup_layer0 = dedup
        e, data, kl = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
        assert abs(e - want) <= 1e-10 * abs(want), (dedup, e, want)
        assert abs(data - wdata) <= 1e-10 * abs(wdata), (dedup, data, wdata)
        assert abs(kl - wkl) <= 1e-10 * abs(wkl), (dedup, kl, wkl)
        # the enqueue / collect halves: bit-identical to the synchronous call
        t = model.enqueue_log_likelihood(X, Y, zs=zs)
        assert model.collect_log_likelihood(t, return_parts=True) == (e, data, kl)
    model.close()


# ---- 2. gradients -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tup", LIKS, ids=lik_id)
@pytest.mark.parametrize("case", ["conv", "dense_ard"])
def test_gradient_vs_torch_autograd(ctx, case, tup):
    torch = pytest.importorskip("torch")
    spec, X, Ylab, Y, zs = make_case(tup, case, 3, N=3, S=2, seed=11)
    e_t, leaves, scale = qr.torch_elbo(tup, spec, X, Ylab, Y, zs)
    flat = [(li, k, t) for li, p in enumerate(leaves) for k, t in p.items()]
    grads = torch.autograd.grad(e_t, [t for _, _, t in flat] + ([scale] if scale is not None else []))
    model = build_from_spec(spec, X, Y, likelihood=make_lik(tup))
    e, g = model.compute_gradients(X, Y, zs=zs)
    assert abs(e - e_t.item()) <= 1e-10 * abs(e_t.item())
    for (li, name, _), gt in zip(flat, grads):
        want, got = gt.numpy(), g[li][name]
        if name == "q_sqrt":
            want, got = np.tril(want), np.tril(got)
        assert np.abs(got - want).max() <= 1e-8 * max(1.0, np.abs(want).max()), (li, name)
    assert "likelihood_variance" not in g[-1]
    # two identical calls: bitwise identical gradient blocks
    blocks = []
    for _ in range(2):
        model.compute_gradients(X, Y, zs=zs, fetch=False)
        blocks.append([grad_block(ctx, model, li) for li in range(len(model.layers))])
    for li in range(len(model.layers)):
        assert np.array_equal(blocks[0][li], blocks[1][li]), li
    rm = build_from_spec(spec, X, np.asarray(Ylab) % 3, likelihood=MultiClass(3))
    rm.compute_gradients(X, np.asarray(Ylab) % 3, zs=zs, fetch=False)
    sizes = [grad_block(ctx, rm, li).size for li in range(len(model.layers))]
    if tup[0] == "studentt":      # the scale's gradient: the last slot of the head's block, one longer than a RobustMax block
        want = grads[-1].item()
        assert abs(g[-1]["likelihood_scale"] - want) <= 1e-8 * max(1.0, abs(want)), (g[-1]["likelihood_scale"], want)
        assert blocks[0][-1][-1] == g[-1]["likelihood_scale"]
        sizes[-1] += 1
    else:                         # Poisson: no parameter, the RobustMax layout
        assert "likelihood_scale" not in g[-1]
    assert [b.size for b in blocks[0]] == sizes
    model.close(), rm.close()


def test_input_gradient_elbo_objective(ctx):
    """input_gradient(objective="elbo") through lik_grad_seeds: J is the image's share of the data term, the gradient finite and non-zero."""
    for tup in ONE_EACH:
        spec, X, Ylab, Y, zs = make_case(tup, "conv", 3, N=4, S=2, seed=8)
        model = build_from_spec(spec, X, Y, likelihood=make_lik(tup))
        J, g = model.input_gradient(X, Y, objective="elbo", zs=zs)
        _, data, _ = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
        assert abs(J.sum() - data) <= 1e-10 * abs(data)
        assert g.shape == (4, 100) and np.all(np.isfinite(g)) and np.abs(g).max() > 0
        model.close()


# ---- 3. operator entries on a hand-made [7][3] array ---------------------------------------------------------------------------------
def hand_array(tup):
    """mu, var, y [7][3]: v = 0 and v = 1e-12 (the clamp branch), the model-level range of v, m = +-4; StudentT: |y - m| / scale = 50;
    Poisson: counts 0 and 60."""
    mu = np.array([[0.3, -0.2, 0.1], [4.0, -4.0, 0.0], [-0.5, 0.4, 0.25], [4.0, -4.0, 1.5], [0.0, -1.0, 2.0], [0.7, -0.7, 0.05],
                   [-4.0, 4.0, -0.3]])
    var = np.array([[0.0, 1e-12, 0.055], [0.91, 2.0, 0.4], [1e-12, 0.0, 0.3], [0.0, 0.5, 1e-12], [2.0, 0.055, 0.91], [0.4, 0.7, 0.0],
                    [0.2, 0.3, 1.0]])
    if tup[0] == "studentt":
        y = mu + np.array([[0.5, -1.0, 50 * tup[1]], [-50 * tup[1], 0.3, 0.0], [2.0, -2.0, 8.0], [50 * tup[1], 1.0, -0.1],
                           [0.2, -50 * tup[1], 3.0], [-0.4, 0.9, 1.1], [6.0, -6.0, 0.0]])
    else:
        y = np.array([[0, 1, 2], [60, 0, 3], [0, 60, 1], [0, 60, 5], [7, 0, 60], [2, 4, 0], [60, 0, 60]], np.float64)
    return mu, var, y


@pytest.mark.parametrize("tup", LIKS, ids=lik_id)
def test_operator_entries(ctx, tup):
    torch = pytest.importorskip("torch")
    L = dev.lib()
    mu, var, y = hand_array(tup)
    par = np.array(tup[1:], np.float64)
    kind = 4 if tup[0] == "studentt" else 5
    dmu, dvar, dy = ctx.to_device(mu), ctx.to_device(var), ctx.to_device(y)
    ve, ld, em, ev = (ctx.empty((7, 3)) for _ in range(4))
    ctx._check(L.dcgp_quad_varexp(ctx.handle, kind, par.ctypes.data, dmu.ptr, dvar.ptr, dy.ptr, 7, 3, ve.ptr))
    ctx._check(L.dcgp_quad_logdensity(ctx.handle, kind, par.ctypes.data, dmu.ptr, dvar.ptr, dy.ptr, 7, 3, ld.ptr))
    ctx._check(L.dcgp_quad_predict(ctx.handle, kind, par.ctypes.data, dmu.ptr, dvar.ptr, 7, 3, em.ptr, ev.ptr))
    we, wv = qr.predict_mean_and_var(tup, mu, var)
    assert rel(ve.numpy(), qr.variational_expectations(tup, mu, var, y)) <= 1e-12
    assert rel(ld.numpy(), qr.log_density(tup, mu, var, y)) <= 1e-12
    assert rel(em.numpy(), we) <= 1e-12 and rel(ev.numpy(), wv) <= 1e-12
    # either output may be NULL
    em2 = ctx.empty((7, 3))
    ctx._check(L.dcgp_quad_predict(ctx.handle, kind, par.ctypes.data, dmu.ptr, dvar.ptr, 7, 3, em2.ptr, None))
    assert np.array_equal(em2.numpy(), em.numpy())
    # the host class goes through the same entry
    assert np.array_equal(make_lik(tup).variational_expectations(mu, var, y), ve.numpy())
    # the reverse tail on the same array (the clamp branch included) against autograd of the torch forward
    tm, tv = torch.tensor(mu, requires_grad=True), torch.tensor(var, requires_grad=True)
    ts = torch.tensor(tup[1], dtype=torch.float64, requires_grad=True) if kind == 4 else None
    tot = 0.37 * qr.torch_ve(tup, tm, tv, torch.tensor(y), ts).sum()
    want = torch.autograd.grad(tot, [tm, tv] + ([ts] if kind == 4 else []))
    gm, gv, gp = ctx.empty((7, 3)), ctx.empty((7, 3)), ctx.empty((1,))
    ctx._check(L.dcgp_quad_grad_seeds(ctx.handle, kind, par.ctypes.data, dmu.ptr, dvar.ptr, dy.ptr, 7, 3, 0.37, gm.ptr, gv.ptr,
                                      gp.ptr if kind == 4 else None))
    assert rel(gm.numpy(), want[0].numpy()) <= 1e-12
    assert rel(gv.numpy(), want[1].numpy()) <= 1e-12
    if kind == 4:
        clamped = 2 * var <= 1e-10
        assert clamped.sum() == 7 and np.all(gv.numpy()[clamped] == 0.0) and np.all(gv.numpy()[~clamped] != 0.0)
        assert abs(gp.numpy()[0] - want[2].item()) <= 1e-12 * abs(want[2].item())
    # bad arguments
    out = ctx.empty((7, 3))
    for bad_kind, bad_par in ((3, par), (6, par), (kind, np.array([-1.0, 3.0])), (kind, np.array([float("nan"), 3.0]))):
        assert L.dcgp_quad_varexp(ctx.handle, bad_kind, bad_par.ctypes.data, dmu.ptr, dvar.ptr, dy.ptr, 7, 3, out.ptr) == dev.ERR_ARG
    assert L.dcgp_quad_varexp(ctx.handle, 4, np.array([1.0, 2.0]).ctypes.data, dmu.ptr, dvar.ptr, dy.ptr, 7, 3, out.ptr) == dev.ERR_ARG
    assert L.dcgp_quad_logdensity(ctx.handle, kind, None, dmu.ptr, dvar.ptr, dy.ptr, 7, 3, out.ptr) == dev.ERR_ARG
    assert L.dcgp_quad_predict(ctx.handle, kind, par.ctypes.data, dmu.ptr, dvar.ptr, 7, 3, None, None) == dev.ERR_ARG


# ---- 4. optimisers ------------------------------------------------------------------------------------------------------------------
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
    if model.student_t:
        out[(len(model.layers) - 1, "likelihood_scale")] = np.array(model.likelihood.scale)
    return out


POSITIVE = ("variance", "lengthscales", "likelihood_scale")


@pytest.mark.parametrize("tup", ONE_EACH, ids=lik_id)
def test_train_step_equals_numpy_adam(ctx, tup):
    spec, X, Ylab, Y, zs = make_case(tup, "conv", 3, N=4, S=2, seed=3)
    lr, b1, b2, eps = 0.01, 0.9, 0.999, 1e-8
    a = build_from_spec(spec, X, Y, likelihood=make_lik(tup))
    _, g = a.compute_gradients(X, Y, zs=zs)
    before = _params(a)
    b = build_from_spec(spec, X, Y, likelihood=make_lik(tup))
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
    if tup[0] == "studentt":
        key = (len(b.layers) - 1, "likelihood_scale")
        assert key in before and after[key] > 0 and after[key] != tup[1]
        # switched off, the scale stays where it is under Adam (the rest still moves)
        b.set_trainable(0, "likelihood_scale", False)
        s = b.likelihood.scale
        b.train_step(X, Y, lr, zs=zs)
        after2 = _params(b)
        assert after2[key] == s
        assert not np.array_equal(after2[(0, "Z")], after[(0, "Z")])
    a.close(), b.close()


@pytest.mark.parametrize("tup", ONE_EACH, ids=lik_id)
@pytest.mark.parametrize("ranks", [2, 3])
def test_sharded_adam_equals_the_full_step(ctx, ranks, tup):
    spec, X, Ylab, Y, zs = make_case(tup, "conv", 3, N=3, S=2, seed=4)
    res = []
    for sharded in (False, True):
        m = build_from_spec(spec, X, Y, likelihood=make_lik(tup))
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
    if tup[0] == "studentt":
        assert res[0][(1, "likelihood_scale")] != tup[1]


@pytest.mark.parametrize("tup", ONE_EACH, ids=lik_id)
@pytest.mark.parametrize("optimizer", ["SGD", "NatGrad"])
def test_sgd_and_natgrad_move_the_parameters(ctx, optimizer, tup):
    spec, X, Ylab, Y, zs = make_case(tup, "conv", 1, N=8, S=2, seed=5)
    m = build_from_spec(spec, X, Y, likelihood=make_lik(tup))
    m.minibatch_size = 4
    before = _params(m)
    hist = train(m, 3, lr=0.01, optimizer=optimizer)
    after = _params(m)
    assert len(hist) == 3 and np.all(np.isfinite(hist))
    moved = [k for k in before if not np.array_equal(before[k], after[k])]
    assert (1, "q_mu") in moved and (0, "Z") in moved, moved
    if tup[0] == "studentt":
        assert (1, "likelihood_scale") in moved
    assert all(np.all(np.isfinite(v)) for v in after.values())
    m.close()


def test_sgd_step_on_the_scale_in_unconstrained_space(ctx):
    tup = ONE_EACH[0]
    spec, X, Ylab, Y, zs = make_case(tup, "conv", 3, N=3, S=2, seed=5)
    m = build_from_spec(spec, X, Y, likelihood=make_lik(tup))
    _, g = m.compute_gradients(X, Y, zs=zs)
    m.sgd_step(1e-3)
    m.pull_parameters()
    y = tup[1] - 1e-6
    u = np.log(np.expm1(y)) + 1e-3 * g[-1]["likelihood_scale"] * -np.expm1(-y)
    assert np.isclose(m.likelihood.scale, np.log1p(np.exp(u)) + 1e-6, rtol=1e-12)
    m.close()


# ---- 5. predictions and evaluation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tup", LIKS, ids=lik_id)
def test_predictions(ctx, tup):
    spec, X, Ylab, Y, zs = make_case(tup, "conv", 3, N=6, S=4, seed=9)
    model = build_from_spec(spec, X, Y, likelihood=make_lik(tup))
    fm, fv = model.predict_f(X, 4, zs=zs)
    pm, pv = model.predict_y(X, 4, zs=zs)
    wm, wv = qr.predict_mean_and_var(tup, fm, fv)
    assert pm.shape == (4, 6, 3) and pv.shape == (4, 6, 3) and rel(pm, wm) < 1e-12 and rel(pv, wv) < 1e-12
    if tup[0] == "studentt":      # the closed forms, written as such on the device
        assert np.array_equal(pm, fm) and rel(pv, fv + tup[1] ** 2 * tup[2] / (tup[2] - 2)) < 1e-15
    ld = model.predict_density(X, Y, 4, zs=zs)
    assert ld.shape == (6, 3) and rel(ld, qr.predict_density(tup, fm, fv, Y)) < 1e-12
    model.close()


@pytest.mark.parametrize("tup", ONE_EACH, ids=lik_id)
@pytest.mark.parametrize("batch", [1, 4, 7, 32])
def test_evaluate_equals_a_predict_density_loop(ctx, batch, tup):
    spec, X, Ylab, Y, zs = make_case(tup, "conv", 3, N=13, S=3, seed=13)
    model = build_from_spec(spec, X, Y, likelihood=make_lik(tup))
    out = model.evaluate(X, Y, S=3, batch_size=batch, seed=21, per_image=True)
    loop, ym = [], []
    for i, lo in enumerate(range(0, 13, batch)):
        sl = slice(lo, lo + batch)
        loop.append(model.predict_density(X[sl], Y[sl], 3, seed=21 + i).sum(1))
        ym.append(model.predict_y(X[sl], 3, seed=21 + i)[0].mean(0))
    loop, ym = np.concatenate(loop), np.concatenate(ym)
    assert set(out) == {"mean_log_density", "rmse", "n", "log_density", "y_mean"}
    assert rel(out["log_density"], loop) < 1e-12
    assert rel(out["y_mean"], ym) < 1e-12
    assert abs(out["mean_log_density"] - loop.mean()) <= 1e-12 * abs(loop.mean())
    rmse = np.sqrt(np.mean(np.square(out["y_mean"] - Y)))
    assert abs(out["rmse"] - rmse) <= 1e-12 * rmse and out["n"] == 13
    assert TestLogDensityLogger(X, Y, batch_size=batch, num_samples=3)(model, seed=21) == out["mean_log_density"]
    model.close()


# ---- 6. error paths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tup", ONE_EACH, ids=lik_id)
def test_error_paths(ctx, tup):
    spec, X, Ylab, Y, zs = make_case(tup, "conv", 3, N=4, S=2, seed=2)
    kind = 4 if tup[0] == "studentt" else 5
    name = "StudentT" if kind == 4 else "Poisson"
    par = np.array(tup[1:], np.float64)
    model = build_from_spec(spec, X, Y, likelihood=make_lik(tup))
    with pytest.raises(ValueError):
        model.compute_log_likelihood(X, Y[:, :1], zs=zs)
    if kind == 5:
        with pytest.raises(ValueError, match="Poisson likelihood"):
            model.compute_log_likelihood(X, Y + 0.5, zs=zs)
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
    # what needs class probabilities, and the density objective, name the likelihood
    for call in (lambda: model.predict_proba(X, 2), lambda: model.evaluate_uncertainty(X, Y), lambda: AccuracyLogger(X, Y)(model)):
        with pytest.raises(ValueError, match=name):
            call()
    with pytest.raises(NotImplementedError, match=name):
        model.input_gradient(X, Y, objective="density")
    dYf = ctx.to_device(Y)
    J, gx = ctx.empty((4,)), ctx.empty((4, 100))
    assert L.dcgp_model_input_grad_f64y(model._model, dX.ptr, dYf.ptr, 4, 2, None, 0, dev.OBJECTIVE_DENSITY, J.ptr, gx.ptr, C.byref(info)) == dev.ERR_ARG
    # likelihood_variance stays Gaussian-only; likelihood_scale is StudentT-only
    one = np.array([0.5])
    assert L.dcgp_model_set_param(model._model, 0, b"likelihood_variance", one.ctypes.data, 1) == dev.ERR_ARG
    assert L.dcgp_model_get_param(model._model, 0, b"likelihood_variance", one.ctypes.data, 1) == dev.ERR_ARG
    assert L.dcgp_model_set_trainable(model._model, 0, b"likelihood_variance", 0) == dev.ERR_ARG
    others = [build_from_spec(spec, X, np.clip(np.rint(np.abs(Y)), 0, 1), likelihood=Bernoulli()), build_from_spec(spec, X, Y, likelihood=Gaussian(0.5))]
    pc = make_case(LIKS[2], "conv", 3, N=4, S=2, seed=2)
    others.append(build_from_spec(pc[0], pc[1], pc[3], likelihood=Poisson()))
    for o in others:
        o._build()
        assert L.dcgp_model_set_param(o._model, 0, b"likelihood_scale", one.ctypes.data, 1) == dev.ERR_ARG
        assert L.dcgp_model_get_param(o._model, 0, b"likelihood_scale", one.ctypes.data, 1) == dev.ERR_ARG
        assert L.dcgp_model_get_grad(o._model, 0, b"likelihood_scale", one.ctypes.data, 1) == dev.ERR_ARG
        assert L.dcgp_model_set_trainable(o._model, 0, b"likelihood_scale", 0) == dev.ERR_ARG
        with pytest.raises(dev.DcgpError):
            o.set_trainable(0, "likelihood_scale", False)
    if kind == 4:
        tiny = np.array([1e-6])
        assert L.dcgp_model_set_param(model._model, 0, b"likelihood_scale", tiny.ctypes.data, 1) == dev.ERR_ARG
        assert L.dcgp_model_set_param(model._model, 0, b"likelihood_scale", one.ctypes.data, 2) == dev.ERR_ARG
        assert L.dcgp_model_get_param(model._model, 0, b"likelihood_scale", one.ctypes.data, 1) == dev.DCGP_OK and one[0] == tup[1]
    # bad parameters, a wrong count, other kinds
    sp = L.dcgp_model_set_likelihood_params
    bads = [np.array([0.0, 3.0]), np.array([1.0, 2.0]), np.array([float("nan"), 3.0]), np.array([1.0, float("inf")])] if kind == 4 else \
           [np.array([0.0]), np.array([-1.0]), np.array([float("inf")])]
    for bad in bads:
        assert sp(model._model, kind, bad.ctypes.data, bad.size) == dev.ERR_ARG
    assert sp(model._model, kind, par.ctypes.data, par.size + 1) == dev.ERR_ARG
    assert sp(model._model, kind, None, par.size) == dev.ERR_ARG
    for other in (0, 1, 2, 3, 6, -1):
        assert sp(model._model, other, par.ctypes.data, par.size) == dev.ERR_ARG
    # dcgp_model_set_likelihood itself takes kinds 0 to 3 only, as before
    assert L.dcgp_model_set_likelihood(model._model, 4, 1.0) == dev.ERR_ARG
    assert L.dcgp_model_set_likelihood(model._model, 5, 1.0) == dev.ERR_ARG
    assert L.dcgp_model_set_likelihood(model._model, 3, 0.0) == dev.ERR_ARG       # (Softmax on a float64-target model)
    # the kind is fixed once a gradient was taken; the same kind may still be set
    e0 = model.compute_log_likelihood(X, Y, zs=zs)
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    okind, opar = (5, np.array([1.0])) if kind == 4 else (4, np.array([1.0, 3.0]))
    assert sp(model._model, okind, opar.ctypes.data, opar.size) == dev.ERR_ARG
    assert L.dcgp_model_set_likelihood(model._model, 1, 1.0) == dev.ERR_ARG
    assert sp(model._model, kind, par.ctypes.data, par.size) == dev.DCGP_OK
    assert model.compute_log_likelihood(X, Y, zs=zs) == e0
    # float targets into a RobustMax model are refused, and so is a switch of a label model that has taken steps
    rm = build_from_spec(spec, X, Ylab % 3, likelihood=MultiClass(3))
    rm._build()
    assert L.dcgp_elbo_forward_f64y(rm._model, dX.ptr, dYf.ptr, 4, 1.0, None, 0, 0, out, C.byref(info)) == dev.ERR_ARG
    assert np.isfinite(rm.compute_log_likelihood(X, Ylab % 3, zs=zs))
    assert sp(rm._model, kind, par.ctypes.data, par.size) == dev.ERR_ARG
    assert np.isfinite(rm.compute_log_likelihood(X, Ylab % 3, zs=zs))
    model.close(), rm.close()
    for o in others:
        o.close()


# ---- 7. checkpoints -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tup", ONE_EACH, ids=lik_id)
def test_checkpoint_round_trip(ctx, tmp_path, tup):
    spec, X, Ylab, Y, zs = make_case(tup, "conv", 3, N=4, S=2, seed=6)
    a = build_from_spec(spec, X, Y, likelihood=make_lik(tup))
    for _ in range(3):
        a.train_step(X, Y, 0.02, zs=zs)
    a.pull_parameters()
    e_a = a.compute_log_likelihood(X, Y, zs=zs)
    path = os.path.join(str(tmp_path), "ckpt.npy")
    save_model_parameters(a, path)
    params = np.load(path, allow_pickle=True).item()
    if tup[0] == "studentt":
        assert params["DGP/likelihood/likelihood/scale"] == a.likelihood.scale != tup[1]
    else:
        assert not any("likelihood" in k for k in params)
    b = build_from_spec(spec, X, Y, likelihood=make_lik(tup))
    for p in b.parameters:
        p.assign(params[p.pathname])
    b.sync_parameters()
    assert b.compute_log_likelihood(X, Y, zs=zs) == e_a
    a.close(), b.close()


# ---- 8. learning --------------------------------------------------------------------------------------------------------------------
def _digits_model(lik, ytr):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from digits_train import VARIANTS, digits
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.dgp import DGP_Base
    from deepcgp_amd.models import ModelBuilder
    Xtr, Ytr, Xte, Yte = digits()
    flags = default_parser().parse_args(["--name", "digits", "--batch-size", "64", "--lr", "0.01", "--num-samples", "5"] + VARIANTS["head"])
    np.random.seed(0)
    base = ModelBuilder(flags, Xtr, Ytr.reshape(-1, 1)).build()
    head = base.layers[-1]
    head.num_outputs, head.q_mu, head.q_sqrt = 1, np.zeros((head.num_inducing, 1)), head.q_sqrt[:1].copy()
    return DGP_Base(base.X, ytr, lik, base.layers, minibatch_size=base.minibatch_size, num_samples=base.num_samples, num_data=base.num_data)


STEPS = 300     # (sklearn's 8 x 8 digits, the SVGP head with the ConvKernel at M = 32, batches of 64: a few hundred short steps)


def test_student_t_beats_gaussian_on_corrupted_targets(ctx):
    """Regression on the standardised digit value with 10 % of the training targets replaced by +-20: the StudentT model's test RMSE
    against the clean targets is below that of a Gaussian model trained with the same seeds and steps."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from digits_train import digits
    Xtr, Ytr, Xte, Yte = digits()
    mu, sd = Ytr.mean(), Ytr.std()
    ytr, yte = ((Ytr - mu) / sd)[:, None], ((Yte - mu) / sd)[:, None]
    rng = np.random.default_rng(0)
    bad = rng.choice(len(ytr), len(ytr) // 10, replace=False)
    ytr = ytr.copy()
    ytr[bad, 0] = rng.choice([-20.0, 20.0], len(bad))
    Xte = Xte.reshape(len(Xte), -1)
    rmse = {}
    for name, lik in (("StudentT", StudentT(1.0, 3.0)), ("Gaussian", Gaussian(1.0))):
        model = _digits_model(lik, ytr)
        train(model, STEPS, lr=0.01, lr_decay_steps=10 ** 9)
        rmse[name] = model.evaluate(Xte, yte, S=5)["rmse"]
        model.close()
    print("digits with 10 %% outliers: test RMSE on clean targets StudentT %.4f, Gaussian %.4f" % (rmse["StudentT"], rmse["Gaussian"]))
    assert rmse["StudentT"] < rmse["Gaussian"], rmse


def test_poisson_learns_digit_values_as_counts(ctx):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from digits_train import digits
    Xtr, Ytr, Xte, Yte = digits()
    model = _digits_model(Poisson(), Ytr[:, None].astype(np.float64))
    Xte, yte = Xte.reshape(len(Xte), -1), Yte[:, None].astype(np.float64)
    before = model.evaluate(Xte, yte, S=5)
    train(model, STEPS, lr=0.01, lr_decay_steps=10 ** 9)
    out = model.evaluate(Xte, yte, S=5)
    print("digits as counts: mean test log density %.4f (untrained %.4f), RMSE %.4f (untrained %.4f)"
          % (out["mean_log_density"], before["mean_log_density"], out["rmse"], before["rmse"]))
    assert out["mean_log_density"] > before["mean_log_density"]
    model.close()

"""GPU: the Softmax likelihood end to end (csrc/softmax.hip) -- stand-alone tails, ELBO, gradient, optimisers, predictions, evaluation,
uncertainty, input gradients, errors and learning -- against the oracle's propagate with a NumPy tail (tests/softmax_ref.py) and torch
autograd of independently written forwards (tests/test_oracle_autograd.py for the parameters, tests/input_grad_ref.py for the pixels)."""
import ctypes as C
import os

import numpy as np
import pytest

import live_specs as ls
import softmax_ref as sr
from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.likelihoods import MultiClass, Softmax
from deepcgp_amd.models import (AccuracyLogger, TestLogDensityLogger, UncertaintyLogger, adversarial_examples, build_from_spec, train)

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def make_case(case, K, white=False, N=5, S=3, seed=7):
    hwc = (10, 10, 1)
    kw = dict(S=S, num_data=300, seed=seed, white=white, conv_q_sqrt_scale=0.3, variance=2.0, ls=1.5, head_outputs=K)
    if case == "conv":
        spec = syn.make_spec(hwc, [(3, 1, 2)], (3, 1), 9, **kw)
    elif case == "head_only":
        spec = syn.make_spec(hwc, [], (3, 1), 9, **kw)
    elif case == "dense_ard":
        spec = syn.make_spec(hwc, [(3, 1, 2)], (3, 1), 9, head_kernel="rbf", **kw)
    X, Ylab = syn.make_batch(hwc, N, seed=seed)
    zs = syn.make_noise(spec, N, seed=seed)
    return spec, X, np.asarray(Ylab, np.int32) % K, zs


def grad_block(ctx, model, li):
    ptr, n = C.c_void_p(), C.c_size_t()
    ctx._check(dev.lib().dcgp_model_grad_block(model._model, li, C.byref(ptr), C.byref(n)))
    host = np.empty(n.value)
    ctx._check(dev.lib().dcgp_d2h(ctx.handle, host.ctypes.data, ptr, host.nbytes))
    return host


# ---- stand-alone tails ----------------------------------------------------------------------------------------------------------------
def _varexp(ctx, m, v, y, nodes):
    n, K = m.shape
    dm, dv, dy, dn = ctx.to_device(m), ctx.to_device(v), ctx.to_device(y, np.int32), ctx.to_device(nodes)
    out = ctx.empty((n,))
    rc = dev.lib().dcgp_softmax_varexp(ctx.handle, dm.ptr, dv.ptr, dy.ptr, n, K, dn.ptr, nodes.shape[0], out.ptr)
    return rc, out.numpy()


def _predict(ctx, m, v, nodes):
    n, K = m.shape
    dm, dv, dn = ctx.to_device(m), ctx.to_device(v), ctx.to_device(nodes)
    out = ctx.empty((n, K))
    rc = dev.lib().dcgp_softmax_predict(ctx.handle, dm.ptr, dv.ptr, n, K, dn.ptr, nodes.shape[0], out.ptr)
    return rc, out.numpy()


@pytest.mark.parametrize("K", [2, 3, 10, 17])
def test_standalone_tails_vs_numpy(ctx, K):
    """dcgp_softmax_varexp / _predict against NumPy, relative error <= 1e-10: Q on both sides of the 16-node chunks, a wave and the
    workgroup's items, row counts that are no multiple of a workgroup's rows, a row with v = 0 exactly and rows with mu up to +-800 (compared
    on their own: their expectations are ~ -1600 and would hide an error in the ordinary rows under a max-norm)."""
    rng = np.random.default_rng(100 + K)
    for Q in (1, 2, 64, 65, 100, 130):
        nodes = Softmax(K, Q, seed=Q).nodes
        for n in (1, 7, 300):
            m, v = 2.0 * rng.standard_normal((n, K)), rng.random((n, K)) + 0.01
            y = rng.integers(0, K, n).astype(np.int32)
            extreme = np.zeros(n, bool)
            if n > 1:
                v[1] = 0.0                                                  # the clamp
                v[2, 0] = 0.0
                m[3] = 800.0 * np.where(rng.random(K) < 0.5, -1.0, 1.0)     # +-800 in every class
                m[4], m[5] = -800.0, 800.0
                m[4, y[4]], m[5, (y[5] + 1) % K] = 800.0, -800.0 + 3.0
                extreme[3:6] = True
            rc, ve = _varexp(ctx, m, v, y, nodes)
            assert rc == dev.DCGP_OK
            want = sr.variational_expectations(m, v, y, nodes)
            assert np.all(np.isfinite(ve)) and np.all(np.isfinite(want))
            rc, p = _predict(ctx, m, v, nodes)
            assert rc == dev.DCGP_OK
            wp = sr.predict_mean_and_var(m, v, nodes)[0]
            assert np.all(np.isfinite(p)) and np.abs(p.sum(1) - 1.0).max() < 1e-13
            for rows in (extreme, ~extreme):
                if rows.any():
                    assert rel(ve[rows], want[rows]) <= 1e-10, (K, Q, n, rel(ve[rows], want[rows]))
                    assert rel(p[rows], wp[rows]) <= 1e-10, (K, Q, n, rel(p[rows], wp[rows]))
            rc2, ve2 = _varexp(ctx, m, v, y, nodes)                          # the same bits on a second call
            assert rc2 == dev.DCGP_OK and np.array_equal(ve, ve2) and np.array_equal(p, _predict(ctx, m, v, nodes)[1])


def test_standalone_limits(ctx):
    rng = np.random.default_rng(5)

    def case(K, Q, n=3):
        return rng.standard_normal((n, max(K, 1))), rng.random((n, max(K, 1))) + 0.1, np.zeros(n, np.int32), rng.standard_normal((max(Q, 1), max(K, 1)))
    for K, Q in ((2, 2048), (4096, 1), (64, 64)):                            # Q * K = 4096: accepted
        m, v, y, nodes = case(K, Q)
        rc, ve = _varexp(ctx, m, v, y, nodes)
        assert rc == dev.DCGP_OK and rel(ve, sr.variational_expectations(m, v, y, nodes)) <= 1e-10, (K, Q)
        rc, p = _predict(ctx, m, v, nodes)
        assert rc == dev.DCGP_OK and rel(p, sr.predict_mean_and_var(m, v, nodes)[0]) <= 1e-10, (K, Q)
    L = dev.lib()
    m, v, y, nodes = case(17, 241)                                           # Q * K = 4097
    assert _varexp(ctx, m, v, y, nodes)[0] == dev.ERR_ARG and _predict(ctx, m, v, nodes)[0] == dev.ERR_ARG
    with pytest.raises(dev.DcgpError) as err:
        ctx._check(_varexp(ctx, m, v, y, nodes)[0])
    assert "4096" in str(err.value)
    m, v, y, nodes = case(3, 4)
    dm, dv, dy, dn, out = ctx.to_device(m), ctx.to_device(v), ctx.to_device(y, np.int32), ctx.to_device(nodes), ctx.empty((3, 3))
    assert L.dcgp_softmax_varexp(ctx.handle, dm.ptr, dv.ptr, dy.ptr, 3, 1, dn.ptr, 4, out.ptr) == dev.ERR_ARG      # K = 1
    assert L.dcgp_softmax_varexp(ctx.handle, dm.ptr, dv.ptr, dy.ptr, 3, 3, dn.ptr, 0, out.ptr) == dev.ERR_ARG      # Q = 0
    assert L.dcgp_softmax_predict(ctx.handle, dm.ptr, dv.ptr, 3, 1, dn.ptr, 4, out.ptr) == dev.ERR_ARG
    assert L.dcgp_softmax_predict(ctx.handle, dm.ptr, dv.ptr, 3, 3, dn.ptr, 0, out.ptr) == dev.ERR_ARG
    assert _varexp(ctx, m, v, np.array([0, 3, 1], np.int32), nodes)[0] == dev.ERR_ARG                               # a label K
    assert _varexp(ctx, m, v, np.array([0, -1, 1], np.int32), nodes)[0] == dev.ERR_ARG
    assert _varexp(ctx, m, v, np.array([0, 2, 1], np.int32), nodes)[0] == dev.DCGP_OK


# ---- ELBO -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,white", [("conv", False), ("conv", True), ("head_only", False), ("head_only", True), ("dense_ard", False),
                                        ("dense_ard", True)])
@pytest.mark.parametrize("K", [3, 10])
@pytest.mark.parametrize("dedup", [False, True])
def test_elbo_vs_numpy(ctx, case, white, K, dedup):
    spec, X, Y, zs = make_case(case, K, white)
    lik = Softmax(K, 100, seed=3)
    want, wdata, wkl = sr.elbo(spec, X, Y, zs, lik.nodes)
    model = build_from_spec(spec, X, Y, likelihood=lik)
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
    # an enqueued step never keeps its chain for a later one (any likelihood): the next synchronous step runs it again and keeps it
    k1 = model.chain_skips
    assert k1 == k0 + 1
    assert model.compute_log_likelihood(X, Y, zs=zs, return_parts=True) == (e, data, kl)
    assert model.chain_skips == k1
    # a new table (another Q as well): the value changes, the chain of the step in front of the call stands
    lik.nodes = Softmax(K, 37, seed=11).nodes
    model.push_likelihood_nodes()
    e2, data2, kl2 = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    assert model.chain_skips == k1 + 1 and kl2 == kl and data2 != data
    want2 = sr.elbo(spec, X, Y, zs, lik.nodes)
    assert abs(e2 - want2[0]) <= 1e-10 * abs(want2[0]) and abs(data2 - want2[1]) <= 1e-10 * abs(want2[1])
    lik.resample(5)                                                          # resample() pushes to the attached model
    assert lik.nodes.shape == (37, K)
    e3 = model.compute_log_likelihood(X, Y, zs=zs)
    assert abs(e3 - sr.elbo(spec, X, Y, zs, lik.nodes)[0]) <= 1e-10 * abs(e3) and e3 != e2
    model.close()


# ---- gradients ------------------------------------------------------------------------------------------------------------------------
def _torch_softmax_elbo(spec, X, Y, zs, nodes):
    """(ELBO, leaves) in torch: the layers of test_oracle_autograd._torch_elbo (its KL recovered from its RobustMax ELBO), the softmax rule
    written here."""
    import torch
    import test_oracle_autograd as ta
    e_rm, leaves, m, v = ta._torch_elbo(spec, X, Y, zs, want_head=True)
    S, N = spec["S"], X.shape[0]
    y = torch.tensor(np.tile(np.asarray(Y).reshape(1, N), [S, 1]).reshape(S * N), dtype=torch.long)
    ve_rm = ta._robustmax_ve(m.reshape(S * N, -1), v.reshape(S * N, -1), y).reshape(S, N).mean(0).sum()
    kl = ve_rm * (spec["num_data"] / N) - e_rm
    return _torch_rule(m, v, Y, nodes, "elbo").sum() * (spec["num_data"] / N) - kl, leaves


def _torch_rule(m, v, Y, nodes, objective):
    """J [N] from the head's marginals m, v [S, N, K] (torch): "elbo" 1/S sum_s ve_sn, "density" log(1/S sum_s p_sn[y])."""
    import torch
    S, N, K = m.shape
    e = torch.tensor(np.asarray(nodes, np.float64))
    f = m[:, :, None, :] + torch.sqrt(torch.clamp(v, min=1e-10))[:, :, None, :] * e           # [S, N, Q, K]
    lsm = torch.log_softmax(f, -1)
    idx = torch.tensor(np.asarray(Y, np.int64).reshape(-1))
    ly = lsm[:, torch.arange(N), :, idx]                                                       # [N, S, Q]
    if objective == "elbo":
        return ly.mean(2).mean(1)
    return torch.log(torch.exp(ly).mean(2).mean(1))


def _torch_gradients(spec, X, Y, zs, nodes):
    import torch
    e_t, leaves = _torch_softmax_elbo(spec, X, Y, zs, nodes)
    flat = [(li, k, t) for li, p in enumerate(leaves) for k, t in p.items()]
    tg = torch.autograd.grad(e_t, [t for _, _, t in flat])
    want = [{} for _ in leaves]
    for (li, k, _), g in zip(flat, tg):
        want[li][k] = np.tril(g.numpy()) if k == "q_sqrt" else g.numpy().copy()
    return e_t.item(), want


@pytest.mark.parametrize("case", ["conv", "dense_ard"])
def test_gradient_vs_torch_autograd(ctx, case):
    pytest.importorskip("torch")
    spec, X, Y, zs = make_case(case, 3, N=3, S=2, seed=11)
    lik = Softmax(3, 100, seed=1)
    e_t, want = _torch_gradients(spec, X, Y, zs, lik.nodes)
    model = build_from_spec(spec, X, Y, likelihood=lik)
    e, g = model.compute_gradients(X, Y, zs=zs)
    assert abs(e - e_t) <= 1e-10 * abs(e_t)
    for li, groups in enumerate(want):
        for name, w in groups.items():
            got = np.tril(g[li][name]) if name == "q_sqrt" else g[li][name]
            err = np.abs(got - w).max()
            print("softmax grad %s L%d %-14s |err| %.3e |want| %.3e" % (case, li, name, err, np.abs(w).max()))
            assert err <= 1e-8 * max(1.0, np.abs(w).max()), (li, name, err)
    assert "likelihood_variance" not in g[-1]
    # two identical calls: bitwise identical gradient blocks, of the length the same spec has under MultiClass
    blocks = []
    for _ in range(2):
        model.compute_gradients(X, Y, zs=zs, fetch=False)
        blocks.append([grad_block(ctx, model, li) for li in range(len(model.layers))])
    rm = build_from_spec(spec, X, Y, likelihood=MultiClass(3))
    rm.compute_gradients(X, Y, zs=zs, fetch=False)
    for li in range(len(model.layers)):
        assert np.array_equal(blocks[0][li], blocks[1][li]), li
        assert blocks[0][li].size == grad_block(ctx, rm, li).size, li
    model.close(), rm.close()


# ---- optimisers -----------------------------------------------------------------------------------------------------------------------
def _close(got, want):
    return np.abs(np.asarray(got) - np.asarray(want)).max() <= 1e-8 * max(1.0, np.abs(want).max())


@pytest.fixture(scope="module")
def opt_case():
    spec, X, Y, zs = make_case("conv", 3, N=4, S=2, seed=3)
    nodes = Softmax(3, 100, seed=2).nodes
    return spec, X, Y, zs, nodes, _torch_gradients(spec, X, Y, zs, nodes)[1]


def test_adam_step_follows_the_autograd_gradient(ctx, opt_case):
    import copy
    spec, X, Y, zs, nodes, want = opt_case
    moved = copy.deepcopy(spec)
    ls.adam_numpy_step(moved, want, {}, 0.01, 1)
    model = build_from_spec(spec, X, Y, likelihood=Softmax(3, nodes=nodes))
    model.train_step(X, Y, 0.01, zs=zs)
    model.pull_parameters()
    for li, (l, now) in enumerate(zip(moved["convs"] + [moved["head"]], ls.model_values(model))):
        for name in now:
            assert _close(now[name], l[ls.SPEC_KEY[name]]), (li, name, np.abs(now[name] - l[ls.SPEC_KEY[name]]).max())
    model.close()


def test_sgd_step_follows_the_autograd_gradient(ctx, opt_case):
    spec, X, Y, zs, nodes, want = opt_case
    lr = 1e-3
    model = build_from_spec(spec, X, Y, likelihood=Softmax(3, nodes=nodes))
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.sgd_step(lr)
    model.pull_parameters()
    for li, (l, now) in enumerate(zip(spec["convs"] + [spec["head"]], ls.model_values(model))):
        for name, w in want[li].items():
            x = np.asarray(l[ls.SPEC_KEY[name]], np.float64)
            if name in ls.POSITIVE:
                expect = np.log1p(np.exp(ls.softplus_inv(x) + lr * w * (1.0 - np.exp(-(x - 1e-6))))) + 1e-6
            else:
                expect = x + lr * w
            assert _close(now[name], expect), (li, name)
            assert not np.array_equal(now[name], x), (li, name)
    model.close()


def test_natgrad_step_follows_the_autograd_gradient(ctx, opt_case):
    from natgrad_ref import natgrad_reference
    spec, X, Y, zs, nodes, want = opt_case
    gamma = 1e-4
    model = build_from_spec(spec, X, Y, likelihood=Softmax(3, nodes=nodes))
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.natgrad_step(gamma)
    model.pull_parameters()
    for li, (l, m) in enumerate(zip(spec["convs"] + [spec["head"]], model.layers)):
        mu1, L1 = natgrad_reference(np.asarray(l["q_mu"]), np.asarray(l["q_sqrt"]), want[li]["q_mu"], want[li]["q_sqrt"], gamma)
        assert _close(m.q_mu, mu1) and _close(m.q_sqrt, L1), (li, np.abs(m.q_mu - mu1).max(), np.abs(m.q_sqrt - L1).max())
        assert not np.array_equal(m.q_mu, np.asarray(l["q_mu"]))
    model.close()


@pytest.mark.parametrize("optimizer", ["Adam", "SGD", "NatGrad"])
def test_train_keeps_the_elbo_finite(ctx, optimizer):
    spec, X, Y, zs = make_case("conv", 3, N=8, S=2, seed=5)
    m = build_from_spec(spec, X, Y, likelihood=Softmax(3, 20, seed=1))
    m.minibatch_size = 4
    hist = train(m, 20, lr=0.01, optimizer=optimizer)
    assert len(hist) == 20 and np.all(np.isfinite(hist))
    assert np.isfinite(m.compute_log_likelihood(X, Y, zs=zs))
    m.close()


# ---- predictions, evaluation, uncertainty -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pred_case():
    spec, X, Y, zs = make_case("conv", 10, N=7, S=3, seed=9)
    nodes = Softmax(10, 100, seed=4).nodes
    _, fm, fv = sr.head(spec, X, Y, zs)
    return spec, X, Y, zs, nodes, sr.predict_mean_and_var(fm, fv, nodes), sr.predict_density(fm, fv, Y, nodes)


def test_predictions_vs_numpy(ctx, pred_case):
    spec, X, Y, zs, nodes, (wp, wv), wld = pred_case
    model = build_from_spec(spec, X, Y, likelihood=Softmax(10, nodes=nodes))
    p, pv = model.predict_y(X, 3, zs=zs)
    assert p.shape == (3, 7, 10) and rel(p, wp) <= 1e-10 and rel(pv, wv) <= 1e-10 and np.abs(p.sum(-1) - 1).max() < 1e-13
    ld = model.predict_density(X, Y, 3, zs=zs)
    assert ld.shape == (7, 1) and rel(ld[:, 0], wld) <= 1e-10
    assert rel(model.predict_proba(X, 3, zs=zs), wp.mean(0)) <= 1e-10
    model.close()


@pytest.mark.parametrize("batch", [1, 3, 7, 32])
def test_evaluate_and_uncertainty(ctx, pred_case, batch):
    spec, X, Y, zs, nodes, (wp, wv), wld = pred_case
    model = build_from_spec(spec, X, Y, likelihood=Softmax(10, nodes=nodes))
    out = model.evaluate(X, Y, S=3, batch_size=batch, zs=zs, per_image=True)
    wpm = wp.mean(0)
    assert rel(out["log_density"], wld) <= 1e-10 and rel(out["p_mean"], wpm) <= 1e-10
    assert out["accuracy"] == np.mean(wpm.argmax(1) == Y) and out["n"] == 7
    assert abs(out["mean_log_density"] - wld.mean()) <= 1e-10 * abs(wld.mean())
    assert np.array_equal(model.predict_density(X, Y, 3, zs=zs)[:, 0], out["log_density"])
    unc = model.evaluate_uncertainty(X, Y, S=3, batch_size=batch, zs=zs, bins=5, per_image=True)
    for k in ("accuracy", "mean_log_density", "n"):
        assert unc[k] == out[k], k
    assert np.array_equal(unc["log_density"], out["log_density"]) and np.array_equal(unc["p_mean"], out["p_mean"])
    ps = model.predict_y(X, 3, zs=zs)[0]
    host = Softmax.predictive_uncertainty(ps)
    assert np.abs(unc["p_mean"] - host["p_mean"]).max() <= 1e-15 and np.array_equal(unc["prediction"], host["prediction"])
    assert np.abs(unc["confidence"] - host["confidence"]).max() <= 1e-15
    for k in ("predictive_entropy", "expected_entropy", "mutual_information"):
        assert np.abs(unc[k] - host[k]).max() <= 1e-12, k
    assert abs(unc["mean_predictive_entropy"] - host["predictive_entropy"].mean()) <= 1e-12
    assert abs(unc["mean_mutual_information"] - host["mutual_information"].mean()) <= 1e-12
    onehot = np.eye(10)[Y]
    assert abs(unc["brier"] - np.square(host["p_mean"] - onehot).sum(1).mean()) <= 1e-12
    b = np.minimum(4, np.floor(host["confidence"] * 5).astype(int))
    hit = host["prediction"] == Y
    count = np.bincount(b, minlength=5)
    assert np.array_equal(unc["reliability"]["count"], count)
    ece = 0.0
    for i in range(5):
        if count[i]:
            assert abs(unc["reliability"]["confidence"][i] - host["confidence"][b == i].mean()) <= 1e-12
            assert abs(unc["reliability"]["accuracy"][i] - hit[b == i].mean()) <= 1e-12
            ece += count[i] / 7.0 * abs(hit[b == i].mean() - host["confidence"][b == i].mean())
    assert abs(unc["ece"] - ece) <= 1e-12
    if batch == 7:      # one batch of all images: predict_uncertainty without labels gives the same per-image values
        free = model.predict_uncertainty(X, 3, zs=zs)
        for k in ("p_mean", "predictive_entropy", "expected_entropy", "mutual_information", "confidence", "prediction"):
            assert np.array_equal(free[k], unc[k]), k
        assert AccuracyLogger(X, Y, batch_size=7, num_samples=3)(model) == model.evaluate(X, Y, S=3, batch_size=7)["accuracy"]
        assert TestLogDensityLogger(X, Y, batch_size=7, num_samples=3)(model) == model.evaluate(X, Y, S=3, batch_size=7)["mean_log_density"]
        assert UncertaintyLogger(X, Y, S=3, bins=5, batch_size=7)(model)["ece"] == model.evaluate_uncertainty(X, Y, S=3, batch_size=7, bins=5)["ece"]
    model.close()


# ---- input gradients --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["conv", "head_only"])      # (dense_ard at this lengthscale has no live pixel gradient: 1e-19)
@pytest.mark.parametrize("objective", ["density", "elbo"])
def test_input_gradient_vs_torch_autograd(ctx, case, objective):
    torch = pytest.importorskip("torch")
    import input_grad_ref as ig
    spec, X, Y, zs = make_case(case, 10 if case == "conv" else 3, N=4, S=3, seed=13)
    lik = Softmax(spec["head"]["R"], 100, seed=6)
    Xt = torch.tensor(X, dtype=torch.float64, requires_grad=True)
    m, v = ig.head_marginals(spec, Xt, zs)
    Jt = _torch_rule(m, v, Y, lik.nodes, objective)
    (gt,) = torch.autograd.grad(Jt.sum(), Xt)
    Jt, gt = Jt.detach().numpy(), gt.numpy()
    model = build_from_spec(spec, X, Y, likelihood=lik)
    J, g = model.input_gradient(X, Y, objective=objective, zs=zs)
    print("softmax input_grad %s %s |dJ| %.3e |dg| %.3e |g| %.3e" % (case, objective, np.abs(J - Jt).max(), np.abs(g - gt).max(), np.abs(gt).max()))
    assert np.abs(J - Jt).max() <= 1e-8 * max(1.0, np.abs(Jt).max())
    assert np.abs(g - gt).max() <= 1e-8 * max(1.0, np.abs(gt).max())
    assert np.abs(gt).max() > 1e-6                                           # (a live gradient)
    J2, g2 = model.input_gradient(X, Y, objective=objective, zs=zs)
    assert np.array_equal(J, J2) and np.array_equal(g, g2)
    if objective == "density":
        assert np.array_equal(J, model.predict_density(X, Y, spec["S"], zs=zs)[:, 0])
    model.close()


def test_saliency_and_adversarial_examples(ctx):
    spec, X, Y, zs = make_case("conv", 10, N=5, S=3, seed=17)
    model = build_from_spec(spec, X, Y, likelihood=Softmax(10, 50, seed=2))
    sal = model.saliency(X, Y, zs=zs)
    assert sal.shape == (5, 10, 10, 1) and np.array_equal(sal.reshape(5, -1), model.input_gradient(X, Y, zs=zs)[1])
    assert model.saliency(X, zs=zs).shape == (5, 10, 10, 1)                  # the model's own prediction as the label
    for objective in ("density", "elbo"):
        J0, _ = model.input_gradient(X, Y, objective=objective, zs=zs)
        adv = adversarial_examples(model, X, Y, 0.05, objective=objective, zs=zs)
        assert np.abs(adv - X).max() <= 0.05 + 1e-15
        J1, _ = model.input_gradient(adv, Y, objective=objective, zs=zs)
        assert np.all(J1 < J0), (objective, J0, J1)
    model.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------------------
def test_error_paths(ctx):
    spec, X, Y, zs = make_case("conv", 3, N=4, S=2, seed=2)
    L = dev.lib()
    model = build_from_spec(spec, X, Y, likelihood=Softmax(3, 10))
    model._build()
    dX, dY, dYf = ctx.to_device(X), ctx.to_device(Y, np.int32), ctx.to_device(np.eye(3)[Y])
    out, info = (C.c_double * 3)(), C.c_int(0)
    # float targets, and the _f64y entry points, on a Softmax model
    assert L.dcgp_elbo_forward_f64y(model._model, dX.ptr, dYf.ptr, 4, 1.0, None, 0, 0, out, C.byref(info)) == dev.ERR_ARG
    assert L.dcgp_elbo_grad_f64y(model._model, dX.ptr, dYf.ptr, 4, 1.0, None, 0, 0, out, C.byref(info)) == dev.ERR_ARG
    ld = ctx.empty((4, 3))
    assert L.dcgp_model_predict_density_f64y(model._model, dX.ptr, dYf.ptr, 4, 2, None, 0, ld.ptr, C.byref(info)) == dev.ERR_ARG
    assert L.dcgp_model_predict_mean_var(model._model, dX.ptr, 4, 2, None, 0, ld.ptr, None, C.byref(info)) == dev.ERR_ARG
    assert L.dcgp_model_input_grad_f64y(model._model, dX.ptr, dYf.ptr, 4, 2, None, 0, 1, None, ctx.empty((4, 100)).ptr, C.byref(info)) == dev.ERR_ARG
    with pytest.raises(ValueError):
        model.input_gradient(X, np.array([0, 1, 2, 3]), zs=zs)      # a label K, checked on the host
    with pytest.raises(dev.DcgpError):          # a label K, checked on the device
        model.evaluate(X, np.array([0, 3, 1, 2]), S=2)
    # the table: limits, an enqueued step outstanding, a model of another kind
    bad = np.zeros((1366, 3))                   # Q * K = 4098
    assert L.dcgp_model_set_likelihood_nodes(model._model, bad.ctypes.data, 1366) == dev.ERR_ARG
    assert L.dcgp_model_set_likelihood_nodes(model._model, bad.ctypes.data, 0) == dev.ERR_ARG
    assert L.dcgp_model_set_likelihood_nodes(model._model, None, 5) == dev.ERR_ARG
    t = model.enqueue_log_likelihood(X, Y, zs=zs)
    assert L.dcgp_model_set_likelihood_nodes(model._model, bad.ctypes.data, 5) == dev.ERR_ARG
    e = model.collect_log_likelihood(t)
    assert e == model.compute_log_likelihood(X, Y, zs=zs)
    rm = build_from_spec(spec, X, Y, likelihood=MultiClass(3))
    rm._build()
    assert L.dcgp_model_set_likelihood_nodes(rm._model, bad.ctypes.data, 5) == dev.ERR_ARG
    # a Softmax model at the C level before any nodes are set: every step is refused, then works once they are
    assert L.dcgp_model_set_likelihood(rm._model, 3, 0.0) == dev.DCGP_OK
    assert L.dcgp_elbo_forward(rm._model, dX.ptr, dY.ptr, 4, 1.0, None, 0, 0, out, C.byref(info)) == dev.ERR_ARG
    assert L.dcgp_elbo_grad(rm._model, dX.ptr, dY.ptr, 4, 1.0, None, 0, 0, out, C.byref(info)) == dev.ERR_ARG
    assert L.dcgp_model_train_step_adam(rm._model, dX.ptr, dY.ptr, 4, 1.0, None, 0, 0, 0.01, 0.9, 0.999, 1e-8, 0, out, C.byref(info)) == dev.ERR_ARG
    p = ctx.empty((2 * 4, 3))
    assert L.dcgp_model_predict_y(rm._model, dX.ptr, 4, 2, None, 0, p.ptr, None, C.byref(info)) == dev.ERR_ARG
    one = ctx.empty((4,))
    assert L.dcgp_model_evaluate(rm._model, dX.ptr, dY.ptr, 4, 4, 2, None, 0, one.ptr, None, out, C.byref(info)) == dev.ERR_ARG
    assert L.dcgp_model_input_grad(rm._model, dX.ptr, dY.ptr, 4, 2, None, 0, 0, one.ptr, ctx.empty((4, 100)).ptr, C.byref(info)) == dev.ERR_ARG
    nodes = np.ascontiguousarray(model.likelihood.nodes)
    assert L.dcgp_model_set_likelihood_nodes(rm._model, nodes.ctypes.data, nodes.shape[0]) == dev.DCGP_OK
    assert L.dcgp_elbo_forward(rm._model, dX.ptr, dY.ptr, 4, 75.0, None, 0, 0, out, C.byref(info)) == dev.DCGP_OK
    assert np.isfinite(out[0])
    assert L.dcgp_model_set_likelihood(rm._model, 4, 0.0) == dev.ERR_ARG
    model.close(), rm.close()


# ---- real images --------------------------------------------------------------------------------------------------------------------------
def test_learns_the_digits_beside_robustmax(ctx):
    """sklearn's 8 x 8 digits, ten classes, tools/digits_train.py's "conv" variant and flags: a --likelihood softmax model and a robustmax
    model trained for the same 500 Adam steps from the same seeds.  The yardstick is the RobustMax model (existing code): the Softmax
    model's test accuracy must come within 0.02 of it -- about two binomial standard deviations at ~0.97 on the held-out images -- and its
    mean log density must rise.  ECE, Brier score and mean log density of both are printed, not ordered."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from digits_train import VARIANTS, digits
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder
    Xtr, Ytr, Xte, Yte = digits()
    Xte = Xte.reshape(len(Xte), -1)
    res = {}
    for kind in ("softmax", "robustmax"):
        flags = default_parser().parse_args(["--name", "digits", "--batch-size", "64", "--lr", "0.01", "--num-samples", "5", "--likelihood", kind]
                                            + VARIANTS["conv"])
        np.random.seed(0)
        model = ModelBuilder(flags, Xtr, Ytr.reshape(-1, 1)).build()
        assert isinstance(model.likelihood, Softmax if kind == "softmax" else MultiClass)
        before = model.evaluate(Xte, Yte, S=5)
        train(model, 500, lr=0.01, lr_decay_steps=10 ** 9)
        out = model.evaluate_uncertainty(Xte, Yte, S=5)
        print("digits %-9s test accuracy %.4f (untrained %.4f), mean log density %.4f (untrained %.4f), ECE %.4f, Brier %.4f"
              % (kind, out["accuracy"], before["accuracy"], out["mean_log_density"], before["mean_log_density"], out["ece"], out["brier"]))
        assert AccuracyLogger(Xte, Yte)(model) == model.evaluate(Xte, Yte, S=5)["accuracy"] == out["accuracy"]
        res[kind] = (before, out)
        model.close()
    assert res["softmax"][1]["accuracy"] >= res["robustmax"][1]["accuracy"] - 0.02, res
    assert res["softmax"][1]["mean_log_density"] > res["softmax"][0]["mean_log_density"], res

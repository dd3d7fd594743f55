"""The linear convolutional mean function on the device (``LinearConv2dMean``, dcgp_model_set_mean_filter; csrc/conv_mean.hip) against the CPU
references of tests/conv_mean_ref.py: the unmodified oracle with a NumPy mean attached (forward; gradients of the unpadded stacks through
``oracle.grad.elbo_and_grad`` plus ``filter_grad()``) and torch autograd of the padded forward with the filter as a leaf (gradients of the
padded stacks -- ``elbo_and_grad`` knows no padded layer --, the Matern-5/2 stack, the input gradient).  The two references agree without a
GPU (tests/test_host_conv_mean.py).

The mean is one more term of a layer's mean, so every bound is the one the tests without it use for the same quantity: RTOL of
tests/test_gpu_model.py (ELBO, data term, KL, class probabilities, two routes of one model), RTOL of tests/test_gpu_ops.py (layer outputs),
TOL_GROUP / TOL_E of tests/test_gpu_grad_m256.py (of tests/test_gpu_grad_large_m.py for ``m264``), the input gradient's
1e-7 * max(1, |want|max) of tests/test_gpu_input_grad.py, RTOL of tests/test_gpu_evaluate.py, and the bit-identity of
tests/test_gpu_train_run.py.  Every figure is printed before it is asserted (run with -s).  The stacks are conv_mean_ref.CASES; N = 3, S = 2,
explicit noise."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.models import build_from_spec
import conv_mean_ref as R
import live_specs as ls
import stack_specs as ss
import test_gpu_grad_large_m as large_m
import test_gpu_grad_m256 as m256
from test_gpu_evaluate import RTOL as RTOL_EVAL, oracle_log_density
from test_gpu_model import RTOL
from test_gpu_ops import RTOL as RTOL_OPS
import torch_ref as tr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]   # a hung launch ends the run instead of holding the device

INPUT_GRAD_TOL = 1e-7      # tests/test_gpu_input_grad.py: |dX - autograd|max <= 1e-7 * max(1, |autograd|max)

# (stack, base kernel of the conv layers)
FORWARD = [("ch_res", None), ("ch_res_white", None), ("even_s2", None), ("wide_R", None), ("m264", None), ("ch_res", "acos"), ("ch_res", "matern52")]
GRAD = FORWARD + [("valid2", None), ("valid2", "acos")]


def _id(case):
    return case[0] + ("" if case[1] is None else "-" + case[1])


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def grad_bounds(spec):
    mod = large_m if any(l["M"] > 256 for l in spec["convs"] + [spec["head"]]) else m256
    return mod.TOL_GROUP, mod.TOL_E


@functools.lru_cache(maxsize=None)
def _case(name, base=None):
    """(spec, X, Y, zs) of a stack with trainable filters, once per process; never written to."""
    return R.make_case(name, base=base)


@functools.lru_cache(maxsize=None)
def _forward_ref(name, base=None):
    """ELBO parts, every conv layer's sample (and mean / variance where the oracle gives them), the head's mean and variance, class
    probabilities.  The oracle where it knows the base kernel, the torch forward for Matern."""
    spec, X, Y, zs = _case(name, base)
    if base == "matern52":
        import torch
        from test_oracle_autograd import _robustmax_predict
        with torch.no_grad():
            out = tr.forward(spec, X, Y, zs)
            S, N, K = out["mean"].shape
            p = _robustmax_predict(out["mean"].reshape(S * N, K), out["var"].reshape(S * N, K)).reshape(S, N, K).numpy()
        Fs = [f.numpy().reshape(S, N, -1) for f in out["F"]]
        return dict(parts=(out["elbo"].item(), out["data"].sum().item(), out["kl"].item()), Fs=Fs, Fm=None, Fv=None,
                    head=(out["mean"].numpy(), out["var"].numpy()), p=p)
    ref, _ = R.oracle_model(spec, X, Y)
    Fs, Fm, Fv = ref.propagate(X, S=spec["S"], zs=zs)
    p, _ = ref.predict_y(X, spec["S"], zs=zs)
    return dict(parts=(ref.compute_log_likelihood(X, Y, zs=zs), ref.data_term(X, Y, zs=zs), ref.KL()), Fs=Fs[:-1], Fm=Fm, Fv=Fv,
                head=(Fm[-1], Fv[-1]), p=p)


@functools.lru_cache(maxsize=None)
def _grad_ref(name, base=None):
    """((ELBO, ...), [per-layer {group: gradient}]): elbo_and_grad + filter_grad() on the unpadded stacks, torch autograd on the others."""
    spec, X, Y, zs = _case(name, base)
    if name == "valid2":
        e, grads = R.oracle_gradient(spec, X, Y, zs)
        for g in grads:
            g["q_sqrt"] = np.tril(g["q_sqrt"])
        return (e,), grads
    pytest.importorskip("torch")
    t = tr.reference(spec, X, Y, zs)
    return t["parts"], t["want"]


# ---- 1. forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedup", [False, True], ids=["tiled", "dedup"])
@pytest.mark.parametrize("case", FORWARD, ids=_id)
def test_stacks_match_the_reference(ctx, case, dedup):
    """ELBO, data term, KL, predict_y and every layer's sample, mean and variance; a second step (the other bank) gives the same bits."""
    spec, X, Y, zs = _case(*case)
    o = _forward_ref(*case)
    tag = _id(case) + ("-dedup" if dedup else "")
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    assert all(l.filter_mean is not None and not l.identity_mean and l.generic_mean is None for l in model.layers[:-1])
    got = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    for what, g, w in zip(("elbo", "data", "kl"), got, o["parts"]):
        print("%s %-4s device %.9f reference %.9f rel %.3e" % (tag, what, g, w, abs(g - w) / max(abs(w), 1.0)))
    Fs, Fm, Fv = model.propagate(X, S=spec["S"], zs=zs)
    p, _ = model.predict_y(X, spec["S"], zs=zs)
    rows = []
    for i in range(len(Fm) - 1):
        rows.append(("layer %d sample" % i, rel(Fs[i], o["Fs"][i])))
        if o["Fm"] is not None:
            rows += [("layer %d mean" % i, rel(Fm[i], o["Fm"][i])), ("layer %d var" % i, rel(Fv[i], o["Fv"][i]))]
    rows += [("head mean", rel(Fm[-1], o["head"][0])), ("head var", rel(Fv[-1], o["head"][1]))]
    for what, err in rows:
        print("%s %-16s %.3e" % (tag, what, err))
    print("%s predict_y %.3e" % (tag, rel(p, o["p"])))
    e, data, kl = o["parts"]
    assert abs(got[0] - e) <= RTOL * abs(e) and abs(got[1] - data) <= RTOL * abs(data) and abs(got[2] - kl) <= RTOL * max(abs(kl), 1.0), (got, o["parts"])
    for what, err in rows:
        assert err < RTOL_OPS, (tag, what, err)
    assert rel(p, o["p"]) < RTOL
    assert model.compute_log_likelihood(X, Y, zs=zs, return_parts=True) == got
    model.close()


# ---- 2. gradients -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedup", [False, True], ids=["tiled", "dedup"])
@pytest.mark.parametrize("case", GRAD, ids=_id)
def test_gradient_of_every_group_including_the_filter(ctx, case, dedup):
    spec, X, Y, zs = _case(*case)
    ref, want = _grad_ref(*case)
    tol_group, tol_e = grad_bounds(spec)
    tag = _id(case) + ("-dedup" if dedup else "")
    ls.assert_live(tag, want)                    # every group of the reference, the filters' among them, is live
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    e, grads = model.compute_gradients(X, Y, zs=zs)
    e2, grads2 = model.compute_gradients(X, Y, zs=zs)
    rows = []
    for li, groups in enumerate(want):
        assert set(groups) == set(grads[li]), (tag, li, sorted(groups), sorted(grads[li]))
        for gname, w in groups.items():
            got = np.asarray(grads[li][gname], np.float64)
            assert got.shape == np.shape(w), (tag, li, gname, got.shape, np.shape(w))
            rows.append((li, gname) + ls.errors(gname, got, w))
            print("%s L%d %-16s group %.3e  entry %.3e  |want|max %.3e" % ((tag,) + rows[-1] + (np.abs(w).max(),)))
    print("%s elbo rel %.3e  WORST group %.3e entry %.3e" % (tag, abs(e - ref[0]) / abs(e), max(r[2] for r in rows), max(r[3] for r in rows)))
    assert all("mean_filter" in g for g in grads[:-1]) and all(np.abs(g["mean_filter"]).max() > 0 for g in want[:-1])
    assert abs(e - ref[0]) <= RTOL * abs(e), (tag, e, ref[0])
    for li, gname, err_g, err_e in rows:
        assert err_g <= tol_group, (tag, li, gname, "group-wise", err_g)
        assert err_e <= tol_e, (tag, li, gname, "entry-wise", err_e)
    assert e == e2
    for a, b in zip(grads, grads2):
        for k in a:
            assert np.array_equal(a[k], b[k]), (tag, k, "repeat")
    model.close()


# ---- 3. input gradient --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedup", [False, True], ids=["tiled", "dedup"])
@pytest.mark.parametrize("name", ["ch_res", "even_s2", "wide_R"])
def test_input_gradient_has_the_means_term(ctx, name, dedup):
    pytest.importorskip("torch")
    spec, X, Y, zs = _case(name)
    Jw, want = tr.input_gradient(spec, X, Y, zs, tr.data_term)
    _, without = tr.input_gradient(R.without_filters(spec), X, Y, zs, tr.data_term)
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    J, got = model.input_gradient(X, Y, objective="elbo", zs=zs)
    err = np.abs(got - want).max()
    print("%s dedup=%d: |dX - autograd| %.3e  |want|max %.3e  J rel %.3e  (the mean's share of dX: %.3e)"
          % (name, dedup, err, np.abs(want).max(), rel(J, Jw), np.abs(want - without).max()))
    assert got.shape == X.shape == want.shape and J.shape == (X.shape[0],)
    assert np.abs(want - without).max() > 1e-3 * np.abs(want).max()          # the term under test is live
    assert rel(J, Jw) <= RTOL
    assert err <= INPUT_GRAD_TOL * max(1.0, np.abs(want).max()), (err, np.abs(want).max())
    model.close()


# ---- 4. centre0 is Conv2dMean by another route ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedup", [False, True], ids=["tiled", "dedup"])
def test_centre0_filter_is_the_conv2d_mean_model(ctx, dedup):
    spec, X, Y, zs = _case("ch_res")
    a = build_from_spec(R.add_filters(copy.deepcopy(spec), "centre0", trainable=True), X, Y)
    b = build_from_spec(R.without_filters(spec, mean_function="conv2d"), X, Y)
    assert all(l.identity_mean for l in b.layers[:-1]) and not any(l.identity_mean for l in a.layers[:-1])
    a.dedup_layer0 = b.dedup_layer0 = dedup
    pa, pb = (m.compute_log_likelihood(X, Y, zs=zs, return_parts=True) for m in (a, b))
    print("LinearConv2dMean(centre0) %r\n               Conv2dMean %r  bit-identical %s" % (pa, pb, pa == pb))
    for g, w in zip(pa, pb):
        assert abs(g - w) <= RTOL * max(abs(w), 1.0), (pa, pb)
    tol_group, tol_e = grad_bounds(spec)
    (_, ga), (_, gb) = (m.compute_gradients(X, Y, zs=zs) for m in (a, b))
    for li, groups in enumerate(gb):
        assert set(ga[li]) - set(groups) == ({"mean_filter"} if li < len(gb) - 1 else set())
        for gname, w in groups.items():
            err_g, err_e = ls.errors(gname, ga[li][gname], w)
            print("L%d %-14s group %.3e entry %.3e" % (li, gname, err_g, err_e))
            assert err_g <= tol_group and err_e <= tol_e, (li, gname, err_g, err_e)
    Ja, da = a.input_gradient(X, Y, objective="elbo", zs=zs)
    Jb, db = b.input_gradient(X, Y, objective="elbo", zs=zs)
    assert rel(Ja, Jb) <= RTOL and np.abs(da - db).max() <= INPUT_GRAD_TOL * max(1.0, np.abs(db).max())
    a.close(), b.close()


# ---- 5. training ----------------------------------------------------------------------------------------------------------------------
def _values(model):
    model.pull_parameters()
    return [(p.pathname, np.array(p.value)) for p in model.parameters]


def _train_models(trainable, dedup, n=2):
    spec, _, _, _ = R.make_case("ch_res", trainable=trainable)
    pool = 11
    X, _ = syn.make_batch(R.CASES["ch_res"]["hwc"], pool, seed=7)
    Y = np.random.default_rng(99).integers(0, 10, pool).astype(np.int32)
    models = []
    for _ in range(n):
        m = build_from_spec(copy.deepcopy(spec), X.copy(), Y.copy())
        m.dedup_layer0 = dedup
        models.append(m)
    return spec, X, Y, models


@pytest.mark.parametrize("dedup", [True, False], ids=["dedup", "tiled"])
def test_train_run_equals_the_loop_bit_for_bit_and_the_filter_moves(ctx, dedup):
    """Five Adam steps with trainable filters: ``train_run`` against five ``train_step`` calls, ELBOs and every parameter -- the filters among
    them -- to the bit; the filters have moved."""
    batch, steps = 4, 5
    spec, X, Y, (a, b) = _train_models(True, dedup)
    idx = np.stack([np.random.default_rng(5 + i).choice(len(X), batch, replace=False) for i in range(steps)])
    lrs = np.array([0.01, 0.01, 0.01, 0.001, 0.001])
    names = [p.pathname for p in a.parameters]
    assert "DGP/layers/0/mean_function/conv_filter" in names and "DGP/layers/1/mean_function/conv_filter" in names
    assert not any(n.startswith("DGP/layers/2/mean_function") for n in names)
    start = dict(_values(a))
    ha = np.array([a.train_step(a.X[idx[i]], a.Y[idx[i]], lrs[i], seed=11 + i) for i in range(steps)])
    b.attach_dataset()
    hb = b.train_run(idx, lrs, seed=11)
    print("loop %s\n run %s" % (ha, hb))
    assert np.all(np.isfinite(ha)) and np.array_equal(ha, hb)
    va, vb = _values(a), _values(b)
    assert [n for n, _ in va] == [n for n, _ in vb]
    for (name, x), (_, y) in zip(va, vb):
        assert np.array_equal(x, y), name
    for li in (0, 1):
        name = "DGP/layers/%d/mean_function/conv_filter" % li
        moved = np.abs(dict(va)[name] - start[name]).max()
        print("%s moved by %.3e" % (name, moved))
        assert moved > 1e-4 and dict(va)[name].shape == start[name].shape
    b.detach_dataset()
    a.close(), b.close()


def test_a_frozen_filter_stays_put_and_set_trainable_switches_it(ctx):
    spec, X, Y, (a,) = _train_models(False, True, n=1)
    start = dict(_values(a))
    zs = ss.make_noise(spec, 4, seed=3)
    for i in range(3):
        a.train_step(X[:4], Y[:4], 0.01, zs=zs)
    now = dict(_values(a))
    for li in (0, 1):
        name = "DGP/layers/%d/mean_function/conv_filter" % li
        assert np.array_equal(now[name], start[name]), name
    assert not np.array_equal(now["DGP/layers/0/q_mu"], start["DGP/layers/0/q_mu"])
    _, grads = a.compute_gradients(X[:4], Y[:4], zs=zs)
    assert not grads[0]["mean_filter"].any()                       # frozen: the gradient is not formed
    a.set_trainable(1, "mean_filter", True)
    assert a.layers[1].filter_mean.trainable and not a.layers[0].filter_mean.trainable
    a.train_step(X[:4], Y[:4], 0.01, zs=zs)
    now = dict(_values(a))
    assert np.array_equal(now["DGP/layers/0/mean_function/conv_filter"], start["DGP/layers/0/mean_function/conv_filter"])
    assert not np.array_equal(now["DGP/layers/1/mean_function/conv_filter"], start["DGP/layers/1/mean_function/conv_filter"])
    with pytest.raises(ValueError, match="LinearConv2dMean"):
        a.set_trainable(2, "mean_filter", True)
    a.close()


def test_sharded_adam_equals_adam_step_with_a_trainable_filter(ctx):
    """dcgp_model_debug_sharded_adam(ranks = 3) cuts every layer's block -- the filter's slots at its end included -- as three ranks would, and
    lands on the parameters of dcgp_model_adam_step, bit for bit (tests/test_gpu_model.py: test_sharded_adam_step_equals_the_full_step)."""
    spec, X, Y, zs = _case("ch_res")
    res = []
    for sharded in (False, True):
        model = build_from_spec(copy.deepcopy(spec), X, Y)
        model.set_trainable(0, "q_mu", False)
        for t in (1, 2):
            model.compute_gradients(X, Y, zs=ss.make_noise(spec, X.shape[0], seed=50 + t), fetch=False)
            if sharded:
                model.debug_sharded_adam(3, 0.05, t)
            else:
                model.adam_step(0.05, t)
        res.append(_values(model) + [("elbo", np.array(model.compute_log_likelihood(X, Y, zs=zs)))])
        model.close()
    start = dict((p.pathname, np.array(p.value)) for p in build_from_spec(copy.deepcopy(spec), X, Y).parameters)
    for (name, a), (_, b) in zip(*res):
        assert np.array_equal(a, b), name
    assert not np.array_equal(dict(res[0])["DGP/layers/1/mean_function/conv_filter"], start["DGP/layers/1/mean_function/conv_filter"])


def test_sync_parameters_pushes_the_filter_and_keeps_the_chain(ctx):
    """A filter changed on the Python side reaches the device through sync_parameters; dcgp_model_set_param("mean_filter") alone starts no new
    parameter version: an evaluation behind it reuses the factorisation chain."""
    spec, X, Y, zs = _case("even_s2")
    model = build_from_spec(copy.deepcopy(spec), X, Y)
    p0 = model.predict_proba(X, 2, zs=zs)
    W = np.array(model.layers[0].filter_mean.conv_filter)
    model.layers[0].filter_mean.conv_filter = 0.5 * W
    skips = model.chain_skips
    Wp = np.ascontiguousarray(0.5 * W)
    model._ctx._check(dev.lib().dcgp_model_set_param(model._model, 0, b"mean_filter", Wp.ctypes.data, Wp.size))
    p1 = model.predict_proba(X, 2, zs=zs)
    assert model.chain_skips == skips + 1 and not np.array_equal(p0, p1)
    half = copy.deepcopy(spec)
    half["convs"][0]["mean_filter"] = 0.5 * W
    other = build_from_spec(half, X, Y)
    assert np.array_equal(other.predict_proba(X, 2, zs=zs), p1)
    model.layers[0].filter_mean.conv_filter = W
    model.sync_parameters()
    assert np.array_equal(model.predict_proba(X, 2, zs=zs), p0)
    model.close(), other.close()


# ---- 6. head riding -------------------------------------------------------------------------------------------------------------------
def _rode(ctx):
    out = (C.c_longlong * 2)()
    assert dev.lib().dcgp_debug_head_ride(ctx.handle, out) == 0
    return out[0], out[1]


def test_a_layer_with_a_filter_mean_carries_no_head_rows(ctx):
    """The smallest case of tests/test_gpu_head_ride.py in which rows ride (28 x 28 x 1, conv f5 s2 R10, head f5, M = 32, N = 2, S = 2, its
    options): with Conv2dMean the layer launch carries the head's rows, with LinearConv2dMean("centre0") none, and the two agree."""
    import test_gpu_head_ride as hr
    M, N, S = 32, 2, 2
    spec = syn.make_spec(hr.HWC, [hr.CONV], hr.HEAD, M=M, S=S, num_data=500, seed=31 + M, conv_q_sqrt_scale=0.3)
    X, Y = syn.make_batch(hr.HWC, N, seed=200 + N)
    zs = syn.make_noise(spec, N, seed=9)
    with ctx.options(fused_shape=0, fused_persist=1, fused_wgs=3, head_ride=1000):
        b = build_from_spec(R.without_filters(spec, mean_function="conv2d"), X, Y)
        n0 = _rode(ctx)[1]
        pb = b.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
        rode = _rode(ctx)
        print("Conv2dMean: %d rows rode, %r" % (rode[0], pb))
        assert rode == (N * S, n0 + 1), rode
        a = build_from_spec(R.add_filters(copy.deepcopy(spec), "centre0"), X, Y)
        pa = a.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
        print("LinearConv2dMean(centre0): %r rows rode, %r" % (_rode(ctx), pa))
        assert _rode(ctx) == (0, n0 + 1), _rode(ctx)
    for g, w in zip(pa, pb):
        assert abs(g - w) <= RTOL * max(abs(w), 1.0), (pa, pb)
    a.close(), b.close()


# ---- 7. evaluation, full covariance ---------------------------------------------------------------------------------------------------
def test_evaluate_and_predict_y(ctx):
    N, S, bs = 7, 2, 3
    spec, _, _, _ = _case("ch_res")
    X, Y = syn.make_batch(R.CASES["ch_res"]["hwc"], N, seed=23)
    zs = ss.make_noise(spec, N, seed=23)
    ref, _ = R.oracle_model(spec, X, Y)
    model = build_from_spec(spec, X, Y)
    want, om = oracle_log_density(ref, X, Y, S, zs)
    r = model.evaluate(X, Y, S=S, batch_size=bs, zs=zs, per_image=True)
    p, _ = model.predict_y(X, S, zs=zs)
    print("evaluate: log density %.3e  p_mean %.3e  predict_y %.3e" % (rel(r["log_density"], want), rel(r["p_mean"], om.mean(axis=0)), rel(p, om)))
    assert rel(r["log_density"], want) < RTOL_EVAL and rel(r["p_mean"], om.mean(axis=0)) < RTOL_EVAL and rel(p, om) < RTOL_EVAL
    assert r["accuracy"] == np.mean(om.mean(axis=0).argmax(axis=1) == Y)
    u = model.evaluate_uncertainty(X, Y, S=S, batch_size=bs, zs=zs, per_image=True)
    assert np.array_equal(u["log_density"], r["log_density"]) and np.array_equal(u["p_mean"], r["p_mean"])
    from deepcgp_amd import augment
    views = augment.views(1, True)
    t = model.evaluate(X, Y, S=S, batch_size=bs, seed=3, views=views)
    assert np.isfinite(t["mean_log_density"]) and 0.0 <= t["accuracy"] <= 1.0
    model.close()


def test_full_cov_path_adds_the_mean_through_call(ctx):
    """The layer-level path (``LinearConv2dMean.__call__`` on the padded image): layer 0's full-covariance mean is the model path's for every
    image, and on ONE image (a 1 x 1 covariance: the same samples) ``predict_f_full_cov``'s mean is ``predict_f``'s."""
    spec, X, Y, zs = _case("ch_res")
    model = build_from_spec(spec, X, Y)
    S = spec["S"]
    _, Fm, _ = model.propagate(X, S=S, zs=zs)
    _, Fm_fc, _ = model.propagate(X, full_cov=True, S=S, zs=zs)
    print("layer 0 mean, full_cov vs model path: %.3e" % rel(Fm_fc[0], Fm[0]))
    assert rel(Fm_fc[0], Fm[0]) < RTOL
    z1 = [z[:, :1] for z in zs]
    fm, fv = model.predict_f_full_cov(X[:1], S, zs=z1)
    m, v = model.predict_f(X[:1], S, zs=z1)
    print("predict_f_full_cov vs predict_f on one image: mean %.3e var %.3e" % (rel(fm, m), rel(fv[:, :, 0, :], v)))
    assert fm.shape == (S, 1, 10) and rel(fm, m) < RTOL and rel(fv[:, :, 0, :], v) < RTOL
    mean, _ = model.layers[0].conditional_ND(X)
    assert rel(mean, Fm[0][0]) < RTOL_OPS
    model.close()


# ---- 8. checkpoint round trip, flags -------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_through_load_model(ctx, tmp_path):
    """ModelBuilder with --mean-filter channels --train-mean, three Adam steps, save_model_parameters, ModelBuilder with --load-model: the same
    ELBO bit for bit at a fixed seed, and the key is in the file.  (--white: the reference's checkpoint holds no frozen prior patches Z0, so
    an unwhitened model's KL term restarts from the trained Z when it is loaded; the whitened prior N(0, I) has no Z0 in it.)"""
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder, save_model_parameters, train
    rng = np.random.default_rng(0)
    X = rng.standard_normal((40, 10, 10, 1))
    Y = rng.integers(0, 10, (40, 1))
    args = ['--name', 't', '-M', '6,7,8', '--feature-maps', '2,2', '--filter-sizes', '3,3,3', '--strides', '1,1,1', '--paddings', '1,1,0',
            '--num-samples', '2', '--batch-size', '8', '--white', '--identity-mean', '--mean-filter', 'channels', '--train-mean']
    np.random.seed(0)
    model = ModelBuilder(default_parser().parse_args(args), X, Y).build()
    assert all(l.filter_mean is not None and l.filter_mean.trainable for l in model.layers[:-1])
    hist = train(model, 3, lr=0.01)
    assert len(hist) == 3 and np.all(np.isfinite(hist))
    W = [np.array(l.filter_mean.conv_filter) for l in model.layers[:-1]]
    from deepcgp_amd.mean_functions import conv_mean_filter
    assert all(not np.array_equal(w, conv_mean_filter("channels", *w.shape[1:])) for w in W)          # trained: no longer the named filter
    path = str(tmp_path / "ckpt.npy")
    saved = save_model_parameters(model, path, global_step=3)
    assert np.array_equal(saved["DGP/layers/1/mean_function/conv_filter"], W[1])
    Xb, Yb = X[:8].reshape(8, -1), Y[:8].reshape(-1)
    e = model.compute_log_likelihood(Xb, Yb, seed=5)
    np.random.seed(1)
    builder = ModelBuilder(default_parser().parse_args(args + ['--load-model', 'ckpt']), X, Y, model_path=path)
    again = builder.build()
    assert builder.global_step == 3
    for l, w in zip(again.layers[:-1], W):
        assert np.array_equal(l.filter_mean.conv_filter, w)
    e2 = again.compute_log_likelihood(Xb, Yb, seed=5)
    print("ELBO %.12f, after the round trip %.12f" % (e, e2))
    assert e == e2
    assert np.array_equal(again.predict_proba(Xb, 2, seed=5), model.predict_proba(Xb, 2, seed=5))
    model.close(), again.close()


def test_refusals(ctx):
    """dcgp_model_set_mean_filter on the head, on an identity_mean layer, after the first gradient step; "mean_filter" on a layer without one."""
    L = dev.lib()
    spec, X, Y, zs = _case("even_s2")

    def refused(rc, word):
        assert rc == dev.ERR_ARG, rc
        with pytest.raises(dev.DcgpError, match=word):
            ctx._check(rc)
    plain = build_from_spec(R.without_filters(spec), X, Y)
    plain._build()
    W = np.ascontiguousarray(spec["convs"][0]["mean_filter"])
    buf = np.empty_like(W)
    refused(L.dcgp_model_set_mean_filter(plain._model, 1, W.ctypes.data, 0), "head")
    refused(L.dcgp_model_set_mean_filter(plain._model, 5, W.ctypes.data, 0), "no layer")
    refused(L.dcgp_model_set_param(plain._model, 0, b"mean_filter", W.ctypes.data, W.size), "no mean filter")
    refused(L.dcgp_model_get_param(plain._model, 0, b"mean_filter", buf.ctypes.data, buf.size), "no mean filter")
    refused(L.dcgp_model_set_trainable(plain._model, 0, b"mean_filter", 1), "no mean filter")
    e0 = plain.compute_log_likelihood(X, Y, zs=zs)
    ctx._check(L.dcgp_model_set_mean_filter(plain._model, 0, W.ctypes.data, 1))              # before the first gradient step: allowed
    with_f = build_from_spec(spec, X, Y)
    assert plain.compute_log_likelihood(X, Y, zs=zs) == with_f.compute_log_likelihood(X, Y, zs=zs) != e0
    ctx._check(L.dcgp_model_get_param(plain._model, 0, b"mean_filter", buf.ctypes.data, buf.size))
    assert np.array_equal(buf, W)
    refused(L.dcgp_model_set_param(plain._model, 0, b"mean_filter", W.ctypes.data, W.size - 1), "expected")
    late = build_from_spec(R.without_filters(spec), X, Y)
    late.compute_gradients(X, Y, zs=zs, fetch=False)
    refused(L.dcgp_model_set_mean_filter(late._model, 0, W.ctypes.data, 0), "before the first")
    idm = build_from_spec(R.without_filters(_case("ch_res")[0], mean_function="conv2d"), *_case("ch_res")[1:3])
    idm._build()
    W0 = np.ascontiguousarray(_case("ch_res")[0]["convs"][0]["mean_filter"])
    refused(L.dcgp_model_set_mean_filter(idm._model, 0, W0.ctypes.data, 0), "identity_mean")
    for m in (plain, with_f, late, idm):
        m.close()

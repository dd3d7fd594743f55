"""Feature combinations on the device against ONE composed torch reference (tests/compose_ref.py): every case of tests/compose_cases.py's
covering table -- stack x likelihood x base kernel x mean function x whitening, every pair of levels in at least one case -- under both
``dedup_layer0`` settings.  The reference and the liveness of its gradients are checked without a GPU in tests/test_host_compose.py.

No tolerance is this file's own.  Per case and dedup setting:

    ELBO, data term, KL                          RTOL of tests/test_gpu_model.py (1e-9); a second step (the other bank): the same bits
    gradient of every group, entry by entry,     TOL_GROUP / TOL_E of tests/test_gpu_grad_m256.py (1e-7 / 5.3e-6), of
    likelihood parameter and mean_filter too     tests/test_gpu_grad_large_m.py where a layer has M > 256 (test_gpu_conv_mean.grad_bounds)
    predict_y, predict_density, evaluate         RTOL of tests/test_gpu_evaluate.py (1e-9); evaluate with batch_size = 2: N = 3 splits 2 + 1
    input_gradient(objective="elbo")             |dX - autograd|max <= 1e-7 * max(1, |autograd|max) (tests/test_gpu_input_grad.py); J: RTOL
    two train_step calls against one train_run   ELBOs, every parameter, and through one more identical step the Adam moments: bit for bit
    of two steps                                 (tests/test_gpu_train_run.py)

Every figure is printed before it is asserted (run with -s; lines that start with COMPOSE).  The pairs of ``compose_cases.EXCLUDED`` must
raise their refusal here, from the device model's first call.  One named case beyond the table -- a Gaussian likelihood with trainable
variance AND trainable mean filters on ch_res -- covers the layout of a layer's parameter block: the sharded Adam step cuts it as three
ranks would and must land on adam_step's parameters bit for bit, and ``set_trainable`` must freeze either of the two while the other moves.

Largest figure seen per quantity on an MI355X, over the 56 cases x 2 dedup settings, with the combination that came closest to its bound:

    quantity                              largest     bound     closest combination
    ELBO                                  2.6e-14     1e-9      ch_72_264-poisson1-acos-conv2d-none (tiled)
    data term                             2.6e-14     1e-9      ch_72_264-poisson1-acos-conv2d-none (tiled)
    KL                                    8.8e-13     1e-9      even_s2-gaussian1-matern32-filter-alternate (tiled)
    gradient, group-wise                  5.3e-11     1e-7      wide_R-multiclass3-matern52-none-all (tiled), layer 1 variance
    gradient, entry-wise, M <= 256        1.6e-9      5.3e-6    small3_20_40_24-studentt3-rbf-none-alternate (tiled), layer 2 Z
    gradient, entry-wise, a layer M > 256 4.0e-7      7.6e-6    ch_72_264-softmax3-rbf-none-alternate (tiled), layer 1 q_sqrt
    predict_y mean / variance             2.6e-12 / 3.7e-13  1e-9   ch_72_264-gaussian1-matern32-none-alternate / ch_72_264-poisson1-acos-conv2d-none
    predict_density                       5.0e-14     1e-9      even_s2-multiclass3-rbf-filter-none (tiled)
    evaluate: log density / mean / rmse   5.0e-14 / 1.3e-12 / 3.1e-14  1e-9   even_s2-multiclass3 / ch_72_264-gaussian1 (y_mean) / ch_72_264-poisson1
    input gradient (absolute)             8.2e-14     1e-7 * max(1, 0.126)   even_s2-multiclass3-rbf-filter-none (dedup); J 5.1e-14 (1e-9)
    train_step x 2 against train_run      bit for bit in all 112 runs; second ELBO step, sharded Adam: bit for bit

The closest any quantity came to its bound is the entry-wise gradient at M > 256: 5 % of TOL_E.  No combination failed and the library was
not changed; the two excluded pairs raised their refusal.
"""
import copy
import functools

import numpy as np
import pytest

from deepcgp_amd import device as dev
from deepcgp_amd.models import build_from_spec
import compose_cases as cc
import compose_ref as cr
import live_specs as ls
import stack_specs as ss
from test_gpu_conv_mean import INPUT_GRAD_TOL, grad_bounds
from test_gpu_evaluate import RTOL as RTOL_EVAL
from test_gpu_model import RTOL

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]   # a hung launch ends the run instead of holding the device

DEDUP = pytest.mark.parametrize("dedup", [False, True], ids=["tiled", "dedup"])
CASE = pytest.mark.parametrize("cid", cc.IDS)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def figure(what, value, bound, tag):
    print("COMPOSE %-22s %.3e  bound %.1e  share %.3e  %s" % (what, value, bound, value / bound, tag))


@functools.lru_cache(maxsize=None)
def _case(cid):
    """(spec, X, Y, zs, likelihood tuple, reference) of a case, once per process; never written to."""
    pytest.importorskip("torch")
    spec, X, Y, zs, lik = cc.make_case(cc.BY_ID[cid])
    return spec, X, Y, zs, lik, cr.reference(spec, X, Y, zs, lik)


def _model(spec, X, Y, lik, dedup):
    model = build_from_spec(copy.deepcopy(spec), X.copy(), Y.copy(), likelihood=cr.make_likelihood(lik))
    model.dedup_layer0 = dedup
    return model


# ---- 1. ELBO and gradient -------------------------------------------------------------------------------------------------------------
@DEDUP
@CASE
def test_elbo_and_every_gradient_group(ctx, cid, dedup):
    spec, X, Y, zs, lik, ref = _case(cid)
    tag = cid + ("-dedup" if dedup else "-tiled")
    tol_group, tol_e = grad_bounds(spec)
    ls.assert_live(tag, ref["want"])
    model = _model(spec, X, Y, lik, dedup)
    got = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    e, data, kl = ref["parts"]
    errs = (abs(got[0] - e) / abs(e), abs(got[1] - data) / abs(data), abs(got[2] - kl) / max(abs(kl), 1.0))
    for what, err in zip(("elbo", "data term", "kl"), errs):
        figure(what, err, RTOL, tag)
    again = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    ge, grads = model.compute_gradients(X, Y, zs=zs)
    rows = []
    for li, groups in enumerate(ref["want"]):
        assert set(groups) == set(grads[li]), (tag, li, sorted(groups), sorted(grads[li]))
        for gname, w in groups.items():
            g = np.asarray(grads[li][gname], np.float64)
            assert g.shape == np.shape(w), (tag, li, gname, g.shape, np.shape(w))
            rows.append((li, gname) + ls.errors(gname, g, w))
            print("%s L%d %-20s group %.3e  entry %.3e  |want|max %.3e" % ((tag,) + rows[-1] + (np.abs(w).max(),)))
    worst_g, worst_e = max(rows, key=lambda r: r[2]), max(rows, key=lambda r: r[3])
    figure("gradient group-wise", worst_g[2], tol_group, "%s L%d %s" % (tag, worst_g[0], worst_g[1]))
    figure("gradient entry-wise", worst_e[3], tol_e, "%s L%d %s" % (tag, worst_e[0], worst_e[1]))
    figure("elbo of the grad step", abs(ge - e) / abs(e), RTOL, tag)
    assert max(errs) <= RTOL, (tag, got, ref["parts"])
    assert again == got, (tag, "second step", again, got)
    assert abs(ge - e) <= RTOL * abs(e), (tag, ge, e)
    for li, gname, err_g, err_e in rows:
        assert err_g <= tol_group, (tag, li, gname, "group-wise", err_g)
        assert err_e <= tol_e, (tag, li, gname, "entry-wise", err_e)
    model.close()


# ---- 2. predictions and evaluation ------------------------------------------------------------------------------------------------------
@DEDUP
@CASE
def test_predictions_and_evaluate(ctx, cid, dedup):
    spec, X, Y, zs, lik, ref = _case(cid)
    tag = cid + ("-dedup" if dedup else "-tiled")
    S, N = spec["S"], X.shape[0]
    model = _model(spec, X, Y, lik, dedup)
    pm, pv = model.predict_y(X, S, zs=zs)
    ld = model.predict_density(X, Y, S, zs=zs)
    r = model.evaluate(X, Y, S=S, batch_size=2, zs=zs, per_image=True)
    mean_key = "y_mean" if lik[0] in ("gaussian", "studentt", "poisson") else "p_mean"
    want_ld = ref["density"]
    rows = [("predict_y mean", rel(pm, ref["py_mean"])), ("predict_y var", rel(pv, ref["py_var"])), ("predict_density", rel(ld, want_ld)),
            ("evaluate log density", rel(r["log_density"], want_ld.sum(1))), ("evaluate " + mean_key, rel(r[mean_key], ref["py_mean"].mean(0))),
            ("evaluate mean ld", abs(r["mean_log_density"] - want_ld.sum(1).mean()) / abs(want_ld.sum(1).mean()))]
    if "rmse" in r:
        want = np.sqrt(np.mean(np.square(ref["py_mean"].mean(0) - Y)))
        rows.append(("evaluate rmse", abs(r["rmse"] - want) / want))
    for what, err in rows:
        figure(what, err, RTOL_EVAL, tag)
    assert pm.shape == ref["py_mean"].shape and ld.shape == want_ld.shape and r["n"] == N
    for what, err in rows:
        assert err < RTOL_EVAL, (tag, what, err)
    if "accuracy" in r:
        p = ref["py_mean"].mean(0)
        want = np.mean((p > 0.5) == (Y == 1)) if lik[0] == "bernoulli" else np.mean(p.argmax(1) == Y)
        assert r["accuracy"] == want, (tag, r["accuracy"], want)
    model.close()


# ---- 3. input gradient ------------------------------------------------------------------------------------------------------------------
@DEDUP
@CASE
def test_input_gradient_of_the_elbo_objective(ctx, cid, dedup):
    spec, X, Y, zs, lik, ref = _case(cid)
    tag = cid + ("-dedup" if dedup else "-tiled")
    model = _model(spec, X, Y, lik, dedup)
    J, got = model.input_gradient(X, Y, objective="elbo", zs=zs)
    want = ref["dX"]
    bound = INPUT_GRAD_TOL * max(1.0, np.abs(want).max())
    err = np.abs(got - want).max()
    figure("input gradient", err, bound, "%s |want|max %.3e" % (tag, np.abs(want).max()))
    figure("input gradient J", rel(J, ref["J"]), RTOL, tag)
    assert got.shape == X.shape == want.shape and J.shape == (X.shape[0],)
    assert np.abs(want).max() > 0
    assert rel(J, ref["J"]) <= RTOL
    assert err <= bound, (tag, err, np.abs(want).max())
    model.close()


# ---- 4. training ------------------------------------------------------------------------------------------------------------------------
def _values(model):
    model.pull_parameters()
    return [(p.pathname, np.array(p.value)) for p in model.parameters]


def _assert_same(a, b, what):
    assert [n for n, _ in a] == [n for n, _ in b]
    for (name, va), (_, vb) in zip(a, b):
        assert np.array_equal(va, vb), (what, name, float(np.max(np.abs(va - vb))))


@DEDUP
@CASE
def test_two_train_steps_equal_a_train_run_of_two(ctx, cid, dedup):
    """The scheme of tests/test_gpu_train_run.py on a pool of five images, batches of three: ELBOs and every parameter to the bit, and one more
    identical step on both models -- its result depends on both moment buffers and on the step count of the bias correction."""
    spec, X, Y, _, lik = cc.make_case(cc.BY_ID[cid], n=5)
    tag = cid + ("-dedup" if dedup else "-tiled")
    a, b = _model(spec, X, Y, lik, dedup), _model(spec, X, Y, lik, dedup)
    idx = np.array([[0, 4, 2], [3, 1, 4]])
    lrs = np.array([0.01, 0.001])
    start = _values(a)
    ha = np.array([a.train_step(a.X[idx[i]], a.Y[idx[i]], lrs[i], seed=11 + i) for i in range(2)])
    b.attach_dataset()
    hb = b.train_run(idx, lrs, seed=11)
    print("%s loop %s run %s" % (tag, ha, hb))
    assert np.all(np.isfinite(ha)) and np.array_equal(ha, hb), (tag, ha, hb)
    va = _values(a)
    _assert_same(va, _values(b), tag + " after the run")
    ea = a.train_step(a.X[idx[1]], a.Y[idx[1]], 0.004, seed=77)
    eb = b.train_step(b.X[idx[1]], b.Y[idx[1]], 0.004, seed=77)
    assert ea == eb, (tag, ea, eb)
    _assert_same(_values(a), _values(b), tag + " one step after the run")
    moved = [n for (n, v0), (_, v1) in zip(start, va) if not np.array_equal(v0, v1)]
    still = sorted(set(n for n, _ in start) - set(moved))
    assert all(n.endswith("invlink/epsilon") for n in still), (tag, still)          # (RobustMax epsilon is no trainable value)
    b.detach_dataset()
    a.close(), b.close()


# ---- 5. the excluded pairs are refused -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", cc.EXCLUDED, ids=lambda p: "%s-%s" % (p[0][1], p[1][1]))
def test_an_excluded_pair_raises_its_refusal(ctx, pair):
    a, b, text = pair
    case = dict(stack="ch_res", likelihood="multiclass3", base="rbf", mean="none", white="none")
    case.update([a, b])
    spec, X, Y, zs, lik = cc.make_case(case)
    model = _model(spec, X, Y, lik, False)
    with pytest.raises(dev.DcgpError, match=text):
        model.compute_log_likelihood(X, Y, zs=zs)


# ---- 6. the parameter block: a Gaussian variance slot and trainable filters together --------------------------------------------------------
BLOCK_CASE = dict(stack="ch_res", likelihood="gaussian3", base="rbf", mean="filter", white="none")
VARIANCE = "DGP/likelihood/likelihood/variance"
FILTERS = ["DGP/layers/%d/mean_function/conv_filter" % li for li in (0, 1)]


def test_sharded_adam_equals_adam_step_with_variance_slot_and_filters(ctx):
    """dcgp_model_debug_sharded_adam(ranks = 3) cuts every layer's block -- the filters' slots at the conv layers' ends, the variance slot at the
    head's -- and lands on dcgp_model_adam_step's parameters bit for bit; both kinds of slot have moved."""
    spec, X, Y, zs, lik = cc.make_case(BLOCK_CASE)
    start = dict(_values(_model(spec, X, Y, lik, False)))
    res = []
    for sharded in (False, True):
        model = _model(spec, X, Y, lik, False)
        for t in (1, 2):
            model.compute_gradients(X, Y, zs=ss.make_noise(spec, X.shape[0], seed=50 + t), fetch=False)
            if sharded:
                model.debug_sharded_adam(3, 0.05, t)
            else:
                model.adam_step(0.05, t)
        res.append(_values(model) + [("elbo", np.array(model.compute_log_likelihood(X, Y, zs=zs)))])
        model.close()
    _assert_same(res[0], res[1], "sharded against full")
    end = dict(res[0])
    assert set(FILTERS + [VARIANCE]) <= set(end)
    for name in FILTERS + [VARIANCE]:
        print("%s moved by %.3e" % (name, np.abs(end[name] - start[name]).max()))
        assert not np.array_equal(end[name], start[name]), name


def test_set_trainable_freezes_the_variance_and_the_filters_independently(ctx):
    spec, X, Y, zs, lik = cc.make_case(BLOCK_CASE)
    model = _model(spec, X, Y, lik, True)
    v0 = dict(_values(model))
    model.set_trainable(0, "likelihood_variance", False)
    model.train_step(X, Y, 0.01, zs=zs)
    v1 = dict(_values(model))
    assert np.array_equal(v1[VARIANCE], v0[VARIANCE])
    assert all(not np.array_equal(v1[n], v0[n]) for n in FILTERS)
    model.set_trainable(0, "likelihood_variance", True)
    for li in (0, 1):
        model.set_trainable(li, "mean_filter", False)
    model.train_step(X, Y, 0.01, zs=zs)
    v2 = dict(_values(model))
    assert not np.array_equal(v2[VARIANCE], v1[VARIANCE])
    assert all(np.array_equal(v2[n], v1[n]) for n in FILTERS)
    assert not np.array_equal(v2["DGP/layers/0/q_mu"], v1["DGP/layers/0/q_mu"])
    model.set_trainable(1, "mean_filter", True)                                   # one filter back on, the other stays
    model.train_step(X, Y, 0.01, zs=zs)
    v3 = dict(_values(model))
    assert np.array_equal(v3[FILTERS[0]], v2[FILTERS[0]]) and not np.array_equal(v3[FILTERS[1]], v2[FILTERS[1]])
    assert not np.array_equal(v3[VARIANCE], v2[VARIANCE])
    model.close()

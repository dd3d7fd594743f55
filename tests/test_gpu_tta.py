"""GPU: test-time augmentation -- ``evaluate`` / ``evaluate_uncertainty`` / ``predict_density`` / ``predict_uncertainty`` with ``views=``
(dcgp_model_set_eval_views, the view gather of csrc/augment.hip inside eval_batches) and the stand-alone gather dcgp_view_images.

With V views a batch of n images is evaluated as V n images, view v of image i at row v n + i, and the head's rows [S][V n][K] are S V samples
of n images to the unchanged tails: member (s, v) of image i is sample s of the forward pass on row v n + i, in the order s outer, v inner.  The
references here are built exactly so: the NumPy mirror ``augment.apply_views`` makes X', the oracle or the device's own ``predict_y`` gives the
per-sample predictions on X', and ``_members`` regroups them to [S V, n, K].

Models are those of tests/test_gpu_evaluate.py (``small_model``: 28 x 28 x 1, one conv layer, M = 32), tests/test_gpu_augment.py (a patch head
alone) and tests/padding_ref.py (a padded first layer), Gaussian / Bernoulli / Softmax those of their own GPU tests."""
import ctypes as C
import csv
import os

import numpy as np
import pytest

import bernoulli_ref as br
import stack_specs as ss
import uncertainty_ref as ur
from deepcgp_amd import augment
from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.likelihoods import Bernoulli, Gaussian, Softmax
from deepcgp_amd.models import TTAAccuracyLogger, TestLogDensityLogger, UncertaintyLogger, build_from_spec
from oracle_build import oracle_model

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]   # a hung launch ends the run instead of holding the device

RTOL = 1e-9            # tests/test_gpu_evaluate.py's bound against the oracle
ATOL_SAMPLES = 1e-12   # tests/test_gpu_uncertainty.py's bound for the entropies against the device's own samples
LOG2PI = np.log(2 * np.pi)
VIEWS3 = np.array([(0, 0, 0), (-2, 3, 1), (1, 0, 0)], np.int32)         # the identity, a flip with a negative shift, a plain shift
PER_IMAGE = ("predictive_entropy", "expected_entropy", "mutual_information", "confidence", "prediction")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def _views_of(X, hwc, views):
    """X [n, H W C] -> X' [V n, H W C], view-major (the mirror)."""
    n = X.shape[0]
    return augment.apply_views(X.reshape((n,) + tuple(hwc)), views).reshape(len(views) * n, -1)


def _members(p, V):
    """[S, V n, K] per-sample predictions on X' -> [S V, n, K], member s V + v = sample s on view v."""
    S, Vn, K = p.shape
    return p.reshape(S * V, Vn // V, K)


def _seq_mean(members):
    """The tail's sum: members in order, a sequential float64 sum, then one division."""
    acc = np.zeros(members.shape[1:])
    for m in members:
        acc = acc + m
    return acc / members.shape[0]


def _lse_mean(l):
    """log mean_m exp(l[m]) over axis 0."""
    mx = l.max(axis=0)
    return mx + np.log(np.exp(l - mx).sum(axis=0)) - np.log(l.shape[0])


def small_spec(S=2, seed=5, white=False):
    """tests/test_gpu_evaluate.py's small_model, with the whitening as an argument."""
    hwc = (28, 28, 1)
    return hwc, syn.make_spec(hwc, [(5, 2, 10)], (5, 1), 32, S=S, num_data=1000, seed=seed, white=white, conv_q_sqrt_scale=0.2)


def head_only_spec(S=2):
    hwc = (12, 12, 1)
    return hwc, syn.make_spec(hwc, [], (3, 1), 24, S=S, num_data=500, seed=5)


def padded_spec(S=2):
    """--paddings 1,0: the first layer pads its 10 x 10 x 1 input by 1, the head does not."""
    hwc = (10, 10, 1)
    return hwc, ss.stack_spec(hwc=hwc, convs=[(3, 1, 2, 1, 1)], head=(3, 1, 0), Ms=12, S=S)


# ---- 1: the gather -----------------------------------------------------------------------------------------------------------------------
GATHER = {
    "9x7x3": ((9, 7, 3), [(0, 0, 0), (-2, 3, 1), (8, 0, 0), (0, -6, 1)]),           # W C = 21; the extreme shifts leave one row / one column
    "5x13x1": ((5, 13, 1), [(0, 0, 0), (4, -1, 1), (-4, 4, 0), (0, 0, 1)]),          # W C = 13
    "28x28x1": ((28, 28, 1), None),                                                  # the cross pattern at t = 2 with the flip: 10 views
    "6x23x3": ((6, 23, 3), [(0, 0, 0), (1, -5, 1), (-5, 2, 0)]),                     # W C = 69: past one wave's 64 lanes, no multiple of 64
    "4x32x4": ((4, 32, 4), [(0, 0, 1), (3, 3, 1), (0, -3, 0)]),                      # W C = 128: a multiple of 64
}


@pytest.mark.parametrize("name", list(GATHER))
def test_view_gather_is_the_mirror(ctx, name):
    (H, W, Cc), v = GATHER[name]
    v = augment.views(2, True) if v is None else np.array(v, np.int32)
    L = dev.lib()
    rng = np.random.default_rng(H * 100 + W)
    for N in (1, 5):
        X = rng.standard_normal((N, H, W, Cc))
        want = augment.apply_views(X, v)
        dX = ctx.to_device(X)
        out = ctx.to_device(np.full((len(v) * N, H, W, Cc), np.nan))              # an unwritten value would show
        ctx._check(L.dcgp_view_images(ctx.handle, dX.ptr, N, H, W, Cc, len(v), v.ctypes.data, out.ptr))
        got = out.numpy()
        assert not np.isnan(got).any(), (name, N)
        assert np.array_equal(got, want), (name, N)
        assert np.array_equal(dX.numpy(), X)                                       # the source is read only
    # refused before any launch
    out = ctx.empty((len(v) * 5, H, W, Cc))
    assert L.dcgp_view_images(ctx.handle, dX.ptr, 5, H, W, Cc, len(v), v.ctypes.data, dX.ptr) == dev.ERR_ARG       # out aliases X
    for bad in ((H, 0, 0), (-H, 0, 1), (0, W, 0), (0, -W, 0), (0, 0, 2)):         # a shift that leaves no pixel, a flip of 2
        b = np.array([(0, 0, 0), bad], np.int32)
        assert L.dcgp_view_images(ctx.handle, dX.ptr, 5, H, W, Cc, 2, b.ctypes.data, out.ptr) == dev.ERR_ARG
    assert L.dcgp_view_images(ctx.handle, dX.ptr, 5, H, W, Cc, 0, v.ctypes.data, out.ptr) == dev.ERR_ARG


# ---- 2: against the oracle, explicit noise -----------------------------------------------------------------------------------------------
ORACLE_N, ORACLE_S, ORACLE_SEED = 7, 2, 1      # seed 1: the oracle's smallest arg-max gap is 2.4e-3 (0.58 whitened), checked on the CPU
Q_MU_SCALE = 300.0


def oracle_case(white):
    hwc, spec = small_spec(S=ORACLE_S, seed=ORACLE_SEED, white=white)
    # tests/test_gpu_uncertainty.py's scale: the synthetic parameters alone predict every class at 0.1 (whitened: to the last bit, a tie)
    spec["head"]["q_mu"] = spec["head"]["q_mu"] * Q_MU_SCALE
    if white:      # make_spec's whitened q_sqrt = I samples the conv layer at its prior's scale, far from the head's inducing patches
        spec["convs"][0]["q_sqrt"] = spec["convs"][0]["q_sqrt"] * 0.05
        spec["convs"][0]["q_mu"] = spec["convs"][0]["q_mu"] * 0.3
    X, Y = syn.make_batch(hwc, ORACLE_N, seed=ORACLE_SEED)
    V = len(VIEWS3)
    zs_flat = syn.make_noise(spec, V * ORACLE_N, seed=3)                                   # [S, V N, D]: the noise of row v N + i of X'
    zs = [z.reshape(ORACLE_S, V, ORACLE_N, -1) for z in zs_flat]                           # [S, V, N, D]: what evaluate(views=...) takes
    Xv = _views_of(X, hwc, VIEWS3)
    om, _ = oracle_model(spec, X, Y).predict_y(Xv, ORACLE_S, zs=zs_flat)                   # [S, V N, K]
    mem = _members(om, V)
    pbar = mem.mean(axis=0)
    logdens = _lse_mean(np.log(mem[:, np.arange(ORACLE_N), Y]))
    return spec, X, Y, zs, pbar, logdens


@pytest.mark.parametrize("white", [False, True])
def test_explicit_noise_vs_oracle_any_batch_size(ctx, white):
    spec, X, Y, zs, pbar, logdens = oracle_case(white)
    top = np.sort(pbar, axis=1)
    gap = (top[:, -1] - top[:, -2]).min()
    print("white=%d: smallest gap between the two largest pbar entries %.3e" % (white, gap))
    assert gap > 1e-6                                                  # the arg-max cannot turn on an error of RTOL
    model = build_from_spec(spec, X, Y)
    runs = {bs: model.evaluate(X, Y, S=ORACLE_S, batch_size=bs, zs=zs, views=VIEWS3, per_image=True) for bs in (3, 1, ORACLE_N)}
    r = runs[3]                                                        # batches of 3, 3 and 1 images
    print("white=%d: log_density rel %.3e, p_mean rel %.3e" % (white, rel(r["log_density"], logdens), rel(r["p_mean"], pbar)))
    assert rel(r["log_density"], logdens) < RTOL
    assert rel(r["p_mean"], pbar) < RTOL
    assert r["accuracy"] == np.mean(pbar.argmax(axis=1) == Y) and r["n"] == ORACLE_N
    assert abs(r["mean_log_density"] - logdens.mean()) < RTOL * abs(logdens.mean())
    for bs in (1, ORACLE_N):
        assert np.max(np.abs(runs[bs]["log_density"] - r["log_density"])) <= 1e-12 * np.max(np.abs(r["log_density"]))
        assert np.max(np.abs(runs[bs]["p_mean"] - r["p_mean"])) <= 1e-12
    # predict_density is the same mixture, in one batch
    ld = model.predict_density(X, Y, ORACLE_S, zs=zs, views=VIEWS3)
    assert ld.shape == (ORACLE_N, 1) and np.array_equal(ld[:, 0], runs[ORACLE_N]["log_density"])
    # the mixture is not the plain evaluation
    plain = model.evaluate(X, Y, S=ORACLE_S, batch_size=3, zs=[z[:, 0] for z in zs], per_image=True)
    assert not np.array_equal(plain["p_mean"], r["p_mean"])
    model.close()


# ---- 3: against the device's own per-sample probabilities, seeded noise ------------------------------------------------------------------
def _own_members(model, X, hwc, views, S, bs, seed):
    """Per batch b the device's predict_y on the mirror's views of the batch under seed + b, regrouped: [S V, N, K] over the whole set."""
    parts = []
    for b, lo in enumerate(range(0, X.shape[0], bs)):
        p = model.predict_y(_views_of(X[lo:lo + bs], hwc, views), S, seed=seed + b)[0]
        parts.append(_members(p, len(views)))
    return np.concatenate(parts, axis=1)


SEEDED = {"conv": small_spec, "head_only": head_only_spec, "padded_1_0": padded_spec}


@pytest.mark.parametrize("dedup", [False, True])
@pytest.mark.parametrize("name", list(SEEDED))
def test_seeded_noise_vs_own_samples(ctx, name, dedup):
    N, S, bs, seed = 7, 2, 3, 11
    hwc, spec = SEEDED[name](S=S)
    X, Y = syn.make_batch(hwc, N, seed=5)
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    mem = _own_members(model, X, hwc, VIEWS3, S, bs, seed)
    assert mem.shape == (S * len(VIEWS3), N, 10)
    want = _seq_mean(mem)
    r = model.evaluate(X, Y, S=S, batch_size=bs, seed=seed, views=VIEWS3, per_image=True)
    assert np.array_equal(r["p_mean"], want)                           # the same probabilities, the same sum order
    assert r["accuracy"] == np.mean(want.argmax(axis=1) == Y)
    ld = _lse_mean(np.log(mem[:, np.arange(N), Y]))
    err = np.max(np.abs(r["log_density"] - ld)) / np.max(np.abs(ld))
    print("%s dedup=%d: log_density vs own samples %.3e" % (name, dedup, err))
    assert err <= 1e-13
    assert TTAAccuracyLogger(X, Y, VIEWS3, batch_size=bs, num_samples=S)(model, seed=seed) == r["accuracy"]
    assert TestLogDensityLogger(X, Y, batch_size=bs, num_samples=S, views=VIEWS3)(model, seed=seed) == r["mean_log_density"]
    model.close()


# ---- 4: identity -------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            for q in a[k]:
                assert np.array_equal(a[k][q], b[k][q], equal_nan=True), (k, q)
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_identity_view_and_flip_alone(ctx):
    N, S, bs, seed = 7, 2, 3, 4
    hwc, spec = small_spec(S=S)
    X, Y = syn.make_batch(hwc, N, seed=5)
    model = build_from_spec(spec, X, Y)
    Xf = np.ascontiguousarray(X.reshape((N,) + hwc)[:, :, ::-1]).reshape(N, -1)
    for views, Xw in (([(0, 0, 0)], X), ([(0, 0, 1)], Xf)):
        kw = dict(S=S, batch_size=bs, seed=seed, per_image=True)
        _same(model.evaluate(X, Y, views=views, **kw), model.evaluate(Xw, Y, **kw))
        _same(model.evaluate_uncertainty(X, Y, views=views, bins=5, **kw), model.evaluate_uncertainty(Xw, Y, bins=5, **kw))
        assert np.array_equal(model.predict_density(X, Y, S, seed=seed, views=views), model.predict_density(Xw, Y, S, seed=seed))
        _same(model.predict_uncertainty(X, S, seed=seed, views=views), model.predict_uncertainty(Xw, S, seed=seed))
    assert not np.array_equal(model.evaluate(X, Y, per_image=True, S=S)["p_mean"], model.evaluate(Xf, Y, per_image=True, S=S)["p_mean"])
    model.close()


# ---- 5: uncertainty ----------------------------------------------------------------------------------------------------------------------
def test_uncertainty_over_samples_and_views(ctx):
    N, S, bs, seed = 7, 2, 3, 11
    hwc, spec = small_spec(S=S)
    spec["head"]["q_mu"] = spec["head"]["q_mu"] * Q_MU_SCALE            # tests/test_gpu_uncertainty.py's scale: the confidences spread
    X, Y = syn.make_batch(hwc, N, seed=5)
    model = build_from_spec(spec, X, Y)
    kw = dict(S=S, batch_size=bs, seed=seed, views=VIEWS3, per_image=True)
    ev = model.evaluate(X, Y, **kw)
    un = model.evaluate_uncertainty(X, Y, bins=5, **kw)
    for k in ("accuracy", "mean_log_density", "n"):
        assert un[k] == ev[k], k
    assert np.array_equal(un["log_density"], ev["log_density"]) and np.array_equal(un["p_mean"], ev["p_mean"])
    want = ur.multiclass(_own_members(model, X, hwc, VIEWS3, S, bs, seed))
    for k in ("predictive_entropy", "expected_entropy", "mutual_information"):
        err = np.max(np.abs(un[k] - want[k]))
        print("%s: max abs error vs own samples %.3e" % (k, err))
        assert err <= ATOL_SAMPLES, (k, err)
    assert np.array_equal(un["confidence"], want["confidence"]) and np.array_equal(un["prediction"], want["prediction"])
    assert abs(un["mean_predictive_entropy"] - want["predictive_entropy"].mean()) <= ATOL_SAMPLES
    assert abs(un["mean_mutual_information"] - want["mutual_information"].mean()) <= ATOL_SAMPLES
    cal = ur.calibration(want["p_mean"], Y, 5)
    assert np.array_equal(un["reliability"]["count"], cal["table"][:, 0].astype(np.int64))
    assert abs(un["ece"] - cal["ece"]) <= ATOL_SAMPLES and abs(un["brier"] - cal["brier"]) <= ATOL_SAMPLES
    # disagreement between views counts: the views' mutual information is not the plain one
    plain = model.evaluate_uncertainty(X, Y, S=S, batch_size=bs, seed=seed, per_image=True)
    assert not np.array_equal(plain["mutual_information"], un["mutual_information"])
    pu = model.predict_uncertainty(X, S, seed=seed, batch_size=bs, views=VIEWS3)
    assert np.array_equal(pu["p_mean"], un["p_mean"])
    for k in PER_IMAGE:
        assert np.array_equal(pu[k], un[k]), k
    assert UncertaintyLogger(X, Y, S=S, bins=5, batch_size=bs, views=VIEWS3)(model, seed=seed)["ece"] == un["ece"]
    model.close()


# ---- 6: float targets, Softmax -------------------------------------------------------------------------------------------------------------
def float_case(N=5, S=2, seed=7, D=3):
    """The "conv" case of tests/test_gpu_gaussian.py / test_gpu_bernoulli.py with the noise of the V N view images."""
    hwc = (10, 10, 1)
    spec = syn.make_spec(hwc, [(3, 1, 2)], (3, 1), 9, S=S, num_data=300, seed=seed, conv_q_sqrt_scale=0.3, variance=2.0, ls=1.5, head_outputs=D)
    X, Ylab = syn.make_batch(hwc, N, seed=seed)
    V = len(VIEWS3)
    zs_flat = syn.make_noise(spec, V * N, seed=seed)
    zs = [z.reshape(S, V, N, -1) for z in zs_flat]
    _, Fm, Fv = oracle_model(spec, X, Ylab).propagate(_views_of(X, hwc, VIEWS3), S=S, zs=zs_flat)
    return spec, X, zs, _members(Fm[-1], V), _members(Fv[-1], V)


# The bound: the Gaussian and Bernoulli GPU tests hold the head's marginals to 1e-9 of the oracle's (test_head_marginals_at_other_widths) and their
# tails to 1e-12 of NumPy on the same marginals; the quantities below are smooth functions of the marginals, so the oracle bound governs.
def test_gaussian_vs_oracle(ctx):
    N, S, D, s2 = 5, 2, 3, 0.45
    spec, X, zs, fm, fv = float_case(N, S, D=D)
    Y = np.random.default_rng(7).standard_normal((N, D))
    model = build_from_spec(spec, X, Y, likelihood=Gaussian(s2))
    r = model.evaluate(X, Y, S=S, batch_size=2, zs=zs, views=VIEWS3, per_image=True)
    ym = fm.mean(axis=0)
    l = -0.5 * (LOG2PI + np.log(fv + s2)) - 0.5 * np.square(Y[None] - fm) / (fv + s2)          # [S V, N, D]
    ld = _lse_mean(l)
    print("gaussian: y_mean rel %.3e, log_density rel %.3e" % (rel(r["y_mean"], ym), rel(r["log_density"], ld.sum(1))))
    assert rel(r["y_mean"], ym) < 1e-9 and rel(r["log_density"], ld.sum(1)) < 1e-9
    rmse = np.sqrt(np.mean(np.square(ym - Y)))
    assert abs(r["rmse"] - rmse) <= 1e-9 * rmse and r["n"] == N
    assert abs(r["mean_log_density"] - ld.sum(1).mean()) <= 1e-9 * abs(ld.sum(1).mean())
    assert rel(model.predict_density(X, Y, S, zs=zs, views=VIEWS3), ld) < 1e-9
    model.close()


def test_bernoulli_vs_oracle(ctx):
    N, S, D = 5, 2, 3
    spec, X, zs, fm, fv = float_case(N, S, D=D)
    Y = (np.random.default_rng(7).random((N, D)) < 0.5).astype(np.float64)
    model = build_from_spec(spec, X, Y, likelihood=Bernoulli())
    r = model.evaluate(X, Y, S=S, batch_size=2, zs=zs, views=VIEWS3, per_image=True)
    p = br.predict_mean_and_var(fm, fv)[0]                                                     # [S V, N, D]
    pm = p.mean(axis=0)
    assert np.abs(pm - 0.5).min() > 1e-6                                                       # no entry's prediction can turn on the bound
    ld = _lse_mean(np.where(Y[None] == 1, np.log(p), np.log(1 - p)))
    print("bernoulli: p_mean rel %.3e, log_density rel %.3e" % (rel(r["p_mean"], pm), rel(r["log_density"], ld.sum(1))))
    assert rel(r["p_mean"], pm) < 1e-9 and rel(r["log_density"], ld.sum(1)) < 1e-9
    assert r["accuracy"] == np.mean((pm > 0.5) == (Y == 1)) and r["n"] == N
    un = model.evaluate_uncertainty(X, Y, S=S, batch_size=2, zs=zs, views=VIEWS3, per_image=True)
    assert np.array_equal(un["p_mean"], r["p_mean"]) and un["accuracy"] == r["accuracy"]
    want = ur.bernoulli(p)
    assert rel(un["predictive_entropy"], want["predictive_entropy"]) < 1e-9 and rel(un["expected_entropy"], want["expected_entropy"]) < 1e-9
    model.close()


def test_softmax_vs_own_samples(ctx):
    N, S, bs, seed = 7, 2, 3, 11
    hwc = (10, 10, 1)
    spec = syn.make_spec(hwc, [(3, 1, 2)], (3, 1), 9, S=S, num_data=300, seed=9, conv_q_sqrt_scale=0.3, variance=2.0, ls=1.5, head_outputs=10)
    X, Y = syn.make_batch(hwc, N, seed=9)
    model = build_from_spec(spec, X, Y, likelihood=Softmax(10, 100, seed=4))
    mem = _own_members(model, X, hwc, VIEWS3, S, bs, seed)
    want = _seq_mean(mem)
    r = model.evaluate(X, Y, S=S, batch_size=bs, seed=seed, views=VIEWS3, per_image=True)
    print("softmax: p_mean max abs difference to own samples %.3e" % np.max(np.abs(r["p_mean"] - want)))
    assert np.array_equal(r["p_mean"], want)
    assert r["accuracy"] == np.mean(want.argmax(axis=1) == Y)
    ld = _lse_mean(np.log(mem[:, np.arange(N), Y]))
    assert np.max(np.abs(r["log_density"] - ld)) <= 1e-13 * np.max(np.abs(ld))
    un = model.evaluate_uncertainty(X, Y, S=S, batch_size=bs, seed=seed, views=VIEWS3, per_image=True)
    assert np.array_equal(un["p_mean"], r["p_mean"]) and np.array_equal(un["log_density"], r["log_density"])
    model.close()


# ---- 7: limits and errors ----------------------------------------------------------------------------------------------------------------
def test_limits_and_errors_leave_nothing_behind(ctx):
    N, S = 6, 2
    hwc, spec = small_spec(S=S)
    X, Y = syn.make_batch(hwc, N, seed=5)
    model = build_from_spec(spec, X, Y)
    kw = dict(S=S, batch_size=4, seed=1, per_image=True)
    good = model.evaluate(X, Y, **kw)
    L = dev.lib()
    v5 = augment.views(1)
    S_eval, S_unc = (8192 - 10) // 50 + 1, (8192 - 10 - 48) // 50 + 1           # the smallest S with S V K + K (+ 48) > 8192 at V = 5, K = 10
    with pytest.raises(ValueError, match="LDS"):
        model.evaluate(X, Y, S=S_eval, views=v5)
    with pytest.raises(ValueError, match="LDS"):
        model.evaluate_uncertainty(X, Y, S=S_unc, views=v5)
    _same(model.evaluate(X, Y, **kw), good)
    # ... and the library's own check, with the views set through the C entry point: nothing is launched, the setting is cleared by hand
    dX, dY = ctx.to_device(X), ctx.to_device(Y, np.int32)
    out, info = (C.c_double * 2)(), C.c_int(0)
    ctx._check(L.dcgp_model_set_eval_views(model._model, 28, 28, 1, 5, v5.ctypes.data))
    assert L.dcgp_model_evaluate(model._model, dX.ptr, dY.ptr, N, 4, S_eval, None, 1, None, None, out, C.byref(info)) == dev.ERR_ARG
    with pytest.raises(dev.DcgpError, match="views"):
        ctx._check(dev.ERR_ARG)
    ctx._check(L.dcgp_model_set_eval_views(model._model, 0, 0, 0, 0, None))
    _same(model.evaluate(X, Y, **kw), good)
    # zs of the wrong shape: [S, N, D] where [S, V, N, D] is due
    with pytest.raises(ValueError, match=r"\[S, V, N, D\]"):
        model.evaluate(X, Y, S=S, batch_size=4, zs=syn.make_noise(spec, N, seed=3), views=v5)
    # bad tables
    for bad, what in (([(28, 0, 0)], "min"), ([(0, -28, 1)], "min"), ([(0, 0, 2)], "flip"), ([(0, 0)], "V, 3"), (np.zeros((0, 3), int), "empty")):
        with pytest.raises(ValueError, match=what):
            model.evaluate(X, Y, S=S, views=bad)
    _same(model.evaluate(X, Y, **kw), good)                                      # the failed calls left no views behind
    # the library itself: another geometry than the model's, a bad shift, a bad flip
    for H, W, Cc in ((28, 14, 2), (14, 28, 2), (27, 28, 1), (28, 28, 2)):
        assert L.dcgp_model_set_eval_views(model._model, H, W, Cc, 5, v5.ctypes.data) == dev.ERR_ARG
    for bad in ((28, 0, 0), (0, -28, 0), (0, 0, 2)):
        b = np.array([(0, 0, 0), bad], np.int32)
        assert L.dcgp_model_set_eval_views(model._model, 28, 28, 1, 2, b.ctypes.data) == dev.ERR_ARG
    # steps enqueued and not yet collected
    ticket = model.enqueue_log_likelihood(X, Y, seed=1)
    assert L.dcgp_model_set_eval_views(model._model, 28, 28, 1, 5, v5.ctypes.data) == dev.ERR_ARG
    with pytest.raises(ValueError, match="collected"):
        model.evaluate(X, Y, S=S, views=v5)
    assert np.isfinite(model.collect_log_likelihood(ticket))
    _same(model.evaluate(X, Y, **kw), good)
    model.close()


def test_dense_head_alone_has_no_views(ctx):
    """--last-kernel rbf without conv layers: feature vectors, no images -- the host says so, and so does the library."""
    import live_specs as ls
    spec = ls.live_spec(hwc=(6, 6, 1), convs=[], head=(3, 1), M=8, c=0.5, a=0.3, head_kernel="rbf")
    X, Y = syn.make_batch((6, 6, 1), 4, seed=5)
    model = build_from_spec(spec, X, Y)
    good = model.evaluate(X, Y, S=2, seed=1, per_image=True)
    with pytest.raises(ValueError, match="dense head"):
        model.evaluate(X, Y, S=2, views=augment.views(1))
    v = augment.views(1)
    assert dev.lib().dcgp_model_set_eval_views(model._model, 6, 6, 1, 5, v.ctypes.data) == dev.ERR_ARG
    _same(model.evaluate(X, Y, S=2, seed=1, per_image=True), good)
    model.close()


# ---- 8: nothing else moves ---------------------------------------------------------------------------------------------------------------
def _values(model):
    model.pull_parameters()
    return [(p.pathname, np.array(p.value)) for p in model.parameters]


def test_only_the_evaluation_consults_the_views(ctx):
    import live_specs as ls
    N, S = 5, 2
    hwc = (12, 12, 1)
    make = lambda: ls.live_spec(S=S, hwc=hwc, convs=[(3, 2, 3)], head=(2, 1), M=12, c=0.5, a=0.3)     # noqa: E731  (every gradient group live)
    X, Y = syn.make_batch(hwc, N, seed=5)
    model, twin = build_from_spec(make(), X, Y), build_from_spec(make(), X, Y)
    L = dev.lib()

    def taken(m):
        return {"predict_y": m.predict_y(X, S, seed=3)[0], "elbo": np.array(m.compute_log_likelihood(X, Y, seed=3)),
                "input_gradient": m.input_gradient(X, Y, S=S, seed=3)[1]}

    before = taken(model)
    ev_before = model.evaluate(X, Y, S=S, batch_size=2, seed=3, per_image=True)
    ctx._check(L.dcgp_model_set_eval_views(model._model, 12, 12, 1, len(VIEWS3), VIEWS3.ctypes.data))
    _same(taken(model), before)
    assert not np.array_equal(model.evaluate(X, Y, S=S, batch_size=2, seed=3, per_image=True)["p_mean"], ev_before["p_mean"])   # the setting is live
    ctx._check(L.dcgp_model_set_eval_views(model._model, 0, 0, 0, 0, None))
    _same(model.evaluate(X, Y, S=S, batch_size=2, seed=3, per_image=True), ev_before)
    # one training step with the views set: the ELBO and the parameters of a twin that never had any
    ctx._check(L.dcgp_model_set_eval_views(model._model, 12, 12, 1, len(VIEWS3), VIEWS3.ctypes.data))
    e, e_twin = model.train_step(X, Y, 0.01, seed=8), twin.train_step(X, Y, 0.01, seed=8)
    assert e == e_twin
    va, vb = _values(model), _values(twin)
    assert [n for n, _ in va] == [n for n, _ in vb]
    for (name, a), (_, b) in zip(va, vb):
        assert np.array_equal(a, b), name
    ctx._check(L.dcgp_model_set_eval_views(model._model, 0, 0, 0, 0, None))
    _same(model.evaluate(X, Y, S=S, batch_size=2, seed=3, per_image=True), twin.evaluate(X, Y, S=S, batch_size=2, seed=3, per_image=True))
    model.close(), twin.close()


# ---- 9: the driver -----------------------------------------------------------------------------------------------------------------------
def test_driver_with_the_flags(ctx, tmp_path):
    """ArrayExperiment on 200 + 60 digits with --test-shift 1 --test-flip, two periods of 20 steps: finite log rows, the flags in options.toml,
    and the logged test_accuracy is ``evaluate(views=views(1, True))``'s under the logger's batching (32 images, five samples, seed 0)."""
    from sklearn.datasets import load_digits
    from deepcgp_amd.experiment import ArrayExperiment, read_args, standardise
    from deepcgp_amd.models import AccuracyLogger
    d = load_digits()
    Xtr, Xte = standardise(d.images[:200], d.images[200:260])
    Ytr, Yte = d.target[:200], d.target[200:260]
    args = ["--name", "tta", "--data", "unused", "--log-dir", str(tmp_path), "-M", "16,16", "--feature-maps", "2", "--filter-sizes", "3,3",
            "--strides", "1,1", "--batch-size", "16", "--num-samples", "2", "--test-every", "20", "--test-size", "60", "--lr", "0.001",
            "--test-shift", "1", "--test-flip"]
    np.random.seed(0)
    exp = ArrayExperiment(read_args(args), Xtr, Ytr, Xte, Yte)
    v = augment.views(1, True)
    assert np.array_equal(exp.test_views, v)
    assert [type(l) for l in exp.log.loggers][1] is TTAAccuracyLogger
    try:
        exp.train_step()
        exp.train_step()
    finally:
        exp.conclude()
    with open(os.path.join(str(tmp_path), "tta", "log.csv"), newline="") as f:
        rows = list(csv.reader(f))
    print(rows)
    assert len(rows) == 3 and rows[0][2] == "test_accuracy" and all(np.isfinite(float(x)) for r in rows[1:] for x in r)
    lines = open(os.path.join(str(tmp_path), "tta", "options.toml")).read().splitlines()
    assert "test_shift = 1" in lines and "test_flip = true" in lines and 'test_views = "cross"' in lines
    Xt = exp.X_test.reshape(exp.X_test.shape[0], -1)
    want = exp.model.evaluate(Xt, exp.Y_test, S=5, batch_size=32, seed=0, views=v)["accuracy"]
    assert float(rows[2][2]) == want
    print("test accuracy with views %.4f, without %.4f" % (want, AccuracyLogger(Xt, exp.Y_test)(exp.model)))
    exp.model.close()

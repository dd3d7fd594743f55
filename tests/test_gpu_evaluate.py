"""GPU: DS-DGP's other prediction methods (predict_density, predict_f, predict_all_layers), the one-call test-set evaluation
(dcgp_model_evaluate: one eval_tail launch per batch, one synchronisation per call) and the two log-density loggers."""
import ctypes as C

import numpy as np
import pytest

from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.models import AccuracyLogger, LogLikelihoodLogger, TestLogDensityLogger, build_from_spec
from oracle_build import oracle_model

pytestmark = pytest.mark.gpu

RTOL = 1e-9

GEOMETRIES = {   # the geometries of test_gpu_model.py::test_elbo_vs_oracle_midsize
    "cfg1_small": ((28, 28, 1), [], (5, 1), 32, 4, 2),
    "ch_M40": ((28, 28, 1), [(5, 2, 10)], (5, 1), 40, 3, 2),
    "cifar3": ((32, 32, 3), [(4, 2, 10), (5, 1, 10)], (5, 1), 24, 2, 2),
}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def oracle_log_density(ref, X, Y, S, zs):
    """log (1/S sum_s p_s(y)) from the oracle's class probabilities: logsumexp over the samples minus log S."""
    om, _ = ref.predict_y(X, S, zs=zs)
    l = np.log(om[:, np.arange(X.shape[0]), np.reshape(Y, (-1,))])       # [S, N]
    mx = l.max(axis=0)
    return mx + np.log(np.exp(l - mx).sum(axis=0)) - np.log(S), om


def small_model(N=7, S=5, seed=5):
    hwc = (28, 28, 1)
    spec = syn.make_spec(hwc, [(5, 2, 10)], (5, 1), 32, S=S, num_data=1000, seed=seed, conv_q_sqrt_scale=0.2)
    X, Y = syn.make_batch(hwc, N, seed=seed)
    return spec, X, Y, build_from_spec(spec, X, Y)


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("case", list(GEOMETRIES))
def test_predict_density_vs_oracle(ctx, case, white):
    hwc, convs, head, M, N, S = GEOMETRIES[case]
    spec = syn.make_spec(hwc, convs, head, M, S=S, num_data=50000, seed=42, white=white, conv_q_sqrt_scale=0.2)
    X, Y = syn.make_batch(hwc, N, seed=42)
    zs = syn.make_noise(spec, N, seed=42)
    ref, model = oracle_model(spec, X, Y), build_from_spec(spec, X, Y)
    want, _ = oracle_log_density(ref, X, Y, S, zs)
    got = model.predict_density(X, Y, S, zs=zs)
    assert got.shape == (N, 1)
    assert rel(got[:, 0], want) < RTOL
    model.close()


def test_predict_density_epsilon_and_empty(ctx):
    spec, X, Y, model = small_model(N=5, S=3)
    ref = oracle_model(spec, X, Y)
    eps = 0.05
    ref.likelihood.epsilon = eps
    ref.likelihood.eps_k1 = eps / (ref.likelihood.num_classes - 1.0)
    model.likelihood.epsilon = eps
    model.sync_parameters()
    zs = syn.make_noise(spec, 5, seed=8)
    want, _ = oracle_log_density(ref, X, Y, 3, zs)
    assert rel(model.predict_density(X, Y, 3, zs=zs)[:, 0], want) < RTOL
    assert model.predict_density(X[:0], Y[:0], 3).shape == (0, 1)
    assert model.evaluate(X[:0], Y[:0], S=3)["n"] == 0
    model.close()


def test_evaluate_matches_the_loop_it_replaces(ctx):
    N, S, seed, bs = 7, 5, 11, 3
    spec, X, Y, model = small_model(N=N, S=S)
    r = model.evaluate(X, Y, S=S, batch_size=bs, seed=seed, per_image=True)
    assert r["n"] == N and r["log_density"].shape == (N,) and r["p_mean"].shape == (N, 10)
    assert r["accuracy"] == AccuracyLogger(X, Y, bs, S)(model, seed=seed)
    for i, lo in enumerate(range(0, N, bs)):
        sl = slice(lo, lo + bs)
        pm = model.predict_proba(X[sl], S, seed=seed + i)
        assert np.array_equal(r["p_mean"][sl], pm)                      # bit-identical: the same probabilities, the same sum order
        ld = model.predict_density(X[sl], Y[sl], S, seed=seed + i)[:, 0]
        assert np.max(np.abs(r["log_density"][sl] - ld)) <= 1e-13 * np.max(np.abs(ld))
    want_acc = np.mean(r["p_mean"].argmax(axis=1) == Y)
    assert r["accuracy"] == want_acc
    assert abs(r["mean_log_density"] - r["log_density"].mean()) <= 1e-13 * abs(r["mean_log_density"])
    assert TestLogDensityLogger(X, Y, batch_size=bs, num_samples=S)(model, seed=seed) == \
        model.evaluate(X, Y, S=S, batch_size=bs, seed=seed)["mean_log_density"]
    model.close()


def test_evaluate_explicit_noise_vs_oracle_any_batch_size(ctx):
    N, S = 9, 3
    spec, X, Y, model = small_model(N=N, S=S, seed=7)
    ref = oracle_model(spec, X, Y)
    zs = syn.make_noise(spec, N, seed=3)
    want, om = oracle_log_density(ref, X, Y, S, zs)
    runs = {bs: model.evaluate(X, Y, S=S, batch_size=bs, zs=zs, per_image=True) for bs in (4, 1, N)}
    r = runs[4]
    assert rel(r["log_density"], want) < RTOL
    assert rel(r["p_mean"], om.mean(axis=0)) < RTOL
    assert r["accuracy"] == np.mean(om.mean(axis=0).argmax(axis=1) == Y)
    for bs in (1, N):
        assert np.max(np.abs(runs[bs]["log_density"] - r["log_density"])) <= 1e-12 * np.max(np.abs(r["log_density"]))
        assert np.max(np.abs(runs[bs]["p_mean"] - r["p_mean"])) <= 1e-12
    model.close()


def test_evaluate_runs_the_chain_once(ctx):
    N, S, bs = 10, 2, 3
    nb = 4
    spec, X, Y, model = small_model(N=N, S=S)
    model.set_factor_reuse(1)
    first = model.evaluate(X, Y, S=S, batch_size=bs, seed=2, per_image=True)
    s0 = model.chain_skips
    again = model.evaluate(X, Y, S=S, batch_size=bs, seed=2, per_image=True)
    assert model.chain_skips - s0 == nb
    assert np.array_equal(first["log_density"], again["log_density"]) and np.array_equal(first["p_mean"], again["p_mean"])
    # a parameter written in between: the next call runs the chain again (once) and follows the new value
    model.layers[-1].kern.base_kernel.variance *= 1.7
    model.sync_parameters()
    s1 = model.chain_skips
    moved = model.evaluate(X, Y, S=S, batch_size=bs, seed=2, per_image=True)
    assert model.chain_skips - s1 == nb - 1
    assert not np.array_equal(moved["p_mean"], first["p_mean"])
    model.set_factor_reuse(0)
    s2 = model.chain_skips
    fresh = model.evaluate(X, Y, S=S, batch_size=bs, seed=2, per_image=True)
    assert model.chain_skips == s2
    assert np.array_equal(fresh["p_mean"], moved["p_mean"]) and np.array_equal(fresh["log_density"], moved["log_density"])
    model.close()


def test_evaluate_error_paths(ctx):
    N, S = 6, 2
    spec, X, Y, model = small_model(N=N, S=S)
    good = model.evaluate(X, Y, S=S, batch_size=4, seed=1, per_image=True)
    Z = model.layers[0].feature.Z.copy()
    model.layers[0].feature.Z = np.full_like(Z, np.nan)
    model.sync_parameters()
    with pytest.raises(dev.NotPositiveDefinite):
        model.predict_y(X, S, seed=1)
    with pytest.raises(dev.NotPositiveDefinite):
        model.evaluate(X, Y, S=S, batch_size=4, seed=1)
    with pytest.raises(dev.NotPositiveDefinite):
        model.predict_density(X, Y, S, seed=1)
    model.layers[0].feature.Z = Z
    model.sync_parameters()
    after = model.evaluate(X, Y, S=S, batch_size=4, seed=1, per_image=True)
    assert np.array_equal(after["log_density"], good["log_density"])
    for bad in (10, -1):
        Yb = Y.copy()
        Yb[3] = bad
        with pytest.raises(dev.DcgpError) as e:
            model.evaluate(X, Yb, S=S, batch_size=4, seed=1)
        assert e.value.code == dev.ERR_ARG
        with pytest.raises(dev.DcgpError) as e:
            model.predict_density(X, Yb, S, seed=1)
        assert e.value.code == dev.ERR_ARG
    with pytest.raises(ValueError):
        model.evaluate(X, Y, S=S, batch_size=0)
    # the C entry point itself refuses a batch of 0 images
    dX, dY = ctx.to_device(X), ctx.to_device(Y, np.int32)
    out, info = (C.c_double * 2)(), C.c_int(0)
    rc = dev.lib().dcgp_model_evaluate(model._model, dX.ptr, dY.ptr, N, 0, S, None, 1, None, None, out, C.byref(info))
    assert rc == dev.ERR_ARG
    after = model.evaluate(X, Y, S=S, batch_size=4, seed=1, per_image=True)
    assert np.array_equal(after["log_density"], good["log_density"]) and after["accuracy"] == good["accuracy"]
    model.close()


def test_predict_f_and_predict_all_layers(ctx):
    N, S = 4, 3
    spec, X, Y, model = small_model(N=N, S=S)
    Fs, Fm, Fv = model.propagate(X, S=S, seed=9)
    fm, fv = model.predict_f(X, S, seed=9)
    assert fm.shape == (S, N, 10) and fv.shape == (S, N, 10)
    assert np.array_equal(fm, Fm[-1]) and np.array_equal(fv, Fv[-1])
    zs = syn.make_noise(spec, N, seed=4)
    got, want = model.predict_all_layers(X, S, zs=zs), model.propagate(X, S=S, zs=zs)
    assert len(got) == 3 and len(got[0]) == len(model.layers)
    for a, b in zip(got, want):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    model.close()


def test_log_likelihood_logger_matches_the_reference_formula(ctx):
    hwc, n = (12, 12, 1), 150
    spec = syn.make_spec(hwc, [(3, 2, 4)], (3, 1), M=24, S=3, num_data=n, seed=5, conv_q_sqrt_scale=0.3)
    X, Y = syn.make_batch(hwc, n, seed=5)
    model = build_from_spec(spec, X, Y)
    got = LogLikelihoodLogger()(model, seed=4)
    batches = 3                                       # ceil(150 / 64): the last batch holds 22 images
    want = sum(model.compute_log_likelihood(X[i * 64:(i + 1) * 64], Y[i * 64:(i + 1) * 64], seed=4 + i) for i in range(batches))
    want /= batches * 64
    assert got == want
    assert LogLikelihoodLogger.title == "train_log_likelihood" and TestLogDensityLogger.title == "test_log_likelihood"
    model.close()

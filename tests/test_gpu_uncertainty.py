"""GPU: device uncertainty evaluation (dcgp_model_evaluate_uncertainty, csrc/uncertainty.hip) -- what it shares with evaluate bit for
bit, the entropies / BALD / confidence against the device's own samples and against the oracle, the calibration table, invariances,
error paths, and the mutual information of intact against pixel-shuffled real digits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bernoulli_ref as br
import uncertainty_ref as ur
from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.likelihoods import Bernoulli, Gaussian
from deepcgp_amd.models import UncertaintyLogger, build_from_spec
from oracle_build import oracle_model

pytestmark = pytest.mark.gpu

RTOL = 1e-9          # tests/test_gpu_evaluate.py's bound against the oracle
ATOL_SAMPLES = 1e-12  # against the device's own samples: sums of <= S K terms of size <= 1/e in fp64 round near 1e-14; the margin
                      # covers another summation order and log implementation

GEOMETRIES = {   # tests/test_gpu_evaluate.py's
    "cfg1_small": ((28, 28, 1), [], (5, 1), 32, 4, 2),
    "ch_M40": ((28, 28, 1), [(5, 2, 10)], (5, 1), 40, 3, 2),
    "cifar3": ((32, 32, 3), [(4, 2, 10), (5, 1, 10)], (5, 1), 24, 2, 2),
}
PER_IMAGE = ("predictive_entropy", "expected_entropy", "mutual_information", "confidence", "prediction")
SCALARS = ("accuracy", "mean_log_density", "ece", "mce", "brier", "mean_predictive_entropy", "mean_mutual_information")
TABLE_N, TABLE_S, TABLE_BINS = 24, 3, 5
Q_MU_SCALE = 300.0


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def multiclass_case(case, white, seed=42):
    hwc, convs, head, M, N, S = GEOMETRIES[case]
    spec = syn.make_spec(hwc, convs, head, M, S=S, num_data=50000, seed=seed, white=white, conv_q_sqrt_scale=0.2)
    X, Y = syn.make_batch(hwc, N, seed=seed)
    return spec, X, Y, syn.make_noise(spec, N, seed=seed), N, S


def bernoulli_case(white, N=5, S=3, seed=7, D=3, q_mu_scale=1.0):
    """tests/test_gpu_bernoulli.py's "conv" case."""
    hwc = (10, 10, 1)
    spec = syn.make_spec(hwc, [(3, 1, 2)], (3, 1), 9, S=S, num_data=300, seed=seed, white=white, conv_q_sqrt_scale=0.3, variance=2.0,
                         ls=1.5, head_outputs=D)
    spec["head"]["q_mu"] = spec["head"]["q_mu"] * q_mu_scale
    X, Ylab = syn.make_batch(hwc, N, seed=seed)
    Y = (np.random.default_rng(seed).random((N, D)) < 0.5).astype(np.float64)
    return spec, X, Ylab, Y, syn.make_noise(spec, N, seed=seed), N, S


def table_case_multiclass(seed=5):
    """The calibration inputs: test_gpu_evaluate.py's small model on TABLE_N images, the head's q_mu scaled up -- the synthetic
    parameters alone predict every class at 0.1, one bin; with the scale the confidences spread from 0.12 to 0.99."""
    hwc = (28, 28, 1)
    spec = syn.make_spec(hwc, [(5, 2, 10)], (5, 1), 32, S=TABLE_S, num_data=1000, seed=seed, conv_q_sqrt_scale=0.2)
    spec["head"]["q_mu"] = spec["head"]["q_mu"] * Q_MU_SCALE
    X, Y = syn.make_batch(hwc, TABLE_N, seed=seed)
    return spec, X, Y, syn.make_noise(spec, TABLE_N, seed=seed)


def oracle_probabilities(spec, X, Ylab, S, zs, bernoulli=False):
    ref = oracle_model(spec, X, Ylab)
    if not bernoulli:
        return ref.predict_y(X, S, zs=zs)[0]
    _, Fm, Fv = ref.propagate(X, S=S, zs=zs)          # the oracle has no Bernoulli of its own
    return br.predict_mean_and_var(Fm[-1], Fv[-1])[0]


def mixed_labels(Y, prediction):
    """Every other label replaced by the given prediction, so that correct and wrong entries both occur."""
    Y = np.array(Y)
    flat, pred = Y.reshape(-1), np.asarray(prediction).reshape(-1)
    flat[::2] = pred[::2]
    return Y


# ---- 1. what evaluate already returns is returned bit for bit ----

@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("case", list(GEOMETRIES))
def test_unchanged_quantities_are_bit_identical_multiclass(ctx, case, white):
    spec, X, Y, zs, N, S = multiclass_case(case, white)
    model = build_from_spec(spec, X, Y)
    for kw in (dict(zs=zs, batch_size=2), dict(seed=3, batch_size=3), dict(seed=3, batch_size=32)):
        want = model.evaluate(X, Y, S=S, per_image=True, **kw)
        got = model.evaluate_uncertainty(X, Y, S=S, per_image=True, **kw)
        for k in ("accuracy", "mean_log_density", "n"):
            assert got[k] == want[k], (k, kw)
        assert np.array_equal(got["log_density"], want["log_density"]) and np.array_equal(got["p_mean"], want["p_mean"])
        pu = model.predict_uncertainty(X, S, zs=kw.get("zs"), seed=kw.get("seed", 0), batch_size=kw["batch_size"])
        assert np.array_equal(pu["p_mean"], want["p_mean"])
        for k in PER_IMAGE:
            assert np.array_equal(pu[k], got[k]), k
    model.close()


@pytest.mark.parametrize("white", [False, True])
def test_unchanged_quantities_are_bit_identical_bernoulli(ctx, white):
    spec, X, Ylab, Y, zs, N, S = bernoulli_case(white)
    model = build_from_spec(spec, X, Y, likelihood=Bernoulli())
    for kw in (dict(zs=zs, batch_size=2), dict(seed=3, batch_size=3), dict(seed=3, batch_size=32)):
        want = model.evaluate(X, Y, S=S, per_image=True, **kw)
        got = model.evaluate_uncertainty(X, Y, S=S, per_image=True, **kw)
        for k in ("accuracy", "mean_log_density", "n"):
            assert got[k] == want[k], (k, kw)
        assert np.array_equal(got["log_density"], want["log_density"]) and np.array_equal(got["p_mean"], want["p_mean"])
        pu = model.predict_uncertainty(X, S, zs=kw.get("zs"), seed=kw.get("seed", 0), batch_size=kw["batch_size"])
        assert np.array_equal(pu["p_mean"], want["p_mean"])
        for k in PER_IMAGE:
            assert pu[k].shape == (N, 3) and np.array_equal(pu[k], got[k]), k
    model.close()


# ---- 2. the new quantities against the device's own samples, 3. against the oracle ----

def check_against_samples(got, want, who):
    for k in ("predictive_entropy", "expected_entropy", "mutual_information"):
        err = np.max(np.abs(got[k] - want[k]))
        print("%s %s: max abs error vs own samples %.3e" % (who, k, err))
        assert err <= ATOL_SAMPLES, (who, k, err)
    assert np.array_equal(got["confidence"], want["confidence"]), who
    assert np.array_equal(got["prediction"], want["prediction"]), who


def check_against_oracle(got, want, who):
    for k in ("predictive_entropy", "expected_entropy", "confidence"):
        print("%s %s: relative error vs oracle %.3e" % (who, k, rel(got[k], want[k])))
        assert rel(got[k], want[k]) < RTOL, (who, k)
    # BALD is a difference of near-equal numbers: absolute, scaled by the entropy it is taken from
    excess = np.abs(got["mutual_information"] - want["mutual_information"]) - RTOL * want["predictive_entropy"]
    print("%s mutual_information: max |error| - 1e-9 H = %.3e (H >= %.3e)" % (who, excess.max(), want["predictive_entropy"].min()))
    assert np.all(excess <= 0), who


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("case", list(GEOMETRIES))
def test_entropies_vs_own_samples_and_oracle_multiclass(ctx, case, white):
    spec, X, Y, zs, N, S = multiclass_case(case, white)
    model = build_from_spec(spec, X, Y)
    ps = model.predict_y(X, S, zs=zs)[0]
    got = model.evaluate_uncertainty(X, Y, S=S, batch_size=N, zs=zs, per_image=True)
    assert got["predictive_entropy"].shape == (N,) and got["prediction"].dtype == np.int32
    check_against_samples(got, ur.multiclass(ps), case)
    assert np.array_equal(got["p_mean"], ur.sample_mean(ps))
    check_against_oracle(got, ur.multiclass(oracle_probabilities(spec, X, Y, S, zs)), case)
    assert np.all(got["mutual_information"] >= -ATOL_SAMPLES) and np.all(got["predictive_entropy"] <= np.log(10) + ATOL_SAMPLES)
    model.close()


@pytest.mark.parametrize("white", [False, True])
def test_entropies_vs_own_samples_and_oracle_bernoulli(ctx, white):
    spec, X, Ylab, Y, zs, N, S = bernoulli_case(white)
    model = build_from_spec(spec, X, Y, likelihood=Bernoulli())
    ps = model.predict_y(X, S, zs=zs)[0]
    got = model.evaluate_uncertainty(X, Y, S=S, batch_size=N, zs=zs, per_image=True)
    assert got["predictive_entropy"].shape == (N, 3)
    check_against_samples(got, ur.bernoulli(ps), "bernoulli")
    assert np.array_equal(got["p_mean"], ur.sample_mean(ps))
    check_against_oracle(got, ur.bernoulli(oracle_probabilities(spec, X, Ylab, S, zs, bernoulli=True)), "bernoulli")
    model.close()


# ---- 4. the calibration table ----

def check_table(r, Y, bins, bern, who):
    """Against the reference applied to the device's own p_mean: counts, correct counts and predictions exactly, sums to 1e-12."""
    c = ur.calibration(r["p_mean"], Y, bins, bernoulli_targets=bern)
    count = r["reliability"]["count"]
    assert np.array_equal(count, c["table"][:, 0]) and count.sum() == c["correct"].size, who
    with np.errstate(invalid="ignore"):
        sum_correct = np.where(count > 0, r["reliability"]["accuracy"] * count, 0.0)
        sum_conf = np.where(count > 0, r["reliability"]["confidence"] * count, 0.0)
    assert np.array_equal(np.rint(sum_correct), c["table"][:, 2]) and np.max(np.abs(sum_correct - np.rint(sum_correct))) <= 1e-12, who
    assert np.array_equal(np.isnan(r["reliability"]["confidence"]), count == 0)
    assert np.array_equal(r["prediction"], c["prediction"].reshape(r["prediction"].shape)), who
    assert r["accuracy"] == c["accuracy"], who
    for name, got, want in (("sum_confidence", sum_conf, c["table"][:, 1]), ("ece", r["ece"], c["ece"]), ("mce", r["mce"], c["mce"]),
                            ("brier", r["brier"], c["brier"])):
        print("%s %s: relative error vs reference on the device's p_mean %.3e" % (who, name, rel(got, want)))
        assert rel(got, want) <= 1e-12, (who, name)
    return c


def check_table_vs_oracle(r, om_mean, Y, bins, bern, who):
    """The same table from the oracle's sample-mean probabilities.  An entry could be left out only where a difference below 1e-9 can
    move it to another bin or prediction; the chosen inputs have no such entry (checked here, on the oracle alone)."""
    assert not ur.near_a_decision(om_mean, bins, 1e-9, bernoulli_targets=bern).any(), who
    c = ur.calibration(om_mean, Y, bins, bernoulli_targets=bern)
    count = r["reliability"]["count"]
    assert np.array_equal(count, c["table"][:, 0]), who
    assert np.array_equal(r["prediction"], c["prediction"].reshape(r["prediction"].shape)), who
    assert r["accuracy"] == c["accuracy"], who
    with np.errstate(invalid="ignore"):
        assert np.array_equal(np.rint(np.where(count > 0, r["reliability"]["accuracy"] * count, 0.0)), c["table"][:, 2]), who
        sum_conf = np.where(count > 0, r["reliability"]["confidence"] * count, 0.0)
    for name, got, want in (("sum_confidence", sum_conf, c["table"][:, 1]), ("ece", r["ece"], c["ece"]), ("mce", r["mce"], c["mce"]),
                            ("brier", r["brier"], c["brier"])):
        print("%s %s: relative error vs oracle %.3e" % (who, name, rel(got, want)))
        assert rel(got, want) < RTOL, (who, name)


def test_calibration_table_multiclass(ctx):
    spec, X, Y, zs = table_case_multiclass()
    om = oracle_probabilities(spec, X, Y, TABLE_S, zs)
    om_mean = ur.sample_mean(om)
    Y = mixed_labels(Y, om_mean.argmax(1))
    model = build_from_spec(spec, X, Y)
    # the entropies once more where the predictions differ from image to image (mutual information up to 0.1 nats)
    r = model.evaluate_uncertainty(X, Y, S=TABLE_S, batch_size=TABLE_N, zs=zs, per_image=True)     # (one batch, as predict_y runs it)
    check_against_samples(r, ur.multiclass(model.predict_y(X, TABLE_S, zs=zs)[0]), "multiclass table case")
    check_against_oracle(r, ur.multiclass(om), "multiclass table case")
    for bins in (TABLE_BINS, 15):
        r = model.evaluate_uncertainty(X, Y, S=TABLE_S, batch_size=7, zs=zs, bins=bins, per_image=True)
        c = check_table(r, Y, bins, False, "multiclass bins=%d" % bins)
        assert 0 < c["correct"].sum() < TABLE_N
        check_table_vs_oracle(r, om_mean, Y, bins, False, "multiclass bins=%d" % bins)
        assert abs(r["mean_predictive_entropy"] - r["predictive_entropy"].mean()) <= 1e-12 * r["mean_predictive_entropy"]
        assert abs(r["mean_mutual_information"] - r["mutual_information"].mean()) <= 1e-12 * r["mean_predictive_entropy"]
    # the logger returns the dataset dict
    log = UncertaintyLogger(X, Y, S=TABLE_S, bins=TABLE_BINS, batch_size=7)(model, seed=4)
    again = model.evaluate_uncertainty(X, Y, S=TABLE_S, batch_size=7, seed=4, bins=TABLE_BINS)
    assert all(log[k] == again[k] for k in SCALARS) and np.array_equal(log["reliability"]["count"], again["reliability"]["count"])
    assert "predictive_entropy" not in log
    model.close()


def test_calibration_table_bernoulli(ctx):
    spec, X, Ylab, Y, zs, N, S = bernoulli_case(False, N=TABLE_N, S=TABLE_S, seed=13, q_mu_scale=Q_MU_SCALE)
    om = oracle_probabilities(spec, X, Ylab, S, zs, bernoulli=True)
    om_mean = ur.sample_mean(om)
    Y = mixed_labels(Y, om_mean > 0.5).astype(np.float64)
    model = build_from_spec(spec, X, Y, likelihood=Bernoulli())
    r = model.evaluate_uncertainty(X, Y, S=S, batch_size=N, zs=zs, per_image=True)     # (one batch, as predict_y runs it)
    check_against_samples(r, ur.bernoulli(model.predict_y(X, S, zs=zs)[0]), "bernoulli table case")
    check_against_oracle(r, ur.bernoulli(om), "bernoulli table case")
    for bins in (TABLE_BINS, 15):
        r = model.evaluate_uncertainty(X, Y, S=S, batch_size=7, zs=zs, bins=bins, per_image=True)
        c = check_table(r, Y, bins, True, "bernoulli bins=%d" % bins)
        assert 0 < c["correct"].sum() < TABLE_N * 3
        check_table_vs_oracle(r, om_mean, Y, bins, True, "bernoulli bins=%d" % bins)
    model.close()


# ---- 5. invariance ----

def test_batch_size_repeat_and_one_bin(ctx):
    spec, X, Y, zs = table_case_multiclass()
    N, S = TABLE_N, TABLE_S
    model = build_from_spec(spec, X, Y)
    runs = {bs: model.evaluate_uncertainty(X, Y, S=S, batch_size=bs, zs=zs, bins=TABLE_BINS, per_image=True) for bs in (4, 1, N)}
    r = runs[4]
    for bs in (1, N):
        for k in ("predictive_entropy", "expected_entropy", "mutual_information", "confidence", "p_mean"):
            assert np.max(np.abs(runs[bs][k] - r[k])) <= 1e-12, (bs, k)
        assert np.max(np.abs(runs[bs]["log_density"] - r["log_density"])) <= 1e-12 * np.max(np.abs(r["log_density"]))
        for k in SCALARS:
            assert abs(runs[bs][k] - r[k]) <= 1e-12 * max(abs(r[k]), 1.0), (bs, k)
    again = model.evaluate_uncertainty(X, Y, S=S, batch_size=4, zs=zs, bins=TABLE_BINS, per_image=True)
    for k in PER_IMAGE + ("p_mean", "log_density"):
        assert np.array_equal(again[k], r[k]), k
    assert all(again[k] == r[k] for k in SCALARS)
    for k in ("count", "confidence", "accuracy"):
        assert np.array_equal(again["reliability"][k], r["reliability"][k], equal_nan=True), k
    one = model.evaluate_uncertainty(X, Y, S=S, batch_size=4, zs=zs, bins=1, per_image=True)
    assert one["reliability"]["count"][0] == N and one["reliability"]["accuracy"][0] == one["accuracy"]
    assert one["ece"] == abs(one["accuracy"] - one["reliability"]["confidence"][0]) and one["mce"] == one["ece"]
    assert abs(one["reliability"]["confidence"][0] - one["confidence"].mean()) <= 1e-12
    model.close()


# ---- 6. errors ----

def test_error_paths(ctx):
    N, S = 6, 2
    hwc = (28, 28, 1)
    spec = syn.make_spec(hwc, [(5, 2, 10)], (5, 1), 32, S=S, num_data=1000, seed=5, conv_q_sqrt_scale=0.2)
    X, Y = syn.make_batch(hwc, N, seed=5)
    model = build_from_spec(spec, X, Y)
    good = model.evaluate_uncertainty(X, Y, S=S, batch_size=4, seed=1, per_image=True)
    before = model.evaluate(X, Y, S=S, batch_size=4, seed=1, per_image=True)

    def still_fine():
        after = model.evaluate_uncertainty(X, Y, S=S, batch_size=4, seed=1, per_image=True)
        for k in PER_IMAGE + ("p_mean", "log_density"):
            assert np.array_equal(after[k], good[k]), k
        assert all(after[k] == good[k] for k in SCALARS)
        assert np.array_equal(model.evaluate(X, Y, S=S, batch_size=4, seed=1, per_image=True)["log_density"], before["log_density"])

    with pytest.raises(dev.DcgpError) as e:
        model.evaluate_uncertainty(X, Y, S=S, batch_size=4, seed=1, bins=0)
    assert e.value.code == dev.ERR_ARG
    still_fine()
    for bad in (10, -1):      # a label outside [0, K): reported as evaluate reports it
        Yb = Y.copy()
        Yb[3] = bad
        with pytest.raises(dev.DcgpError) as e:
            model.evaluate_uncertainty(X, Yb, S=S, batch_size=4, seed=1)
        assert e.value.code == dev.ERR_ARG
        with pytest.raises(dev.DcgpError) as e2:
            model.evaluate(X, Yb, S=S, batch_size=4, seed=1)
        assert e2.value.code == e.value.code
        still_fine()
    with pytest.raises(ValueError):
        model.evaluate_uncertainty(X, Y, S=S, batch_size=0)
    # the C entry points themselves: a batch of 0 images, no bins, float targets into a RobustMax model
    L = dev.lib()
    dX, dY = ctx.to_device(X), ctx.to_device(Y, np.int32)
    out, info = (C.c_double * 7)(), C.c_int(0)
    none = [None] * 8
    assert L.dcgp_model_evaluate_uncertainty(model._model, dX.ptr, dY.ptr, N, 0, S, None, 1, 15, *none, out, C.byref(info)) == dev.ERR_ARG
    assert L.dcgp_model_evaluate_uncertainty(model._model, dX.ptr, dY.ptr, N, 4, S, None, 1, 0, *none, out, C.byref(info)) == dev.ERR_ARG
    assert L.dcgp_model_evaluate_uncertainty_f64y(model._model, dX.ptr, None, N, 4, S, None, 1, 15, *none, out, C.byref(info)) == dev.ERR_ARG
    still_fine()
    # a not-positive-definite Kuu is reported as evaluate reports it
    Z = model.layers[0].feature.Z.copy()
    model.layers[0].feature.Z = np.full_like(Z, np.nan)
    model.sync_parameters()
    with pytest.raises(dev.NotPositiveDefinite):
        model.evaluate_uncertainty(X, Y, S=S, batch_size=4, seed=1)
    model.layers[0].feature.Z = Z
    model.sync_parameters()
    still_fine()
    assert model.evaluate_uncertainty(X[:0], Y[:0], S=S)["n"] == 0
    empty = model.predict_uncertainty(X[:0], S)
    assert empty["p_mean"].shape == (0, 10) and empty["mutual_information"].shape == (0,)
    model.close()
    # the int32 entry on a Bernoulli model, and a Bernoulli model after it
    spec, X, Ylab, Y, zs, N, S = bernoulli_case(False)
    bm = build_from_spec(spec, X, Y, likelihood=Bernoulli())
    good = bm.evaluate_uncertainty(X, Y, S=S, batch_size=4, seed=1, per_image=True)
    dX, dY = ctx.to_device(X), ctx.to_device(Ylab.astype(np.int32) % 3, np.int32)
    assert L.dcgp_model_evaluate_uncertainty(bm._model, dX.ptr, dY.ptr, N, 4, S, None, 1, 15, *none, out, C.byref(info)) == dev.ERR_ARG
    assert L.dcgp_model_evaluate_uncertainty_f64y(bm._model, dX.ptr, None, N, 4, S, None, 1, 0, *none, out, C.byref(info)) == dev.ERR_ARG
    after = bm.evaluate_uncertainty(X, Y, S=S, batch_size=4, seed=1, per_image=True)
    for k in PER_IMAGE + ("p_mean", "log_density"):
        assert np.array_equal(after[k], good[k]), k
    bm.close()
    ga = build_from_spec(spec, X, Y, likelihood=Gaussian(0.5))
    with pytest.raises(ValueError):
        ga.evaluate_uncertainty(X, Y, S=S)
    with pytest.raises(ValueError):
        ga.predict_uncertainty(X, S)
    ga._build()
    dYf = ctx.to_device(Y)
    assert L.dcgp_model_evaluate_uncertainty_f64y(ga._model, dX.ptr, dYf.ptr, N, 4, S, None, 1, 15, *none, out, C.byref(info)) == dev.ERR_ARG
    assert np.isfinite(ga.evaluate(X, Y, S=S)["mean_log_density"])
    ga.close()


# ---- 7. behaviour on real images ----

def test_mutual_information_rises_on_shuffled_digits(ctx):
    """sklearn's 8 x 8 digits, the "conv" variant (one ConvLayer + head) trained as tests/test_gpu_model.py::test_learns_real_digits trains
    it (750 Adam steps in blocks of 250): the mean mutual information of test images whose pixels are shuffled by one fixed permutation
    exceeds that of the intact test images.  No margin is fixed; both values are printed (DESIGN.md records them).  The "head" variant
    has nothing to compare: without a sampled hidden layer its S samples are the same distribution and the mutual information is
    zero up to rounding."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from digits_train import VARIANTS, digits
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder, train
    Xtr, Ytr, Xte, Yte = digits()
    flags = default_parser().parse_args(["--name", "digits", "--batch-size", "64", "--lr", "0.01", "--num-samples", "5"] + VARIANTS["conv"])
    np.random.seed(0)
    model = ModelBuilder(flags, Xtr, Ytr.reshape(-1, 1)).build()
    for done in (0, 250, 500):
        train(model, 250, lr=0.01, lr_decay_steps=10 ** 9, global_step=done, seed=0)
    Xte = Xte.reshape(len(Xte), -1)
    perm = np.random.default_rng(0).permutation(Xte.shape[1])
    intact = model.evaluate_uncertainty(Xte, Yte, S=5, per_image=True)
    shuffled = model.evaluate_uncertainty(Xte[:, perm], Yte, S=5, per_image=True)
    mi_in, mi_out = intact["mean_mutual_information"], shuffled["mean_mutual_information"]
    print("digits conv variant, 750 steps: accuracy %.4f ece %.4f brier %.4f | mean mutual information intact %.6e shuffled %.6e ratio %.2f"
          " | mean predictive entropy intact %.4f shuffled %.4f"
          % (intact["accuracy"], intact["ece"], intact["brier"], mi_in, mi_out, mi_out / mi_in, intact["mean_predictive_entropy"],
             shuffled["mean_predictive_entropy"]))
    assert intact["accuracy"] >= 0.93, intact["accuracy"]
    assert np.array_equal(model.predict_uncertainty(Xte, 5, batch_size=32)["mutual_information"], intact["mutual_information"])
    assert mi_out > mi_in, (mi_in, mi_out)
    model.close()

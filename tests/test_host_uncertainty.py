"""CPU: the host closed forms of the predictive uncertainty (likelihoods.MultiClass / Bernoulli.predictive_uncertainty) against the
NumPy reference (tests/uncertainty_ref.py) and scipy.stats.entropy, known answers of the definitions, and the C-ABI declarations of
dcgp_model_evaluate_uncertainty and its _f64y twin."""
import re

import numpy as np
import pytest
from scipy.stats import entropy

import uncertainty_ref as ur
from deepcgp_amd import device as dev
from deepcgp_amd.likelihoods import Bernoulli, MultiClass

KEYS = ("p_mean", "predictive_entropy", "expected_entropy", "mutual_information", "confidence")


def test_multiclass_closed_forms_vs_reference_and_scipy():
    rng = np.random.default_rng(1)
    ps = rng.dirichlet(np.full(10, 0.3), (5, 40)) * (1 - 1e-3) + 1e-4          # S x N x K, every entry > 0
    got, want = MultiClass.predictive_uncertainty(ps), ur.multiclass(ps)
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.max(np.abs(got[k] - want[k])) <= 1e-14, k
    assert np.array_equal(got["prediction"], want["prediction"]) and got["prediction"].shape == (40,)
    norm = ps / ps.sum(-1, keepdims=True)
    u = MultiClass.predictive_uncertainty(norm)
    assert np.max(np.abs(u["predictive_entropy"] - entropy(norm.mean(0), axis=-1))) <= 1e-13
    assert np.max(np.abs(u["expected_entropy"] - entropy(norm, axis=-1).mean(0))) <= 1e-13
    assert np.all(u["mutual_information"] >= -1e-13)


def test_bernoulli_closed_forms_vs_reference_and_scipy():
    rng = np.random.default_rng(2)
    ps = rng.uniform(1e-3, 1 - 1e-3, (4, 30, 3))
    got, want = Bernoulli.predictive_uncertainty(ps), ur.bernoulli(ps)
    for k in KEYS:
        assert got[k].shape == (30, 3) and np.max(np.abs(got[k] - want[k])) <= 1e-14, k
    assert np.array_equal(got["prediction"], want["prediction"])
    two = np.stack([ps, 1 - ps])                                               # scipy's entropy over the two outcomes
    assert np.max(np.abs(got["expected_entropy"] - entropy(two, axis=0).mean(0))) <= 1e-13
    pbar = ps.mean(0)
    assert np.max(np.abs(got["predictive_entropy"] - entropy(np.stack([pbar, 1 - pbar]), axis=0))) <= 1e-13
    assert np.array_equal(got["confidence"], np.maximum(got["p_mean"], 1 - got["p_mean"]))


def test_known_answers():
    K, S, N = 7, 4, 3
    # identical samples: the mutual information is exactly zero (powers of two keep the sample mean exact)
    one = np.array([0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.015625])
    ps = np.tile(one, (S, N, 1))
    for lik, ref in ((MultiClass, ur.multiclass),):
        assert np.all(lik.predictive_uncertainty(ps)["mutual_information"] == 0.0)
        assert np.all(ref(ps)["mutual_information"] == 0.0)
    pb = np.tile(np.array([0.25, 0.5, 0.875]), (S, N, 1))
    assert np.all(Bernoulli.predictive_uncertainty(pb)["mutual_information"] == 0.0)
    assert np.all(ur.bernoulli(pb)["mutual_information"] == 0.0)
    # a uniform mean: log K, also when the samples are one-sided (maximal disagreement: mutual information = log K - H(sample))
    u = MultiClass.predictive_uncertainty(np.full((S, N, K), 1.0 / K))
    assert np.allclose(u["predictive_entropy"], np.log(K), rtol=0, atol=1e-15) and np.all(u["prediction"] == 0)   # first index on ties
    assert np.allclose(u["confidence"], 1.0 / K, rtol=0, atol=1e-16)
    eps = 1e-3
    hot = np.full((K, 1, K), eps / (K - 1)) + np.eye(K)[:, None, :] * (1 - eps - eps / (K - 1))
    u = MultiClass.predictive_uncertainty(hot)
    h_one = -((1 - eps) * np.log(1 - eps) + eps * np.log(eps / (K - 1)))
    assert abs(u["predictive_entropy"][0] - np.log(K)) <= 1e-14 and abs(u["mutual_information"][0] - (np.log(K) - h_one)) <= 1e-14
    b = Bernoulli.predictive_uncertainty(np.full((S, N, 2), 0.5))
    assert np.allclose(b["predictive_entropy"], np.log(2), rtol=0, atol=1e-16) and np.all(b["prediction"] == 0)


def test_hand_built_three_bin_table():
    # six images, two classes; confidences 0.9 0.8 | 0.6 0.55 0.5 | (none below 1/3), with bins=3: bin 2 = [2/3, 1], bin 1 = [1/3, 2/3)
    pbar = np.array([[0.9, 0.1], [0.2, 0.8], [0.6, 0.4], [0.45, 0.55], [0.5, 0.5], [1.0, 0.0]])
    Y = np.array([0, 0, 0, 1, 1, 0])
    c = ur.calibration(pbar, Y, 3)
    assert np.array_equal(c["prediction"], [0, 1, 0, 1, 0, 0])            # the tie goes to the first index
    assert np.array_equal(c["correct"], [True, False, True, True, False, True])
    want = np.array([[0, 0, 0], [3, 0.6 + 0.55 + 0.5, 2], [3, 0.9 + 0.8 + 1.0, 2]])     # confidence 1.0 lands in the last bin
    assert np.array_equal(c["table"][:, [0, 2]], want[:, [0, 2]]) and np.allclose(c["table"][:, 1], want[:, 1], rtol=0, atol=1e-15)
    gap1, gap2 = abs(2 - 1.65) / 3, abs(2 - 2.7) / 3
    assert abs(c["ece"] - (0.5 * gap1 + 0.5 * gap2)) <= 1e-15 and abs(c["mce"] - gap2) <= 1e-15
    assert abs(c["brier"] - (2 * 0.01 + 2 * 0.64 + 2 * 0.16 + 2 * 0.2025 + 2 * 0.25 + 0) / 6) <= 1e-15
    # one bin: |accuracy - mean confidence|
    one = ur.calibration(pbar, Y, 1)
    assert abs(one["ece"] - abs(4 / 6 - pbar.max(1).mean())) <= 1e-15 and one["ece"] == one["mce"]
    # Bernoulli entries
    pb = np.array([[0.9, 0.2], [0.5, 0.7]])
    cb = ur.calibration(pb, np.array([[1, 0], [1, 0]]), 2, bernoulli_targets=True)
    assert np.array_equal(cb["correct"], [[True, True], [False, False]]) and np.array_equal(cb["table"][:, 0], [0, 4])
    assert abs(cb["brier"] - (0.01 + 0.04 + 0.25 + 0.49) / 4) <= 1e-15


def test_near_a_decision_flags_edges_and_ties():
    pbar = np.array([[0.6, 0.4], [0.5 + 2e-10, 0.5 - 2e-10], [0.8 + 5e-10, 0.2 - 5e-10], [0.7, 0.3]])
    assert np.array_equal(ur.near_a_decision(pbar, 5), [True, True, True, False])      # 0.6 and 0.8 are edges of five bins
    assert np.array_equal(ur.near_a_decision(pbar, 3), [False, True, False, False])


def _declaration(src, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,label", [("dcgp_model_evaluate_uncertainty", "const int32_t* y"),
                                        ("dcgp_model_evaluate_uncertainty_f64y", "const double* y")])
def test_uncertainty_declarations_parse(name, label):
    with open(dev.HEADER_PATH) as fh:
        src = fh.read()
    assert name in dev.declared_symbols()
    args = _declaration(src, name)
    assert len(args) == 19 == len(dev._SIGS[name]), (name, args)
    assert args[0].startswith("dcgp_model*") and label in args
    for a in ("int bins", "double* out_table", "double* out_host", "int32_t* out_prediction", "double* out_mutual_info"):
        assert a in args, a

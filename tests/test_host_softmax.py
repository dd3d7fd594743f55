"""Host side of the Softmax likelihood (no GPU): the default node table, the closed forms against torch, the --likelihood flag."""
import numpy as np
import pytest

from deepcgp_amd import device as dev
from deepcgp_amd.arguments import default_parser
from deepcgp_amd.likelihoods import MultiClass, Softmax
from deepcgp_amd.models import ModelBuilder

NEW_SYMBOLS = ("dcgp_model_set_likelihood_nodes", "dcgp_softmax_varexp", "dcgp_softmax_predict")


def test_default_table_shape_pairs_and_seed():
    a = Softmax(10)
    assert a.nodes.shape == (100, 10) and a.nodes.dtype == np.float64 and a.num_monte_carlo_points == 100
    assert np.array_equal(a.nodes[:50], np.random.RandomState(0).standard_normal((50, 10)))
    assert np.array_equal(a.nodes[50:], -a.nodes[:50])
    assert np.array_equal(Softmax(10, seed=0).nodes, a.nodes) and not np.array_equal(Softmax(10, seed=1).nodes, a.nodes)
    odd = Softmax(3, num_monte_carlo_points=7, seed=4)
    assert odd.nodes.shape == (7, 3) and np.array_equal(odd.nodes[3:6], -odd.nodes[:3])
    one = Softmax(4, num_monte_carlo_points=1)
    assert one.nodes.shape == (1, 4)
    given = np.arange(6.0).reshape(2, 3)
    assert np.array_equal(Softmax(3, nodes=given).nodes, given)
    with pytest.raises(ValueError):
        Softmax(3, nodes=np.zeros((2, 4)))
    with pytest.raises(ValueError):
        Softmax(1)
    with pytest.raises(ValueError):
        Softmax(10, num_monte_carlo_points=410)                           # Q * K > 4096
    b = Softmax(5, 12, seed=2)
    old = b.nodes.copy()
    new = b.resample(np.random.RandomState(9))
    assert new.shape == old.shape and not np.array_equal(new, old) and np.array_equal(new[6:], -new[:6])
    assert np.array_equal(new[:6], np.random.RandomState(9).standard_normal((6, 5)))
    assert Softmax.predictive_uncertainty is MultiClass.predictive_uncertainty


def test_closed_forms_against_torch():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    n, K = 9, 5
    lik = Softmax(K, 14, seed=5)
    m, v, y = 2.0 * rng.standard_normal((n, K)), rng.random((n, K)) + 0.05, rng.integers(0, K, n)
    v[2, 1] = 0.0                                                         # the clamp: no derivative there
    m[4], m[5, 0], m[5, 1] = 800.0 * np.sign(rng.standard_normal(K)), 800.0, -800.0
    F = rng.standard_normal((n, K)) * 3
    tF = torch.tensor(F)
    assert np.allclose(lik.logp(F, y), torch.log_softmax(tF, -1)[torch.arange(n), torch.tensor(y)].numpy(), rtol=1e-13, atol=1e-13)
    assert np.allclose(lik.conditional_mean(F), torch.softmax(tF, -1).numpy(), rtol=1e-13, atol=1e-15)
    p = lik.conditional_mean(F)
    assert np.allclose(lik.conditional_variance(F), p - p * p, rtol=0, atol=1e-16)
    # the rule in torch: ve, p and the two derivative formulas of the variational expectation
    tm, tv = torch.tensor(m, requires_grad=True), torch.tensor(v, requires_grad=True)
    e = torch.tensor(lik.nodes)
    s = torch.sqrt(torch.clamp(tv, min=1e-10))
    f = tm[:, None, :] + s[:, None, :] * e[None]
    ls = torch.log_softmax(f, -1)
    ve = ls[torch.arange(n), :, torch.tensor(y)].mean(1)
    gm, gv = torch.autograd.grad(ve.sum(), [tm, tv])
    sig = np.exp(ls.detach().numpy())                                     # [n, Q, K]
    ind = np.eye(K)[y][:, None, :]
    sd = np.sqrt(np.maximum(v, 1e-10))
    want_m = (ind - sig).mean(1)
    want_v = np.where(v > 1e-10, ((ind - sig) * lik.nodes[None]).mean(1) / (2 * sd), 0.0)
    assert np.allclose(gm.numpy(), want_m, rtol=1e-12, atol=1e-14) and np.allclose(gv.numpy(), want_v, rtol=1e-12, atol=1e-14)
    pm, pv = lik.predict_mean_and_var(m, v)
    assert np.all(np.isfinite(pm)) and np.abs(pm.sum(1) - 1.0).max() < 1e-14
    assert np.allclose(pm, sig.mean(1), rtol=1e-12, atol=1e-300) and np.allclose(pv, pm - pm * pm, rtol=0, atol=1e-16)
    ld = lik.predict_density(m, v, y)
    assert np.allclose(ld[pm[np.arange(n), y] > 0], np.log(pm[np.arange(n), y])[pm[np.arange(n), y] > 0], rtol=1e-13)
    import softmax_ref as sr
    assert np.allclose(sr.variational_expectations(m, v, y, lik.nodes), ve.detach().numpy(), rtol=1e-13, atol=1e-13)
    assert np.allclose(sr.predict_mean_and_var(m, v, lik.nodes)[0], pm, rtol=1e-12, atol=1e-300)


def test_new_entry_points_are_declared_and_bound():
    declared = set(dev.declared_symbols())
    for name in NEW_SYMBOLS:
        assert name in declared and name in dev._SIGS, name
    assert len(dev._SIGS["dcgp_softmax_varexp"]) == 9 and len(dev._SIGS["dcgp_softmax_predict"]) == 8


def _flags(extra):
    return default_parser().parse_args(["--name", "t", "--batch-size", "8", "--num-samples", "2", "-M", "4", "--feature-maps", "", "--filter-sizes",
                                        "3", "--strides", "1"] + extra)


def test_likelihood_flag_and_model_builder():
    assert _flags([]).likelihood == "robustmax"
    X = np.random.default_rng(0).standard_normal((20, 6, 6, 1))
    Y = np.arange(20).reshape(-1, 1) % 10
    assert isinstance(ModelBuilder(_flags([]), X, Y).likelihood(), MultiClass)
    lik = ModelBuilder(_flags(["--likelihood", "softmax"]), X, Y).likelihood()
    assert isinstance(lik, Softmax) and lik.num_classes == 10 and lik.nodes.shape == (100, 10)
    with pytest.raises(ValueError) as err:      # refused before anything is built
        ModelBuilder(_flags(["--likelihood", "probit"]), X, Y).build()
    assert "robustmax" in str(err.value) and "softmax" in str(err.value)
    # a model with the class: int32 labels, no likelihood entry among the parameters (the table is no parameter)
    from deepcgp_amd import synthetic as syn
    from deepcgp_amd.models import build_from_spec
    spec = syn.make_spec((6, 6, 1), [], (3, 1), 4, S=2, num_data=20, seed=1, head_outputs=10)
    sm = build_from_spec(spec, X.reshape(20, -1), Y, likelihood=lik)
    assert sm.softmax and not sm.float_targets and sm.Y.dtype == np.int32 and sm.Y.shape == (20,)
    assert not any("likelihood" in p.pathname for p in sm.parameters)

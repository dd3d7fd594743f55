"""CPU: the StudentT and Poisson likelihoods' host side -- logp against torch.distributions, the closed forms against SciPy's adaptive
quadrature and the 20-node rule, constructor and target checks, the checkpoint path and the C-ABI declarations."""
import numpy as np
import pytest
from scipy import integrate

import quad_ref as qr
from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.likelihoods import Poisson, StudentT
from deepcgp_amd.models import AccuracyLogger, build_from_spec

NEW_SYMBOLS = ["dcgp_model_set_likelihood_params", "dcgp_quad_varexp", "dcgp_quad_predict", "dcgp_quad_logdensity", "dcgp_quad_grad_seeds"]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


@pytest.mark.parametrize("scale,nu", [(1.0, 3.0), (0.7, 4.5), (2.5, 2.1), (0.05, 30.0)])
def test_student_t_logp_vs_torch(scale, nu):
    torch = pytest.importorskip("torch")
    F = np.linspace(-6, 6, 25)[:, None] * np.ones((1, 7))
    Y = np.array([-40.0, -3.0, -0.2, 0.0, 0.9, 8.0, 55.0])[None] * np.ones((25, 1))
    want = torch.distributions.StudentT(torch.tensor(nu, dtype=torch.float64), loc=torch.tensor(F), scale=torch.tensor(scale, dtype=torch.float64)
                                        ).log_prob(torch.tensor(Y)).numpy()
    for got in (StudentT(scale, nu).logp(F, Y), qr.logp(("studentt", scale, nu), F, Y)):
        assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-13


@pytest.mark.parametrize("b", [1.0, 2.5, 0.3])
def test_poisson_logp_vs_torch(b):
    torch = pytest.importorskip("torch")
    F = np.linspace(-4, 4, 17)[:, None] * np.ones((1, 6))
    Y = np.array([0.0, 1.0, 2.0, 7.0, 60.0, 300.0])[None] * np.ones((17, 1))
    want = torch.distributions.Poisson(torch.tensor(b * np.exp(F))).log_prob(torch.tensor(Y)).numpy()
    for got in (Poisson(binsize=b).logp(F, Y), qr.logp(("poisson", b), F, Y)):
        assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-13


@pytest.mark.parametrize("m,v", [(0.7, 0.4), (-0.5, 0.055), (0.4, 0.91), (-4.0, 2.0), (4.0, 0.2), (0.0, 1e-12)])
@pytest.mark.parametrize("y,b", [(0.0, 1.0), (3.0, 2.5), (60.0, 1.0)])
def test_poisson_closed_form_vs_adaptive_quadrature(m, v, y, b):
    """E_{f ~ N(m, v)} logp(f, y) by SciPy's adaptive quadrature against gpflow's closed form, 1e-9 relative to max(1, |value|)."""
    lik = Poisson(binsize=b)
    sd = np.sqrt(v)

    def integrand(f):
        return np.exp(-0.5 * ((f - m) / sd) ** 2) / (sd * np.sqrt(2 * np.pi)) * float(lik.logp(f, y))
    want, err = integrate.quad(integrand, m - 12 * sd, m + 12 * sd, epsabs=1e-13, epsrel=1e-13, limit=400)
    got = float(qr.variational_expectations(("poisson", b), m, v, y))
    assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (got, want, err)


def test_poisson_predictive_mean_is_the_lognormal_mean():
    """E_y of the 20-node rule against b exp(m + v / 2) for v <= 0.5 (e^f is entire: the rule's error there is rounding), and V_y
    against the closed form E_y + (e^v - 1) E_y^2 of a Poisson mixed over a log-normal rate."""
    for b in (1.0, 2.5):
        lik = Poisson(binsize=b)
        m = np.array([0.7, -0.5, 0.4, -2.0, 2.0, 0.0])
        v = np.array([0.4, 0.055, 0.5, 0.3, 0.1, 0.0])
        want = b * np.exp(m + 0.5 * v)
        for e, vy in (lik.predict_mean_and_var(m, v), qr.predict_mean_and_var(("poisson", b), m, v)):
            print("Poisson E_y relative error %.3e" % np.max(np.abs(e - want) / want))
            assert np.max(np.abs(e - want) / want) <= 1e-10
            wv = want + np.expm1(np.maximum(v, 5e-11)) * want ** 2     # (the rule's clamp: 2 v >= 1e-10)
            assert np.max(np.abs(vy - wv) / wv) <= 1e-9
    e, _ = Poisson().predict_mean_and_var(np.array(0.7), np.array(0.4))
    assert abs(float(e) - np.exp(0.9)) <= 1e-14 * np.exp(0.9)


def test_student_t_predictive_closed_forms():
    """E_y = m and V_y = v + scale^2 nu / (nu - 2): the rule integrates f and f^2 exactly."""
    for scale, nu in ((0.7, 3.0), (1.3, 4.5)):
        lik = StudentT(scale, nu)
        m = np.array([0.3, -0.5, 4.0, -4.0, 0.0])
        v = np.array([0.4, 0.055, 2.0, 0.91, 0.0])
        for e, vy in (lik.predict_mean_and_var(m, v), qr.predict_mean_and_var(("studentt", scale, nu), m, v)):
            assert np.max(np.abs(e - m)) <= 1e-14
            want = np.maximum(v, 5e-11) + scale ** 2 * nu / (nu - 2)
            assert rel(vy, want) <= 1e-13
        assert np.array_equal(lik.conditional_mean(m), m)
        assert np.allclose(lik.conditional_variance(m), scale ** 2 * nu / (nu - 2), rtol=1e-15)


def test_host_classes_agree_with_the_reference_forms():
    rng = np.random.default_rng(0)
    m, v = rng.standard_normal((6, 3)), rng.random((6, 3)) + 0.05
    for lik, tup, Y in ((StudentT(0.7, 4.5), ("studentt", 0.7, 4.5), rng.standard_normal((6, 3))),
                        (Poisson(binsize=2.5), ("poisson", 2.5), rng.poisson(2.5, (6, 3)).astype(np.float64))):
        assert rel(lik.predict_density(m, v, Y), qr.log_density(tup, m, v, Y)) <= 1e-13
        e, vy = lik.predict_mean_and_var(m, v)
        we, wv = qr.predict_mean_and_var(tup, m, v)
        assert rel(e, we) <= 1e-14 and rel(vy, wv) <= 1e-13
    # one sample, zero variance: the density collapses to logp at the mean (up to the clamp's 1e-5-wide spread)
    assert abs(float(StudentT(1.0, 3.0).predict_density(np.array(0.2), np.array(0.0), np.array(0.5))) - float(StudentT(1.0, 3.0).logp(0.2, 0.5))) <= 1e-9


def test_constructors():
    assert (StudentT().scale, StudentT().deg_free) == (1.0, 3.0)
    assert (Poisson().invlink, Poisson().binsize) == ("exp", 1.0)
    for kw in (dict(scale=0.0), dict(scale=1e-6), dict(scale=-1.0), dict(scale=float("nan")), dict(deg_free=2.0), dict(deg_free=1.0),
               dict(deg_free=float("inf"))):
        with pytest.raises(ValueError, match="StudentT"):
            StudentT(**kw)
    for kw in (dict(invlink="log1pexp"), dict(invlink="probit"), dict(binsize=0.0), dict(binsize=-2.0), dict(binsize=float("inf"))):
        with pytest.raises(ValueError, match="Poisson"):
            Poisson(**kw)


def _spec(D):   # (head only: a conv layer's prior factorisation needs the device)
    return syn.make_spec((10, 10, 1), [], (3, 1), 9, S=2, num_data=100, seed=1, head_outputs=D)


def test_targets():
    X, _ = syn.make_batch((10, 10, 1), 4, seed=1)
    Y = np.array([[1, 0, 3], [0, 0, 60], [2, 1, 1], [0, 7, 0]])
    for t in (Y, Y.astype(np.float32), Y.astype(np.int64)):
        m = build_from_spec(_spec(3), X, t, likelihood=Poisson())
        assert m.poisson and m.float_targets and not m.gaussian and not m.student_t
        assert m.Y.dtype == np.float64 and np.array_equal(m.Y, Y)
        assert not any("likelihood" in p.pathname for p in m.parameters)
    one = build_from_spec(_spec(1), X, Y[:, 0], likelihood=Poisson())      # D = 1 accepts a flat count vector
    assert one.Y.shape == (4, 1)
    for bad, word in ((Y - 1, ">= 0"), (Y * 0.5, "integer"), (np.where(Y == 60, np.inf, Y), "finite"), (np.where(Y == 60, np.nan, Y), "finite")):
        with pytest.raises(ValueError, match="Poisson likelihood.*" + word):
            build_from_spec(_spec(3), X, bad, likelihood=Poisson())
    with pytest.raises(ValueError, match="Poisson likelihood"):
        build_from_spec(_spec(3), X, Y[:, :2], likelihood=Poisson())
    Yr = np.random.default_rng(1).standard_normal((4, 3))
    st = build_from_spec(_spec(3), X, Yr, likelihood=StudentT(0.7))
    assert st.student_t and st.float_targets and not st.poisson and np.array_equal(st.Y, Yr)
    with pytest.raises(ValueError, match="StudentT likelihood"):
        build_from_spec(_spec(3), X, Yr[:, :2], likelihood=StudentT())


def test_checkpoint_path_and_refusals_that_need_no_device():
    X, _ = syn.make_batch((10, 10, 1), 4, seed=1)
    Yr = np.random.default_rng(1).standard_normal((4, 3))
    st = build_from_spec(_spec(3), X, Yr, likelihood=StudentT(0.7, 4.5))
    names = [p.pathname for p in st.parameters]
    assert names[0] == "DGP/likelihood/likelihood/scale" and "DGP/likelihood/likelihood/variance" not in names
    assert not any("deg_free" in n or "epsilon" in n for n in names)
    st.parameters[0].assign(0.25)
    assert st.likelihood.scale == 0.25 and float(st.parameters[0].value) == 0.25
    po = build_from_spec(_spec(3), X, np.ones((4, 3)), likelihood=Poisson())
    for model, name in ((st, "StudentT"), (po, "Poisson")):
        with pytest.raises(ValueError, match=name):
            model.predict_proba(X, 2)
        with pytest.raises(ValueError, match=name):
            model.evaluate_uncertainty(X, model.Y)
        with pytest.raises(ValueError, match=name):
            model.predict_uncertainty(X, 2)
        with pytest.raises(ValueError, match=name):
            AccuracyLogger(X, model.Y)(model)
        with pytest.raises(NotImplementedError, match=name):
            model.input_gradient(X, model.Y, objective="density")


def test_new_entry_points_are_declared_and_bound():
    declared = set(dev.declared_symbols())
    for name in NEW_SYMBOLS:
        assert name in declared and name in dev._SIGS, name

"""CPU: the Bernoulli likelihood's host side -- closed forms against SciPy, target checks, the logger and the C-ABI declarations."""
import numpy as np
import pytest
from scipy import integrate
from scipy.special import ndtr

from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.likelihoods import Bernoulli
from deepcgp_amd.models import AccuracyLogger, build_from_spec

NEW_SYMBOLS = ["dcgp_model_set_likelihood", "dcgp_elbo_forward_f64y", "dcgp_elbo_forward_enqueue_f64y", "dcgp_elbo_grad_f64y",
               "dcgp_model_train_step_adam_f64y", "dcgp_model_predict_mean_var", "dcgp_model_predict_density_f64y",
               "dcgp_model_evaluate_f64y"]


def test_probit_and_logp():
    lik = Bernoulli()
    x = np.linspace(-9, 9, 37)
    p = lik.conditional_mean(x)
    assert np.allclose(p, ndtr(x) * (1 - 2e-3) + 1e-3, rtol=1e-12, atol=0)
    assert p.min() >= 1e-3 and p.max() <= 1 - 1e-3
    assert np.allclose(lik.conditional_variance(x), p - p * p, rtol=1e-14)
    # Y == 1 positive, anything else negative (gpflow's tf.equal(Y, 1))
    assert np.array_equal(lik.logp(x, np.ones_like(x)), np.log(p))
    assert np.array_equal(lik.logp(x, np.zeros_like(x)), np.log(1 - p))
    assert np.array_equal(lik.logp(x, np.full_like(x, 2.0)), np.log(1 - p))
    with pytest.raises(ValueError):
        Bernoulli(invlink="logit")


@pytest.mark.parametrize("mu,var", [(0.3, 0.2), (-1.2, 1.5), (2.5, 0.05), (0.0, 4.0), (-3.0, 0.7)])
@pytest.mark.parametrize("y", [0.0, 1.0])
def test_variational_expectation_vs_adaptive_quadrature(mu, var, y):
    """E_{f ~ N(mu, var)} log p(y | f) by SciPy's adaptive quadrature.  The same rule at 200 points converges to it, which pins the
    integrand and the node scaling; gpflow's 20-point rule agrees within its own truncation error, measured against the 200-point rule
    (up to 2e-3 where the jitter's bend in log p sits inside a wide Gaussian, as at var = 4)."""
    lik = Bernoulli()
    sd = np.sqrt(var)

    def integrand(f):
        return np.exp(-0.5 * ((f - mu) / sd) ** 2) / (sd * np.sqrt(2 * np.pi)) * float(lik.logp(f, y))
    want, err = integrate.quad(integrand, mu - 12 * sd, mu + 12 * sd, epsabs=1e-13, epsrel=1e-13, limit=200)
    got = float(lik.variational_expectations(np.array(mu), np.array(var), np.array(y)))
    fine = Bernoulli()
    fine.num_gauss_hermite_points = 200
    got200 = float(fine.variational_expectations(np.array(mu), np.array(var), np.array(y)))
    assert abs(got200 - want) <= 1e-6, (got200, want, err)
    assert abs(got - want) <= abs(got - got200) + 1e-6, (got, want)
    assert abs(got - want) <= 2e-3


def test_predictive_identity():
    """int Phi(f) N(f; mu, v) df = Phi(mu / sqrt(1 + v)) before the jitter: predict_mean_and_var's p is that, jittered."""
    lik = Bernoulli()
    for mu, v in [(0.4, 0.3), (-1.5, 2.0), (2.0, 0.01)]:
        sd = np.sqrt(v)
        want, _ = integrate.quad(lambda f: ndtr(f) * np.exp(-0.5 * ((f - mu) / sd) ** 2) / (sd * np.sqrt(2 * np.pi)),
                                 mu - 12 * sd, mu + 12 * sd, epsabs=1e-14, epsrel=1e-13)
        p, var = lik.predict_mean_and_var(np.array(mu), np.array(v))
        assert abs(float(p) - (want * (1 - 2e-3) + 1e-3)) <= 1e-12
        assert abs(float(var) - float(p) * (1 - float(p))) <= 1e-15
        assert float(lik.predict_density(np.array(mu), np.array(v), np.array(1.0))) == float(np.log(p))
        assert float(lik.predict_density(np.array(mu), np.array(v), np.array(0.0))) == float(np.log(1 - p))


def _spec(D):   # (head only: a conv layer's prior factorisation needs the device)
    return syn.make_spec((10, 10, 1), [], (3, 1), 9, S=2, num_data=100, seed=1, head_outputs=D)


def test_targets():
    """Bool, int or float N x D targets in {0, 1}; anything else is refused before the device is touched."""
    X, _ = syn.make_batch((10, 10, 1), 4, seed=1)
    Y = np.array([[1, 0, 1], [0, 0, 1], [1, 1, 1], [0, 1, 0]])
    for t in (Y, Y.astype(bool), Y.astype(np.float32)):
        m = build_from_spec(_spec(3), X, t, likelihood=Bernoulli())
        assert m.bernoulli and m.float_targets and not m.gaussian
        assert m.Y.dtype == np.float64 and np.array_equal(m.Y, Y)
        assert not any("likelihood" in p.pathname for p in m.parameters)
    one = build_from_spec(_spec(1), X, Y[:, 0], likelihood=Bernoulli())      # D = 1 accepts a flat label vector
    assert one.Y.shape == (4, 1)
    for bad in (Y * 2, Y - 1, Y * 0.5):
        with pytest.raises(ValueError):
            build_from_spec(_spec(3), X, bad, likelihood=Bernoulli())
    with pytest.raises(ValueError):
        build_from_spec(_spec(3), X, Y[:, :2], likelihood=Bernoulli())


def test_accuracy_logger_thresholds_the_sample_mean():
    X = np.zeros((5, 100))
    Y = np.array([[1, 0], [0, 0], [1, 1], [0, 1], [1, 0]])
    P = np.array([[0.9, 0.2], [0.5, 0.1], [0.51, 0.4], [0.3, 0.7], [0.2, 0.6]])

    class Stub:   # predict_proba of a Bernoulli model: the sample-mean p, N x D
        bernoulli, gaussian = True, False

        def __init__(self):
            self.calls = []

        def predict_proba(self, Xb, S, seed=0):
            lo = sum(len(c) for c, _ in self.calls)
            self.calls.append((Xb, seed))
            return P[lo:lo + len(Xb)]
    stub = Stub()
    # correct: (0.9 vs 1, 0.2 vs 0) (0.5 is not > 0.5 vs 0, 0.1 vs 0) (0.51 vs 1, 0.4 vs 1 wrong) (0.3 vs 0, 0.7 vs 1) (0.2 vs 1 wrong, 0.6 vs 0 wrong)
    assert AccuracyLogger(X, Y, batch_size=2, num_samples=3)(stub, seed=10) == 7 / 10
    assert [s for _, s in stub.calls] == [10, 11, 12]


def test_new_entry_points_are_declared_and_bound():
    declared = set(dev.declared_symbols())
    for name in NEW_SYMBOLS:
        assert name in declared and name in dev._SIGS, name

"""CPU: the Gaussian likelihood's host side -- closed forms, target checks, checkpoint naming, loggers and the C-ABI declarations."""
import numpy as np
import pytest

from deepcgp_amd import device as dev
from deepcgp_amd.likelihoods import Gaussian
from deepcgp_amd.models import AccuracyLogger, TestLogDensityLogger

NEW_SYMBOLS = ["dcgp_model_set_likelihood", "dcgp_elbo_forward_f64y", "dcgp_elbo_forward_enqueue_f64y", "dcgp_elbo_grad_f64y",
               "dcgp_model_train_step_adam_f64y", "dcgp_model_predict_mean_var", "dcgp_model_predict_density_f64y",
               "dcgp_model_evaluate_f64y"]


def test_closed_forms():
    lik = Gaussian(0.3)
    rng = np.random.default_rng(0)
    mu, var, y = rng.standard_normal((5, 2)), rng.random((5, 2)), rng.standard_normal((5, 2))
    # E_{f ~ N(mu, var)} log N(y; f, s2) by Monte Carlo-free quadrature (Gauss-Hermite is exact for this quadratic)
    x, w = np.polynomial.hermite.hermgauss(20)
    f = mu[..., None] + np.sqrt(2 * var)[..., None] * x
    quad = (lik.logp(f, y[..., None]) * w).sum(-1) / np.sqrt(np.pi)
    assert np.allclose(lik.variational_expectations(mu, var, y), quad, rtol=1e-12)
    m, v = lik.predict_mean_and_var(mu, var)
    assert np.array_equal(m, mu) and np.array_equal(v, var + 0.3)
    dens = np.exp(lik.predict_density(mu, var, y))
    assert np.allclose(dens, np.exp(-0.5 * (y - mu) ** 2 / (var + 0.3)) / np.sqrt(2 * np.pi * (var + 0.3)))
    with pytest.raises(ValueError):
        Gaussian(0.0)


def test_loggers():
    X = np.zeros((4, 100))
    Y = np.random.default_rng(1).standard_normal((4, 3))
    assert TestLogDensityLogger(X, Y).Y_test.shape == (4, 3)
    assert TestLogDensityLogger(X, np.arange(4).reshape(4, 1)).Y_test.shape == (4,)

    class GaussianModel:   # AccuracyLogger refuses before it touches the model
        gaussian = True
    with pytest.raises(ValueError):
        AccuracyLogger(X, Y)(GaussianModel())


def test_new_entry_points_are_declared_and_bound():
    declared = set(dev.declared_symbols())
    for name in NEW_SYMBOLS:
        assert name in declared and name in dev._SIGS, name

"""Test helper: the Bernoulli (probit) likelihood's tails in NumPy / SciPy, written from gpflow 1.x likelihoods.Bernoulli,
logdensities.bernoulli and Likelihood.variational_expectations (ndiagquad, 20 Gauss-Hermite points) under DS-DGP's
BroadcastingLikelihood, on top of the oracle's propagate."""
import numpy as np
from scipy.special import logsumexp, ndtr

from oracle_build import oracle_model


def probit(x):
    return ndtr(x) * (1 - 2e-3) + 1e-3


def logp(F, Y):
    p = probit(F)
    return np.where(np.asarray(Y) == 1, np.log(p), np.log(1 - p))


def variational_expectations(m, v, Y):
    """sum_i w_i / sqrt(pi) logp(m + sqrt(2 v) x_i, Y) per element (2 v clamped at 1e-10, as the device tail clamps it)."""
    x, w = np.polynomial.hermite.hermgauss(20)
    F = m[..., None] + np.sqrt(np.maximum(2 * v, 1e-10))[..., None] * x
    return (logp(F, np.asarray(Y)[..., None]) * (w / np.sqrt(np.pi))).sum(-1)


def predict_mean_and_var(m, v):
    p = probit(m / np.sqrt(1 + v))
    return p, p - p * p


def predict_density(m, v, Y):
    """m, v [S, N, D] -> [N, D]: logsumexp_s logp(Y; p_s) - log S."""
    p = predict_mean_and_var(m, v)[0]
    l = np.where(np.asarray(Y)[None] == 1, np.log(p), np.log(1 - p))
    return logsumexp(l, axis=0) - np.log(m.shape[0])


def elbo(spec, X, Ylab, Y, zs):
    """(ELBO, data term, KL) of DGP_Base._build_likelihood: the mean over S of the per-row sums, summed over N, scaled by num_data / N,
    minus the layers' KL."""
    ref = oracle_model(spec, X, Ylab)
    S, N = spec["S"], X.shape[0]
    _, Fm, Fv = ref.propagate(X, S=S, zs=zs)
    ve = variational_expectations(Fm[-1], Fv[-1], np.broadcast_to(Y[None], Fm[-1].shape))     # [S, N, D]
    data = ve.sum(2).mean(0).sum()
    kl = sum(l.KL() for l in ref.layers)
    return data * spec["num_data"] / N - kl, data, kl

"""Test helper: the Softmax likelihood's tails in NumPy / SciPy -- gpflow 1.x likelihoods.SoftMax as a MonteCarloLikelihood with the
per-call draw replaced by a fixed table of nodes [Q, K] -- on top of the oracle's propagate."""
import numpy as np
from scipy.special import logsumexp

from oracle_build import oracle_model


def latents(m, v, nodes):
    """[..., Q, K]: f_q = m + sqrt(max(v, 1e-10)) * nodes[q] (the clamp of the device tails)."""
    return np.asarray(m)[..., None, :] + np.sqrt(np.maximum(v, 1e-10))[..., None, :] * np.asarray(nodes)


def variational_expectations(m, v, y, nodes):
    """1/Q sum_q (f_q[y] - logsumexp_k f_q[k]); m, v [..., K], y [...] integer labels."""
    F = latents(m, v, nodes)
    y = np.broadcast_to(np.asarray(y, np.int64), F.shape[:-2])
    fy = np.take_along_axis(F, y[..., None, None], -1)[..., 0]
    return (fy - logsumexp(F, axis=-1)).mean(-1)


def predict_mean_and_var(m, v, nodes):
    F = latents(m, v, nodes)
    p = np.exp(F - logsumexp(F, axis=-1, keepdims=True)).mean(-2)
    return p, p - p * p


def predict_density(m, v, y, nodes):
    """m, v [S, N, K] -> [N]: log(1/S sum_s p_s[y])."""
    p = predict_mean_and_var(m, v, nodes)[0]
    y = np.asarray(y, np.int64).reshape(-1)
    return np.log(p[:, np.arange(len(y)), y].mean(0))


def head(spec, X, Ylab, zs):
    """(oracle model, Fmean, Fvar [S, N, K]) of the head."""
    ref = oracle_model(spec, X, Ylab)
    _, Fm, Fv = ref.propagate(X, S=spec["S"], zs=zs)
    return ref, Fm[-1], Fv[-1]


def elbo(spec, X, Ylab, zs, nodes):
    """(ELBO, data term, KL) of DGP_Base._build_likelihood: the mean over S of the rows' expectations, summed over N, scaled by
    num_data / N, minus the layers' KL."""
    ref, m, v = head(spec, X, Ylab, zs)
    N = X.shape[0]
    ve = variational_expectations(m, v, np.asarray(Ylab).reshape(1, N), nodes)     # [S, N]
    data = ve.mean(0).sum()
    kl = sum(l.KL() for l in ref.layers)
    return data * spec["num_data"] / N - kl, data, kl

"""Test helper: the StudentT and Poisson likelihoods' tails in NumPy / SciPy, written from gpflow 1.x likelihoods.StudentT / Poisson,
Likelihood.variational_expectations / predict_mean_and_var / predict_density (ndiagquad, 20 Gauss-Hermite points) under DS-DGP's
BroadcastingLikelihood, on top of the oracle's propagate -- and the same forward in torch with logp written by torch.distributions, for
autograd.  A likelihood is named by a tuple: ("studentt", scale, deg_free) or ("poisson", binsize)."""
import math

import numpy as np
from scipy.special import gammaln, logsumexp

from oracle_build import oracle_model


def logp(lik, F, Y):
    F, Y = np.asarray(F, np.float64), np.asarray(Y, np.float64)
    if lik[0] == "studentt":
        _, s, nu = lik
        c = gammaln(0.5 * (nu + 1)) - gammaln(0.5 * nu) - 0.5 * np.log(nu * np.pi)
        return c - np.log(s) - 0.5 * (nu + 1) * np.log1p(np.square((Y - F) / s) / nu)
    b = lik[1]
    return Y * (F + np.log(b)) - b * np.exp(F) - gammaln(Y + 1.0)


def cond_mean(lik, F):
    return np.asarray(F, np.float64) if lik[0] == "studentt" else lik[1] * np.exp(F)


def cond_var(lik, F):
    return np.full(np.shape(F), lik[1] ** 2 * lik[2] / (lik[2] - 2.0)) if lik[0] == "studentt" else lik[1] * np.exp(F)


def nodes(m, v):
    """(f_i [..., 20], c_i [20]): f_i = m + sqrt(max(2 v, 1e-10)) x_i, c_i = w_i / sqrt(pi)"""
    x, w = np.polynomial.hermite.hermgauss(20)
    m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
    return m[..., None] + np.sqrt(np.maximum(2 * v, 1e-10))[..., None] * x, w / np.sqrt(np.pi)


def variational_expectations(lik, m, v, Y):
    """StudentT: sum_i c_i logp(f_i, Y); Poisson: gpflow's closed form for the exp link (no quadrature, no clamp)."""
    m, v, Y = (np.asarray(a, np.float64) for a in (m, v, Y))
    if lik[0] == "poisson":
        b = lik[1]
        return Y * m - b * np.exp(m + 0.5 * v) - gammaln(Y + 1.0) + Y * np.log(b)
    F, c = nodes(m, v)
    return (logp(lik, F, Y[..., None]) * c).sum(-1)


def predict_mean_and_var(lik, m, v):
    F, c = nodes(m, v)
    cm = cond_mean(lik, F)
    e = (cm * c).sum(-1)
    return e, ((cond_var(lik, F) + cm * cm) * c).sum(-1) - e * e


def log_density(lik, m, v, Y):
    """logsumexp_i (logp(f_i, Y) + log c_i) per element"""
    F, c = nodes(m, v)
    return logsumexp(logp(lik, F, np.asarray(Y, np.float64)[..., None]) + np.log(c), axis=-1)


def predict_density(lik, m, v, Y):
    """m, v [S, N, D] -> [N, D]: logsumexp_s ld_s - log S."""
    return logsumexp(log_density(lik, m, v, np.broadcast_to(np.asarray(Y)[None], m.shape)), axis=0) - np.log(m.shape[0])


_HEAD = {}


def head_marginals(spec, X, Ylab, zs, key=None):
    """(Fmean, Fvar [S, N, D], KL) of the oracle; computed once per `key` and shared by the tests that ask for the same case."""
    if key is not None and key in _HEAD:
        return _HEAD[key]
    ref = oracle_model(spec, X, Ylab)
    _, Fm, Fv = ref.propagate(X, S=spec["S"], zs=zs)
    out = (Fm[-1], Fv[-1], sum(l.KL() for l in ref.layers))
    for a in out[:2]:
        a.setflags(write=False)
    if key is not None:
        _HEAD[key] = out
    return out


def elbo(lik, spec, X, Ylab, Y, zs, key=None):
    """(ELBO, data term, KL) of DGP_Base._build_likelihood: the mean over S of the per-row sums, summed over N, scaled by num_data / N,
    minus the layers' KL."""
    m, v, kl = head_marginals(spec, X, Ylab, zs, key)
    ve = variational_expectations(lik, m, v, np.broadcast_to(Y[None], m.shape))     # [S, N, D]
    data = ve.sum(2).mean(0).sum()
    return data * spec["num_data"] / X.shape[0] - kl, data, kl


def torch_logp(lik, F, y, scale=None):
    """logp by torch.distributions: StudentT(df, loc=F, scale).log_prob(y) / Poisson(rate = b e^F).log_prob(y).  `scale` (a tensor) replaces the
    tuple's scale where the caller differentiates with respect to it."""
    import torch
    if lik[0] == "studentt":
        s = scale if scale is not None else torch.tensor(lik[1], dtype=torch.float64)
        return torch.distributions.StudentT(torch.tensor(lik[2], dtype=torch.float64), loc=F, scale=s).log_prob(y)
    return torch.distributions.Poisson(lik[1] * torch.exp(F)).log_prob(y)


def torch_ve(lik, m, v, y, scale=None):
    """The variational expectation on tensors m, v, y of one shape.  StudentT: sum_i c_i logp(f_i, y).  Poisson: gpflow's closed form (no
    quadrature, no clamp), written as Poisson(rate = b exp(m + v / 2)).log_prob(y) - y v / 2 = y (m + log b) - b exp(m + v / 2) - lgamma(y + 1)."""
    import torch
    if lik[0] == "poisson":
        return torch.distributions.Poisson(lik[1] * torch.exp(m + 0.5 * v)).log_prob(y) - 0.5 * y * v
    gx, gw = np.polynomial.hermite.hermgauss(20)
    gx, gw = torch.tensor(gx, dtype=torch.float64), torch.tensor(gw / math.sqrt(math.pi), dtype=torch.float64)
    F = m[..., None] + torch.sqrt(torch.clamp(2.0 * v, min=1e-10))[..., None] * gx
    return (torch_logp(lik, F, y[..., None].expand(F.shape), scale) * gw).sum(-1)


def torch_elbo(lik, spec, X, Ylab, Y, zs):
    """(ELBO tensor, leaves per layer, the scale leaf or None): test_oracle_autograd's torch forward with the RobustMax tail replaced."""
    import torch
    import test_oracle_autograd as ta
    Ylab = np.asarray(Ylab) % Y.shape[1]          # (labels of the RobustMax forward the KL is recovered from)
    e_rm, leaves, m, v = ta._torch_elbo(spec, X, Ylab, zs, want_head=True)
    S, N = spec["S"], X.shape[0]
    y = torch.tensor(np.tile(np.asarray(Ylab).reshape(1, N), [S, 1]).reshape(S * N), dtype=torch.long)
    ve_rm = ta._robustmax_ve(m.reshape(S * N, -1), v.reshape(S * N, -1), y).reshape(S, N).mean(0).sum()
    kl = ve_rm * (spec["num_data"] / N) - e_rm
    scale = torch.tensor(lik[1], dtype=torch.float64, requires_grad=True) if lik[0] == "studentt" else None
    yt = torch.tensor(Y, dtype=torch.float64)[None].expand(m.shape)
    ve = torch_ve(lik, m, v, yt, scale)      # [S, N, D]
    return ve.sum(2).mean(0).sum() * (spec["num_data"] / N) - kl, leaves, scale

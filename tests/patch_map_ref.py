"""Test helper: float64 NumPy restatement of the per-patch evidence maps, written from
    c[n, p, r] = (w_p / P) * sum_m k(z_m, x_n[p]) * beta[m, r],      Fmean[n, r] = sum_p c[n, p, r],
beta = L^-T q_mu (white) or Kuu^-1 q_mu with L = chol(Kuu + jitter I); patches in FullView's (kh, kw, c) order."""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

from oracle.views import FullView


def rbf(A, B, variance, ls, exact=False):
    """[len(A), len(B)].  exact: squared distances from the differences themselves (no cancellation; for large arguments)."""
    if exact:
        sq = np.empty((A.shape[0], B.shape[0]))
        for i in range(A.shape[0]):
            d = B - A[i]
            sq[i] = np.einsum("nl,nl->n", d, d)
    else:
        sq = np.maximum(np.sum(A * A, 1)[:, None] + np.sum(B * B, 1)[None, :] - 2.0 * A @ B.T, 0.0)
    return variance * np.exp(-0.5 * sq / ls ** 2)


def patches(X, geom):
    """X [N, H*W*C] or NHWC -> [N, P, L] in (kh, kw, c) order, through the oracle's FullView."""
    H, W, C, f, s = geom
    return FullView((H, W), f, C, s).extract_patches(np.asarray(X, np.float64).reshape(-1, H, W, C))


def patch_mean(X, geom, Z, variance, ls, w, beta, exact=False):
    """[N, P, R]"""
    pt = patches(X, geom)
    N, P, L = pt.shape
    k = rbf(np.asarray(Z, np.float64), pt.reshape(N * P, L), variance, ls, exact)       # M x NP
    c = (k.T @ np.asarray(beta, np.float64)).reshape(N, P, -1)
    return c * (np.asarray(w, np.float64) / P)[None, :, None]


def head_beta(Z, variance, ls, q_mu, white, jitter):
    Ku = rbf(Z, Z, variance, ls) + jitter * np.eye(Z.shape[0])
    Lu = np.linalg.cholesky(Ku)
    if white:
        return solve_triangular(Lu.T, q_mu, lower=False)
    return cho_solve((Lu, True), q_mu)


def head_patch_mean(h, X, jitter):
    """Per-patch maps of the head `h` of a deepcgp_amd.synthetic spec on its input X [N, H*W*C]."""
    geom = (h["H"], h["W"], h["C"], h["f"], h["s"])
    beta = head_beta(h["Z"], h["variance"], h["ls"], h["q_mu"], h["white"], jitter)
    return patch_mean(X, geom, h["Z"], h["variance"], h["ls"], h["w"], beta)

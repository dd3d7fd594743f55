"""Test helper: float64 NumPy restatements of the head's full covariances, written from the formulas of conv_gp/kernels.py:34-51,
:81-104 (ConvKernel.K / AdditivePatchKernel.K, X2 reshaped like X) and of DS-DGP's SVGP_Layer.conditional_ND(full_cov=True), on top
of the oracle's patch view and base kernels."""
import numpy as np
from scipy.linalg import solve_triangular


def rbf(A, B, variance, ls):
    sq = np.sum(A * A, 1)[:, None] + np.sum(B * B, 1)[None, :] - 2.0 * A @ B.T
    return variance * np.exp(-0.5 * sq / ls ** 2)


def patch_K(view, X, X2, variance, ls, w, additive, rows=None):
    """[N, N2] (rows: only these rows of it).  X, X2: NHWC; X2 None -> X."""
    X2 = X if X2 is None else X2
    Pa, Pb = view.extract_patches(X), view.extract_patches(X2)          # N x P x L
    N, P, L = Pa.shape
    N2 = Pb.shape[0]
    rows = np.arange(N) if rows is None else np.asarray(rows)
    w = np.asarray(w, np.float64)
    out = np.empty((rows.size, N2))
    flatb = Pb.reshape(N2 * P, L)
    for i, n in enumerate(rows):
        if additive:
            out[i] = sum(w[p] * rbf(Pa[n, p][None], Pb[:, p], variance, ls)[0] for p in range(P)) / P
        else:
            k = rbf(Pa[n], flatb, variance, ls).reshape(P, N2, P)       # p x n' x p'
            out[i] = np.einsum("pmq,p,q->m", k, w, w) / P ** 2
    return out


def head_full_cov(Kuf, Ku, Kff, q_mu, q_sqrt, white):
    """mean [N, R], var [N, N, R]: var_r = Kff - A1^T A1 + (Lq_r^T A)^T (Lq_r^T A), A1 = Lu^-1 Kuf, A = A1 or Lu^-T A1."""
    Lu = np.linalg.cholesky(Ku)
    A1 = solve_triangular(Lu, Kuf, lower=True)
    A = A1 if white else solve_triangular(Lu.T, A1, lower=False)
    mean = A.T @ q_mu
    base = Kff - A1.T @ A1
    R = q_mu.shape[1]
    var = np.empty(Kff.shape + (R,))
    for r in range(R):
        T = np.tril(q_sqrt[r]).T @ A
        var[:, :, r] = base + T.T @ T
    return mean, var

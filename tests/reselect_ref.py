"""Float64 NumPy mirror of the inducing-point transfer q'(u') = int p(u' | u) q(u) du (csrc/transfer.hip), of the cross Gram matrix it is built from
and of the Nystrom trace, written from the formulas alone: the four base kernels and RBF-ARD, squared distances from explicit differences, both
whitenings.  Shared by tests/test_host_reselect.py and tests/test_gpu_reselect.py; imports nothing of the package."""
import numpy as np

KINDS = ("rbf", "acos", "matern32", "matern52")
KIND_CODE = {"rbf": 0, "acos": 1, "matern32": 2, "matern52": 3}


def cross(A, B, kind, variance, p1=1.0, p2=0.0, ard=None):
    """k(a_i, b_j), [m, n], the kernels' off-diagonal form.  kind "rbf" (p1 the lengthscale, or ``ard`` [d] lengthscales), "matern32" / "matern52"
    (r = sqrt(|x - z|^2 / l^2 + 1e-12)), "acos" (order 0; p1 the weight variance, p2 the bias variance)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    if kind == "acos":
        # products summed the same way for x.z, |x|^2 and |z|^2: on coincident rows the cosine is an exact 1
        dot = p1 * np.sum(A[:, None, :] * B[None, :, :], axis=-1) + p2
        na = p1 * np.sum(A[:, None, :] * A[:, None, :], axis=-1) + p2
        nb = p1 * np.sum(B[None, :, :] * B[None, :, :], axis=-1) + p2
        cos = dot / np.sqrt(na * nb)
        theta = np.arccos(np.minimum(1e-15 + (1.0 - 2e-15) * cos, 1.0))
        return variance * (np.pi - theta) / np.pi
    scale = np.asarray(ard, np.float64) if ard is not None else float(p1)
    diff = A[:, None, :] / scale - B[None, :, :] / scale
    r2 = np.sum(diff * diff, axis=-1)
    if kind == "rbf":
        return variance * np.exp(-0.5 * r2)
    r = np.sqrt(r2 + 1e-12)
    a = np.sqrt(3.0 if kind == "matern32" else 5.0) * r
    if kind == "matern32":
        return variance * (1.0 + a) * np.exp(-a)
    if kind == "matern52":
        return variance * (1.0 + a + a * a / 3.0) * np.exp(-a)
    raise ValueError(kind)


def kdiag(kind, variance):
    """A Gram matrix's own diagonal: variance; for the ArcCosine the entry its formula gives at cos = 1."""
    return variance * (np.pi - np.arccos(1.0 - 1e-15)) / np.pi if kind == "acos" else float(variance)


def gram(Z, kind, variance, p1=1.0, p2=0.0, ard=None, jitter=0.0):
    """k(Z, Z) + jitter I as the Kuu operators form it."""
    K = cross(Z, Z, kind, variance, p1, p2, ard)
    K = 0.5 * (K + K.T)
    if kind == "acos":
        K[np.diag_indices_from(K)] = kdiag(kind, variance)
    return K + jitter * np.eye(K.shape[0])


def new_covariances(Z, Zn, kind, variance, p1, p2, ard, jitter, q_mu, q_sqrt, white):
    """(m' [M', R] and S' [R, M', M'] in UNwhitened coordinates, L, L'): S'_r = Kn - B^T B + T_r^T T_r."""
    K = gram(Z, kind, variance, p1, p2, ard, jitter)
    Kn = gram(Zn, kind, variance, p1, p2, ard, jitter)
    Kc = cross(Z, Zn, kind, variance, p1, p2, ard)
    L, Ln = np.linalg.cholesky(K), np.linalg.cholesky(Kn)
    q_mu = np.asarray(q_mu, np.float64)
    Lq = np.tril(np.asarray(q_sqrt, np.float64))
    if white:
        q_mu, Lq = L @ q_mu, np.einsum("ij,rjk->rik", L, Lq)
    B = np.linalg.solve(L, Kc)
    P = np.linalg.solve(L.T, B)
    base = Kn - B.T @ B
    S = np.empty((Lq.shape[0], Zn.shape[0], Zn.shape[0]))
    for r in range(Lq.shape[0]):
        T = Lq[r].T @ P
        Sr = base + T.T @ T
        S[r] = 0.5 * (Sr + Sr.T)
    return P.T @ q_mu, S, L, Ln


def transfer(Z, Zn, kind, variance, p1, p2, ard, jitter, q_mu, q_sqrt, white=False):
    """(q_mu' [M', R], q_sqrt' [R, M', M']): chol of the new covariances; white: inv(L') of both."""
    mn, S, _, Ln = new_covariances(Z, Zn, kind, variance, p1, p2, ard, jitter, q_mu, q_sqrt, white)
    Ls = np.linalg.cholesky(S)
    if white:
        mn = np.linalg.solve(Ln, mn)
        Ls = np.stack([np.linalg.solve(Ln, Ls[r]) for r in range(Ls.shape[0])])
    return mn, Ls


def gauss_kl(q_mu, q_sqrt, K=None):
    """sum_r KL[N(q_mu_r, q_sqrt_r q_sqrt_r^T) || N(0, K)]; K None: the unit prior of whitened coordinates."""
    M, R = q_mu.shape
    Lk = np.linalg.cholesky(K) if K is not None else np.eye(M)
    total = 0.0
    for r in range(R):
        a = np.linalg.solve(Lk, q_mu[:, r])
        G = np.linalg.solve(Lk, np.tril(q_sqrt[r]))
        total += 0.5 * (a @ a + np.sum(G * G) - M + 2.0 * np.sum(np.log(np.diag(Lk))) - 2.0 * np.sum(np.log(np.abs(np.diag(q_sqrt[r])))))
    return total


def nystrom_trace(Z, cand, kind, variance, p1=1.0, p2=0.0, ard=None, jitter=0.0):
    """tr(K_ff) - |inv(L) k(Z, cand)|_F^2 with L L^T = k(Z, Z) + jitter I: what of the candidates' prior variance Z leaves unexplained."""
    L = np.linalg.cholesky(gram(Z, kind, variance, p1, p2, ard, jitter))
    A = np.linalg.solve(L, cross(Z, cand, kind, variance, p1, p2, ard))
    return cand.shape[0] * kdiag(kind, variance) - np.sum(A * A)


def random_q(rng, M, R, scale=1.0):
    """A q(u): q_mu [M, R], q_sqrt [R, M, M] lower triangular with a positive diagonal, entries of size ``scale``."""
    q_mu = rng.normal(size=(M, R))
    Ls = np.tril(rng.normal(size=(R, M, M))) * 0.3 * scale
    idx = np.arange(M)
    Ls[:, idx, idx] = np.abs(Ls[:, idx, idx]) + 0.1 * scale
    return q_mu, Ls

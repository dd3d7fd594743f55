"""Float64 NumPy reference of greedy conditional-variance selection (a partial pivoted Cholesky factorisation of the candidates' Gram
matrix), written from the algorithm and the four base kernels' formulas alone: plain loops over pivots, ``np.argmax`` (lowest index on ties).
Shared by tests/test_host_greedy.py and tests/test_gpu_greedy.py; imports nothing of the package."""
import numpy as np


def kernel_column(X, j, kind, variance, p1=1.0, p2=0.0, ard=None):
    """k(x_i, x_j) for every row i.  kind: "rbf" (p1 the lengthscale, or ``ard`` [d] lengthscales), "matern32" / "matern52" (p1 the lengthscale,
    r = sqrt(|x - z|^2 / l^2 + 1e-12)), "acos" (order 0; p1 the weight variance, p2 the bias variance)."""
    if kind == "acos":
        dot = p1 * (X @ X[j]) + p2
        norms = p1 * np.sum(X * X, axis=1) + p2
        cos = dot / np.sqrt(norms * norms[j])
        theta = np.arccos(np.minimum(1e-15 + (1.0 - 2e-15) * cos, 1.0))
        return variance * (np.pi - theta) / np.pi
    scale = np.asarray(ard, np.float64) if ard is not None else float(p1)
    diff = (X - X[j]) / scale
    r2 = np.sum(diff * diff, axis=1)
    if kind == "rbf":
        return variance * np.exp(-0.5 * r2)
    r = np.sqrt(r2 + 1e-12)
    if kind == "matern32":
        a = np.sqrt(3.0) * r
        return variance * (1.0 + a) * np.exp(-a)
    if kind == "matern52":
        a = np.sqrt(5.0) * r
        return variance * (1.0 + a + a * a / 3.0) * np.exp(-a)
    raise ValueError(kind)


def kdiag(kind, variance):
    """The Gram matrix's diagonal, where the residual starts: variance for the stationary kernels (gpflow's Kdiag; their k(x, x) is variance to
    1.5e-12), for the ArcCosine the entry its formula gives at cos = 1, variance (1 - acos(1 - 1e-15) / pi), 1.4e-8 variance below Kdiag."""
    return variance * (np.pi - np.arccos(1.0 - 1e-15)) / np.pi if kind == "acos" else float(variance)


def gram(X, kind, variance, p1=1.0, p2=0.0, ard=None):
    return np.stack([kernel_column(X, j, kind, variance, p1, p2, ard) for j in range(X.shape[0])], axis=1)


def greedy_variance_ref(X, k, kind, variance, p1=1.0, p2=0.0, ard=None, min_variance=0.0):
    """{"rows" [k] (-1 behind n_greedy), "n_greedy", "trace" [k] (last value repeated behind n_greedy), "residual" [n], "factor" [k, n] (zero rows
    behind n_greedy), "pivots": the d_j of every pick, "gaps": largest minus second-largest distinct residual in front of every pick}."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    d = np.full(n, kdiag(kind, variance))
    C = np.zeros((k, n))
    rows = np.full(k, -1, np.int64)
    trace = np.zeros(k)
    pivots, gaps = [], []
    n_greedy = k
    for m in range(k):
        j = int(np.argmax(d))
        if d[j] <= min_variance:
            n_greedy = m
            break
        distinct = np.unique(d)
        gaps.append(distinct[-1] - distinct[-2] if distinct.size > 1 else np.inf)
        pivots.append(d[j])
        rows[m] = j
        col = kernel_column(X, j, kind, variance, p1, p2, ard)
        proj = np.zeros(n)
        for t in range(m):
            proj += C[t, j] * C[t]
        c = (col - proj) / np.sqrt(d[j])
        c[d == 0.0] = 0.0            # nothing is left of such a candidate (a pick, or a copy of one): the factor's triangle is exact
        c[j] = np.sqrt(d[j])
        C[m] = c
        d = np.maximum(d - c * c, 0.0)
        d[j] = 0.0
        trace[m] = d.sum()
    trace[n_greedy:] = trace[n_greedy - 1] if n_greedy > 0 else d.sum()
    return {"rows": rows, "n_greedy": n_greedy, "trace": trace, "residual": d, "factor": C, "pivots": np.array(pivots), "gaps": np.array(gaps)}

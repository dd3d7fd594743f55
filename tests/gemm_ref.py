"""The strided GEMM of the reverse pass (csrc/gemm_gen.h) stated in plain NumPy, flags included:

    C_b(i, j) (+)= alpha * colscale_b[j] * (sum_k A_b(i, k) kscale_b[k] B_b(k, j) - sub_v_b[i] sub_x_b(i, j))

then, before the accumulation: lower_only writes 0 at j > i; phi keeps the strictly lower part, halves the diagonal and zeroes the rest; and after it:
mirror stores the entries below the diagonal transposed as well, so that with accumulate the lower triangle accumulates and the upper one is its mirror
image.  Operands are the logical [batch, M, K], [batch, K, N] ... arrays (how they lie in memory is the case table's business); any dtype NumPy can
multiply in: float64, longdouble for the rounding cases, int64 for the self-check of the exact ones."""
import numpy as np


def contraction(A, B, kscale=None, dtype=np.float64):
    """sum_k A_b(i, k) kscale_b[k] B_b(k, j) as [batch, M, N] in `dtype`; a leading extent of 1 in A or B broadcasts over the batch"""
    A, B = np.asarray(A, dtype), np.asarray(B, dtype)
    if kscale is not None:
        B = np.asarray(kscale, dtype)[:, :, None] * B
    if dtype != np.float64:      # no BLAS behind these: NumPy's own loop runs along k, so lay both operands out with k contiguous (speed only)
        A = np.ascontiguousarray(A)
        B = np.swapaxes(np.ascontiguousarray(np.swapaxes(B, -1, -2)), -1, -2)
    return np.matmul(A, B)


def epilogue(P, C0, alpha=1.0, accumulate=False, colscale=None, sub_v=None, sub_x=None, lower_only=False, mirror=False, phi=False):
    """what the operator leaves in C [batch, M, N] for the contraction P [batch or 1, M, N] and the previous content C0"""
    dtype = P.dtype
    batch = C0.shape[0]
    v = np.broadcast_to(P, (batch,) + P.shape[1:]).copy()
    if sub_v is not None:
        v = v - np.asarray(sub_v, dtype)[:, :, None] * np.asarray(sub_x, dtype)
    v = v * dtype.type(alpha)
    if colscale is not None:
        v = v * np.asarray(colscale, dtype)[:, None, :]
    if lower_only:
        v = np.tril(v)
    if phi:
        diag = v * np.eye(v.shape[1], v.shape[2], dtype=dtype)
        v = np.tril(v, -1) + diag / dtype.type(2)
    if accumulate:
        v = v + np.asarray(C0, dtype)
    if mirror:
        v = np.tril(v) + np.transpose(np.tril(v, -1), (0, 2, 1))
    return v


def gemm(A, B, C0, kscale=None, dtype=np.float64, **ep):
    return epilogue(contraction(A, B, kscale, dtype), np.asarray(C0, dtype), **ep)


def magnitude(A, B, C0, alpha=1.0, accumulate=False, colscale=None, kscale=None, sub_v=None, sub_x=None, **_):
    """|alpha| |A| diag|ks| |B| |cs| + |alpha| |sub_v| |sub_x| + |C0|, elementwise [batch, M, N]: what a rounding bound of the operator multiplies
    (the previous content only where it is accumulated)"""
    m = contraction(np.abs(A), np.abs(B), None if kscale is None else np.abs(kscale))
    m = np.broadcast_to(m, (C0.shape[0],) + m.shape[1:]).copy()
    if colscale is not None:
        m = m * np.abs(colscale)[:, None, :]
    if sub_v is not None:
        m = m + np.abs(sub_v)[:, :, None] * np.abs(sub_x)
    return abs(alpha) * m + (np.abs(C0) if accumulate else 0.0)

"""Kernels of the conv-GP path -- same surface as /root/reference/conv_gp/kernels.py, backed by HIP.

``RBF`` stands in for gpflow.kernels.RBF with a scalar lengthscale (what conv_gp/models.py:114-117
builds); the patch kernels keep the reference's names, constructor arguments and method names.
"""
import numpy as np

from . import device as dev

JITTER = 1e-3    # settings.jitter from /root/reference/gpflowrc:11


class RBF:
    """gpflow.kernels.RBF(input_dim, variance, lengthscales, ARD=False) -- parameters + evaluations on device.
    Scalar lengthscale: the base kernel of the conv layers / ConvKernel heads (conv_gp/models.py:114-117,178-185).
    ``ARD=True`` (one lengthscale per input dimension): the dense head of ``--last-kernel rbf`` on the flattened features
    (conv_gp/models.py:160-168), used with ``InducingPoints``; inputs are divided by the lengthscales and the unit-
    lengthscale kernel evaluated, which is gpflow's own formulation.  Also a conv layer's base kernel (``--ard``): one lengthscale per
    patch element, ``input_dim = f * f * C``; not the base kernel of a patch head."""

    def __init__(self, input_dim, variance=1.0, lengthscales=1.0, ARD=False):
        self.input_dim = int(input_dim)
        self.variance = float(variance)
        self.ARD = bool(ARD)
        if self.ARD:
            ls = np.asarray(lengthscales, np.float64)
            self.lengthscales = np.full(self.input_dim, float(ls)) if ls.ndim == 0 else ls.reshape(self.input_dim).copy()
        else:
            self.lengthscales = float(lengthscales)
        if not (self.variance > 0 and np.all(np.asarray(self.lengthscales) > 0)):
            raise ValueError("variance and lengthscales must be positive")

    def K(self, X, X2=None):
        return self._gram(X, 0.0) if X2 is None else self.Kzx(X, X2)

    def _scaled(self, A):
        A = np.ascontiguousarray(A, np.float64)
        if A.shape[1] != self.input_dim:
            raise ValueError("expected inputs of length %d, got %d" % (self.input_dim, A.shape[1]))
        return np.ascontiguousarray(A / self.lengthscales) if self.ARD else A

    def _gram(self, Z, jitter):
        ctx = dev.get_context()
        Z = self._scaled(Z)
        M, L = Z.shape
        dZ, out = ctx.to_device(Z), ctx.empty((M, M))
        ctx._check(dev.lib().dcgp_kuu_rbf(ctx.handle, dZ.ptr, M, L, self.variance, 1.0 if self.ARD else self.lengthscales,
                                          float(jitter), out.ptr))
        return out.numpy()

    # gpflow's InducingPoints dispatch: Kuu = K(Z) + jitter I, Kuf = K(Z, X)
    def Kzz(self, Z):
        return self._gram(Z, 0.0)

    def Kzx(self, Z, X):
        """K(Z, X), M x N, for dense inputs: every row is a 1 x 1 image with D channels, one patch, weight 1."""
        ctx = dev.get_context()
        Z, X = self._scaled(Z), self._scaled(X)
        (M, D), N = Z.shape, X.shape[0]
        if N == 0:
            return np.zeros((M, 0))
        dX, dZ, dw, out = ctx.to_device(X), ctx.to_device(Z), ctx.to_device(np.ones(1)), ctx.empty((M, N))
        ctx._check(dev.lib().dcgp_convkernel_kzx(ctx.handle, dX.ptr, N, 1, 1, D, 1, 1, dZ.ptr, M, self.variance,
                                                 1.0 if self.ARD else self.lengthscales, dw.ptr, out.ptr))
        return out.numpy()

    def Kdiag(self, X):
        return np.full(np.shape(X)[0], self.variance)

    def _describe(self):
        """{type, variance, p1, p2} of dcgp_model_set_param(..., "base_kernel", ...)."""
        return [0.0, self.variance, 1.0 if self.ARD else self.lengthscales, 0.0]

    def _kuf(self, ctx, dX, N, H, W, C, f, s, dZ, M, out, layout):
        if self.ARD:     # one lengthscale per patch element: the sweep's scaling instance (dZ holds the unscaled Z)
            if f * f * C != self.input_dim:
                raise ValueError("RBF(ARD=True) with %d lengthscales on patches of length %d" % (self.input_dim, f * f * C))
            dls = ctx.to_device(np.ascontiguousarray(self.lengthscales, np.float64))
            ctx._check(dev.lib().dcgp_kuf_patches_rbf_ard(ctx.handle, dX.ptr, N, H, W, C, f, s, dZ.ptr, M, self.variance, dls.ptr, out.ptr, layout))
            return
        ctx._check(dev.lib().dcgp_kuf_patches_rbf(ctx.handle, dX.ptr, N, H, W, C, f, s, dZ.ptr, M, self.variance,
                                                  self.lengthscales, out.ptr, layout))


class ArcCosine:
    """gpflow.kernels.ArcCosine(input_dim, order=0) -- the conv layers' base kernel under ``--base-kernel acos``
    (conv_gp/models.py:118-119).  k = variance * (pi - theta) / pi with theta the angle between the augmented inputs,
    <x, z> = weight_variances * x.z + bias_variance; Kdiag = variance.  Order 0 only."""

    def __init__(self, input_dim, order=0, variance=1.0, weight_variances=1.0, bias_variance=1.0):
        if order != 0:
            raise NotImplementedError("only ArcCosine(order=0) is on the accelerated path (the reference uses order 0)")
        self.input_dim = int(input_dim)
        self.order = 0
        self.variance = float(variance)
        self.weight_variances = float(weight_variances)
        self.bias_variance = float(bias_variance)
        if not (self.variance > 0 and self.weight_variances > 0 and self.bias_variance >= 0):
            raise ValueError("variance and weight_variances must be positive, bias_variance non-negative")

    def K(self, X, X2=None):
        if X2 is not None:
            raise NotImplementedError("cross-covariances are evaluated by the fused patch kernels")
        return self._gram(X, 0.0)

    def _gram(self, Z, jitter):
        ctx = dev.get_context()
        Z = np.ascontiguousarray(Z, np.float64)
        M, L = Z.shape
        if L != self.input_dim:
            raise ValueError("expected inputs of length %d, got %d" % (self.input_dim, L))
        dZ, out = ctx.to_device(Z), ctx.empty((M, M))
        ctx._check(dev.lib().dcgp_kuu_acos(ctx.handle, dZ.ptr, M, L, self.variance, self.weight_variances,
                                           self.bias_variance, float(jitter), out.ptr))
        return out.numpy()

    def Kdiag(self, X):
        return np.full(np.shape(X)[0], self.variance)

    def _describe(self):
        return [1.0, self.variance, self.weight_variances, self.bias_variance]

    def _kuf(self, ctx, dX, N, H, W, C, f, s, dZ, M, out, layout):
        ctx._check(dev.lib().dcgp_kuf_patches_acos(ctx.handle, dX.ptr, N, H, W, C, f, s, dZ.ptr, M, self.variance,
                                                   self.weight_variances, self.bias_variance, out.ptr, layout))


class _Matern:
    """gpflow Stationary kernel with ARD=False in the Matern family: k is a function of
    r = sqrt(|x - z|^2 / lengthscales^2 + 1e-12) (gpflow's scaled_euclid_dist); Kdiag = variance.  A base kernel of the conv layers
    (``--base-kernel matern32 | matern52``); the heads stay RBF-based."""

    nu2 = None      # 2 nu: 3 or 5
    _type = None    # dcgp_model_set_param's base-kernel type

    def __init__(self, input_dim, variance=1.0, lengthscales=1.0, ARD=False):
        if ARD:
            raise NotImplementedError("%s: only ARD=False (one lengthscale) is on the accelerated path" % type(self).__name__)
        if np.ndim(lengthscales) != 0:
            raise ValueError("lengthscales must be a scalar")
        self.input_dim = int(input_dim)
        self.variance = float(variance)
        self.lengthscales = float(lengthscales)
        self.ARD = False
        if not (self.variance > 0 and self.lengthscales > 0):
            raise ValueError("variance and lengthscales must be positive")

    def K(self, X, X2=None):
        if X2 is not None:
            raise NotImplementedError("cross-covariances are evaluated by the fused patch kernels")
        return self._gram(X, 0.0)

    def _gram(self, Z, jitter):
        ctx = dev.get_context()
        Z = np.ascontiguousarray(Z, np.float64)
        M, L = Z.shape
        if L != self.input_dim:
            raise ValueError("expected inputs of length %d, got %d" % (self.input_dim, L))
        dZ, out = ctx.to_device(Z), ctx.empty((M, M))
        ctx._check(dev.lib().dcgp_kuu_matern(ctx.handle, dZ.ptr, M, L, self.nu2, self.variance, self.lengthscales, float(jitter), out.ptr))
        return out.numpy()

    def Kdiag(self, X):
        return np.full(np.shape(X)[0], self.variance)

    def _describe(self):
        return [float(self._type), self.variance, self.lengthscales, 0.0]

    def _kuf(self, ctx, dX, N, H, W, C, f, s, dZ, M, out, layout):
        ctx._check(dev.lib().dcgp_kuf_patches_matern(ctx.handle, dX.ptr, N, H, W, C, f, s, dZ.ptr, M, self.nu2, self.variance,
                                                     self.lengthscales, out.ptr, layout))


class Matern32(_Matern):
    """gpflow.kernels.Matern32(input_dim, variance, lengthscales): k = variance (1 + a) exp(-a), a = sqrt(3) r."""
    nu2, _type = 3, 2


class Matern52(_Matern):
    """gpflow.kernels.Matern52(input_dim, variance, lengthscales): k = variance (1 + a + a^2 / 3) exp(-a), a = sqrt(5) r."""
    nu2, _type = 5, 3


class AdditivePatchKernel:
    """K(x, x') = mean_i w_i k(x[i], x'[i]) (conv_gp/kernels.py:15-77).  Kzx / Kdiag / Kzz serve the training path; the full
    ``K`` (prediction with full covariances) runs on the image-pair kernel of csrc/head_full.hip."""

    kernel_type = 1

    def __init__(self, base_kernel, view, patch_weights=None):
        if isinstance(base_kernel, _Matern):
            raise NotImplementedError("the head kernels are RBF-based: Matern base kernels belong to the conv layers")
        self.base_kernel = base_kernel
        self.view = view
        self.patch_length = view.patch_length
        self.patch_count = view.patch_count
        self.image_size = self.view.input_size
        if patch_weights is None or np.size(patch_weights) != self.patch_count:      # kernels.py:26-27
            patch_weights = np.ones(self.patch_count)
        self.patch_weights = np.array(patch_weights, np.float64)

    def _reshape_X(self, ND_X):
        ND_X = np.ascontiguousarray(ND_X, np.float64)
        size = list(self.view.input_size)
        if len(size) == 2:
            size = size + [self.view.feature_maps]
        return ND_X.reshape([ND_X.shape[0]] + size)

    def _padded_X(self, ND_X):
        """The images as the sliding window sees them: reshaped and, on a padded view, with the zero border."""
        return self.view.pad(self._reshape_X(ND_X))

    def _geom(self, X):
        N, H, W, Cc = X.shape
        return N, H, W, Cc, self.view.filter_size, self.view.stride

    def Kzx(self, ML_Z, ND_X):
        ctx = dev.get_context()
        X = self._padded_X(ND_X)
        Z = np.ascontiguousarray(ML_Z, np.float64)
        N, H, W, Cc, f, s = self._geom(X)
        M = Z.shape[0]
        if N == 0:
            return np.zeros((M, 0))
        dX, dZ, dw = ctx.to_device(X), ctx.to_device(Z), ctx.to_device(self.patch_weights)
        out = ctx.empty((M, N))
        ctx._check(dev.lib().dcgp_convkernel_kzx(ctx.handle, dX.ptr, N, H, W, Cc, f, s, dZ.ptr, M,
                                                 self.base_kernel.variance, self.base_kernel.lengthscales, dw.ptr, out.ptr))
        return out.numpy()

    def patch_mean(self, ML_Z, ND_X, beta):
        """[N, P, R] per-patch shares of ``Kzx(Z, X).T @ beta``: out[n, p, r] = (w_p / P) sum_m k(z_m, x_n[p]) beta[m, r], so that
        ``out.sum(1) == Kzx(Z, X).T @ beta`` -- per output, where in the image the evidence comes from (``view.as_maps`` makes images
        of it).  One launch (dcgp_convkernel_patch_mean), K_uf is never stored.  Scalar-lengthscale RBF base kernel only."""
        bk = self.base_kernel
        if not isinstance(bk, RBF) or bk.ARD:
            raise NotImplementedError("patch_mean needs a scalar-lengthscale RBF base kernel")
        Z = np.ascontiguousarray(ML_Z, np.float64)
        beta = np.ascontiguousarray(beta, np.float64)
        if Z.ndim != 2 or Z.shape[1] != self.patch_length:
            raise ValueError("Z must be M x %d, got %s" % (self.patch_length, Z.shape))
        if beta.ndim != 2 or beta.shape[0] != Z.shape[0] or beta.shape[1] < 1:
            raise ValueError("beta must be M x R with M = %d and R >= 1, got %s" % (Z.shape[0], beta.shape))
        X = self._padded_X(ND_X)
        N, H, W, Cc, f, s = self._geom(X)
        M, R = beta.shape
        if N == 0:
            return np.zeros((0, self.patch_count, R))
        ctx = dev.get_context()
        dX, dZ, dw, db = ctx.to_device(X), ctx.to_device(Z), ctx.to_device(self.patch_weights), ctx.to_device(beta)
        out = ctx.empty((N, self.patch_count, R))
        ctx._check(dev.lib().dcgp_convkernel_patch_mean(ctx.handle, dX.ptr, N, H, W, Cc, f, s, dZ.ptr, M, bk.variance, bk.lengthscales,
                                                        dw.ptr, db.ptr, R, out.ptr))
        return out.numpy()

    def Kdiag(self, ND_X):
        ctx = dev.get_context()
        N = np.shape(ND_X)[0]
        if N == 0:
            return np.zeros((0,))
        dw, out = ctx.to_device(self.patch_weights), ctx.empty((N,))
        ctx._check(dev.lib().dcgp_additive_kdiag(ctx.handle, N, self.patch_count, self.base_kernel.variance, dw.ptr, out.ptr))
        return out.numpy()

    def Kzz(self, Z):
        return self.base_kernel.K(Z)

    def K(self, ND_X, X2=None):
        """N x N2 covariance (conv_gp/kernels.py:34-51): K[n, n'] = (1/P) sum_p w_p k(x_{n,p}, x2_{n',p}).  X2 is reshaped like X,
        which is what the reference evidently intends: its :40 names an undefined ``patches`` where X2 is None."""
        X = self._reshape_X(ND_X)
        X2 = None if X2 is None else self._reshape_X(X2)
        return self._K_batched(X[None], None if X2 is None else X2[None])[0]

    def _K_batched(self, X, X2=None):
        """K of B independent image sets in one launch (dcgp_convkernel_k): X [B, N, H, W, C], X2 [B, N2, H, W, C] or None
        (then symmetric: K[b] == K[b].T bit for bit) -> [B, N, N2].  RBF base kernel only (the heads of conv_gp/models.py:178-185)."""
        bk = self.base_kernel
        if not isinstance(bk, RBF) or bk.ARD:
            raise NotImplementedError("the full K of a patch kernel needs a scalar-lengthscale RBF base kernel")
        p = getattr(self.view, "padding", 0)
        border = ((0, 0), (0, 0), (p, p), (p, p), (0, 0))      # a padded view: the zero border around every image of both sets
        X = np.ascontiguousarray(np.pad(X, border) if p else X, np.float64)
        B, N, H, W, Cc = X.shape
        if X2 is not None:
            X2 = np.ascontiguousarray(np.pad(X2, border) if p else X2, np.float64)
            if X2.shape[0] != B or X2.shape[2:] != X.shape[2:]:
                raise ValueError("X2 of shape %s does not match X of shape %s" % (X2.shape, X.shape))
        N2 = N if X2 is None else X2.shape[1]
        if B == 0 or N == 0 or N2 == 0:
            return np.zeros((B, N, N2))
        ctx = dev.get_context()
        dX, dw, out = ctx.to_device(X), ctx.to_device(self.patch_weights), ctx.empty((B, N, N2))
        dX2 = ctx.to_device(X2) if X2 is not None else None
        ctx._check(dev.lib().dcgp_convkernel_k(ctx.handle, dX.ptr, dX2.ptr if dX2 else None, B, N, N2, H, W, Cc, self.view.filter_size,
                                               self.view.stride, bk.variance, bk.lengthscales, dw.ptr, int(self.kernel_type == 1), out.ptr))
        return out.numpy()


class ConvKernel(AdditivePatchKernel):
    """Weighted convolutional kernel of the classification head (conv_gp/kernels.py:79-136)."""

    kernel_type = 0

    def K(self, ND_X, X2=None):
        """N x N2 covariance (conv_gp/kernels.py:81-104): K[n, n'] = (1/P^2) sum_{p,p'} w_p w_p' k(x_{n,p}, x2_{n',p'}), without
        ever forming the NP x N2P patch Gram.  X2 is reshaped like X, which is what the reference evidently intends: its :90
        extracts patches from X2 without that reshape."""
        return AdditivePatchKernel.K(self, ND_X, X2)

    def Kdiag(self, ND_X):
        ctx = dev.get_context()
        X = self._padded_X(ND_X)
        N, H, W, Cc, f, s = self._geom(X)
        if N == 0:
            return np.zeros((0,))
        dX, dw, out = ctx.to_device(X), ctx.to_device(self.patch_weights), ctx.empty((N,))
        ctx._check(dev.lib().dcgp_convkernel_kdiag(ctx.handle, dX.ptr, N, H, W, Cc, f, s, self.base_kernel.variance,
                                                   self.base_kernel.lengthscales, dw.ptr, out.ptr))
        return out.numpy()


def _sample_patches(HW_image, N, patch_size, patch_length):
    """N random patch_size x patch_size patches of ONE image, flattened -- the helper the reference's notebooks import from
    conv_gp/kernels.py (:139-145); same draw order (row, then column, per patch)."""
    rows = np.empty((N, patch_length))
    hi_y, hi_x = HW_image.shape[0] - patch_size, HW_image.shape[1] - patch_size
    for i in range(N):
        top, left = np.random.randint(0, hi_y), np.random.randint(0, hi_x)
        rows[i] = np.reshape(HW_image[top:top + patch_size, left:left + patch_size], patch_length)
    return rows


def kmeans(points, k, max_iter=300, tol=1e-4, rng=None, distinct_start=False):
    """Lloyd's k-means on the device (dcgp_kmeans): sklearn.cluster.KMeans(n_clusters=k, init='random', n_init=1) in
    its own terms -- k random observations as the initial centres, ``tol`` relative to the mean feature variance,
    stop when the summed squared centre shift falls below it.  Returns the [k, d] centres."""
    import ctypes as C
    from . import device as dev
    ctx = dev.get_context()
    P = np.ascontiguousarray(points, np.float64)
    n, d = P.shape
    rng = rng or np.random
    if distinct_start:
        # start from k rows that differ in VALUE where the sample has that many (sklearn relocates empty clusters instead)
        _, first = np.unique(P.round(12), axis=0, return_index=True)
        pool = first if first.size >= k else np.arange(n)
        rows = np.ascontiguousarray(rng.choice(pool, size=k, replace=False), np.int32)
    else:
        rows = np.ascontiguousarray(rng.choice(n, size=k, replace=False), np.int32)
    dP, dC = ctx.to_device(P), ctx.empty((k, d))
    iters = C.c_int(0)
    ctx._check(dev.lib().dcgp_kmeans(ctx.handle, dP.ptr, n, d, k, rows.ctypes.data, int(max_iter), float(tol * np.mean(np.var(P, axis=0))),
                                     dC.ptr, C.byref(iters)))
    return dC.numpy()


def _cluster_patches(NHWC_X, M, patch_size, dilation=1):
    """Inducing patches of PatchInducingFeatures.from_images (conv_gp/kernels.py:147-164): k-means centres of 100 * M patches cut at
    random from random images.  The sample is one vectorised gather (deepcgp_amd.models.draw_patches); Lloyd's iterations run
    on the device (``kmeans``), started from M DISTINCT patches -- on images with large constant regions (MNIST borders) a
    plain random start picks many identical rows, whose clusters then stay empty and leave duplicate inducing patches."""
    from .models import draw_patches
    sample = draw_patches(np.asarray(NHWC_X, np.float64), 100 * M, patch_size, dilation=dilation)
    return kmeans(sample, M, distinct_start=True)


def _greedy_kernel_args(base_kernel):
    """(type, variance, p1, p2, ARD lengthscales or None) of ``dcgp_greedy_variance`` for a base kernel: ``_describe()``'s codes."""
    if not isinstance(base_kernel, (RBF, ArcCosine, _Matern)):
        raise TypeError("greedy_variance: base_kernel must be an RBF, ArcCosine, Matern32 or Matern52, got %r" % (base_kernel,))
    kind, variance, p1, p2 = base_kernel._describe()
    ard = np.ascontiguousarray(base_kernel.lengthscales, np.float64) if getattr(base_kernel, "ARD", False) else None
    return int(kind), float(variance), float(p1), float(p2), ard


def _greedy_fill(rows, n_greedy, residual, k):
    """The k selected rows: the ``n_greedy`` greedy picks, then -- the greedy phase stalled at the floor -- the candidates of largest residual
    (ties: lower index) that are not picked yet and whose residual is not exactly 0 (a copy of a pick).  Fewer than k usable candidates:
    ValueError giving their number."""
    rows = np.asarray(rows[:n_greedy], np.int64)
    if n_greedy >= k:
        return rows[:k]
    residual = np.asarray(residual, np.float64)
    usable = residual > 0.0
    usable[rows] = False
    pool = np.flatnonzero(usable)
    if n_greedy + pool.size < k:
        raise ValueError("greedy_variance: only %d usable candidates (%d selected above the floor, %d more with a non-zero residual) for k = %d"
                         % (n_greedy + pool.size, n_greedy, pool.size, k))
    order = pool[np.argsort(-residual[pool], kind="stable")]      # pool ascends, the sort is stable: ties go to the lower index
    return np.concatenate([rows, order[:k - n_greedy]])


def greedy_variance_device(points, k, base_kernel, min_variance=JITTER, factor=False):
    """dcgp_greedy_variance as it is: {"rows" [k] (-1 behind n_greedy), "n_greedy", "trace" [k], "residual" [n], "factor" [k, n] or None}."""
    import ctypes as C
    P = np.ascontiguousarray(points, np.float64)
    if P.ndim != 2:
        raise ValueError("greedy_variance: points must be [n, d], got shape %r" % (P.shape,))
    n, d = P.shape
    k = int(k)
    if k < 1 or n < k:
        raise ValueError("greedy_variance: k = %d rows of n = %d candidates" % (k, n))
    if d != base_kernel.input_dim:
        raise ValueError("expected inputs of length %d, got %d" % (base_kernel.input_dim, d))
    kind, variance, p1, p2, ard = _greedy_kernel_args(base_kernel)
    ctx = dev.get_context()
    dP = ctx.to_device(P)
    dls = ctx.to_device(ard) if ard is not None else None
    rows, trace, resid = ctx.empty((k,), np.int32), ctx.empty((k,)), ctx.empty((n,))
    fac = ctx.empty((k, n)) if factor else None
    ng = C.c_int(0)
    ctx._check(dev.lib().dcgp_greedy_variance(ctx.handle, dP.ptr, n, d, k, kind, variance, p1, p2, dls.ptr if dls else None,
                                              float(min_variance), rows.ptr, trace.ptr, resid.ptr, fac.ptr if fac else None, C.byref(ng)))
    return {"rows": rows.numpy(), "n_greedy": ng.value, "trace": trace.numpy(), "residual": resid.numpy(),
            "factor": fac.numpy() if fac else None}


def greedy_variance(points, k, base_kernel, min_variance=JITTER, return_info=False):
    """Greedy conditional-variance selection (dcgp_greedy_variance; Burt, Rasmussen & van der Wilk 2020): ``k`` rows of ``points`` [n, d], each
    the candidate whose prior variance under ``base_kernel`` -- an ``RBF`` (scalar or ``ARD=True``), ``ArcCosine``, ``Matern32`` or
    ``Matern52`` -- conditioned on the rows chosen before it is largest.  The greedy phase stops at ``min_variance`` (default: the jitter
    K_uu receives anyway, below which it cannot tell candidates apart); the remaining rows are then taken in decreasing residual
    (``_greedy_fill``).  Returns Z [k, d]; ``return_info=True`` adds {"rows", "n_greedy", "trace", "residual"}: the chosen row indices, how
    many of them the greedy phase picked, the candidates' Nystrom trace tr(K_ff - Q_ff) after every greedy pick, the final residual."""
    P = np.ascontiguousarray(points, np.float64)
    out = greedy_variance_device(P, k, base_kernel, min_variance)
    chosen = _greedy_fill(out["rows"], out["n_greedy"], out["residual"], int(k))
    Z = P[chosen].copy()
    if return_info:
        return Z, {"rows": chosen, "n_greedy": out["n_greedy"], "trace": out["trace"], "residual": out["residual"]}
    return Z


def _greedy_patches(NHWC_X, M, patch_size, base_kernel, min_variance, dilation=1):
    """The greedy counterpart of ``_cluster_patches``: the same 100 * M patches (same generator, same order), M of them selected."""
    from .models import draw_patches
    sample = draw_patches(np.asarray(NHWC_X, np.float64), 100 * M, patch_size, dilation=dilation)
    return greedy_variance(sample, M, base_kernel, min_variance=min_variance, return_info=True)


def _rows_for(name, A, base_kernel):
    A = np.ascontiguousarray(A, np.float64)
    if A.ndim != 2 or A.shape[0] < 1:
        raise ValueError("%s must be [n, d] with n >= 1, got shape %r" % (name, A.shape))
    if A.shape[1] != base_kernel.input_dim:
        raise ValueError("expected inputs of length %d, got %d" % (base_kernel.input_dim, A.shape[1]))
    return A


def cross_gram(A, B, base_kernel):
    """k(a_i, b_j), [m, n], for A [m, d] and B [n, d] under ``base_kernel`` -- an ``RBF`` (scalar or ``ARD=True``), ``ArcCosine``, ``Matern32``
    or ``Matern52`` (dcgp_cross_gram).  Every entry is the kernel's off-diagonal form: no jitter, also where a row of B equals a row of A."""
    kind, variance, p1, p2, ard = _greedy_kernel_args(base_kernel)
    A, B = _rows_for("A", A, base_kernel), _rows_for("B", B, base_kernel)
    ctx = dev.get_context()
    dA, dB, out = ctx.to_device(A), ctx.to_device(B), ctx.empty((A.shape[0], B.shape[0]))
    dls = ctx.to_device(ard) if ard is not None else None
    ctx._check(dev.lib().dcgp_cross_gram(ctx.handle, dA.ptr, A.shape[0], dB.ptr, B.shape[0], A.shape[1], kind, variance, p1, p2,
                                         dls.ptr if dls else None, out.ptr))
    return out.numpy()


TRANSFER_FAILED = {1: "K(Z, Z)", 2: "K(Z_new, Z_new)"}      # dcgp_inducing_transfer's info[0]; 3 + r: S' of output r


def transfer_inducing(Z, Z_new, base_kernel, q_mu, q_sqrt, white=False, jitter=JITTER):
    """q(u) = N(q_mu, q_sqrt q_sqrt^T) at the inducing inputs ``Z`` [M, L] moved to ``Z_new`` [M', L]: the projection
    q'(u') = int p(u' | u) q(u) du under ``base_kernel``'s prior (dcgp_inducing_transfer).  q_mu [M, R], q_sqrt [R, M, M] -> (q_mu' [M', R],
    q_sqrt' [R, M', M']), lower triangular with exact zeros above a positive diagonal.  ``white``: both in whitened coordinates.

    u and u' carry independent jitter, so the KL to the prior never rises (data processing), chol succeeds however small q_sqrt is -- and a
    transfer onto an identical Z is a projection, not the identity.  A matrix that is not positive definite raises ``NotPositiveDefinite``
    (``.which``: 1 K, 2 K_new, 3 + r the new covariance of output r); nothing is returned then and no device output was written."""
    import ctypes as C
    kind, variance, p1, p2, ard = _greedy_kernel_args(base_kernel)
    Z, Zn = _rows_for("Z", Z, base_kernel), _rows_for("Z_new", Z_new, base_kernel)
    q_mu, q_sqrt = np.ascontiguousarray(q_mu, np.float64), np.ascontiguousarray(q_sqrt, np.float64)
    M, Mn = Z.shape[0], Zn.shape[0]
    if q_mu.ndim != 2 or q_mu.shape[0] != M:
        raise ValueError("q_mu must be [M, R] with M = %d, got shape %r" % (M, q_mu.shape))
    R = q_mu.shape[1]
    if q_sqrt.shape != (R, M, M):
        raise ValueError("q_sqrt must be [R, M, M] = %r, got shape %r" % ((R, M, M), q_sqrt.shape))
    ctx = dev.get_context()
    dZ, dZn, dm, dS = ctx.to_device(Z), ctx.to_device(Zn), ctx.to_device(q_mu), ctx.to_device(q_sqrt)
    dls = ctx.to_device(ard) if ard is not None else None
    om, oS = ctx.empty((Mn, R)), ctx.empty((R, Mn, Mn))
    info = (C.c_int * 2)(0, 0)
    rc = dev.lib().dcgp_inducing_transfer(ctx.handle, dZ.ptr, M, dZn.ptr, Mn, Z.shape[1], kind, variance, p1, p2, dls.ptr if dls else None,
                                          float(jitter), int(bool(white)), dm.ptr, dS.ptr, R, om.ptr, oS.ptr, info)
    try:
        ctx._check(rc, C.c_int(info[1]))
    except dev.NotPositiveDefinite as e:
        e.which = info[0]
        raise
    return om.numpy(), oS.numpy()


class InducingPoints:
    """gpflow.features.InducingPoints(Z) -- the dense head's feature (conv_gp/models.py:168)."""

    def __init__(self, Z):
        self.Z = np.array(Z, np.float64)

    def __len__(self):
        return self.Z.shape[0]


class PatchInducingFeatures:
    """conv_gp/kernels.py:166-170 (InducingPointsBase: ``Z`` and ``len``)."""

    def __init__(self, Z):
        self.Z = np.array(Z, np.float64)

    def __len__(self):
        return self.Z.shape[0]

    @classmethod
    def from_images(cls, NHWC_X, M, patch_size, method="kmeans", base_kernel=None, min_variance=JITTER, dilation=1):
        """``method="kmeans"``: the reference's recipe, centres of 100 M random patches.  ``"greedy"``: M of the same patches by conditional
        variance under ``base_kernel`` (``greedy_variance``); the selection's info stays on the feature as ``init_info``.  ``dilation``: the
        candidates are the layer's dilated windows (taps that many pixels apart)."""
        if method == "kmeans":
            return cls(_cluster_patches(NHWC_X, M, patch_size, dilation))
        if method != "greedy":
            raise ValueError("from_images: method must be 'kmeans' or 'greedy', got %r" % (method,))
        if base_kernel is None:
            raise ValueError("from_images: method 'greedy' needs the layer's base_kernel")
        Z, info = _greedy_patches(NHWC_X, M, patch_size, base_kernel, min_variance, dilation)
        feature = cls(Z)
        feature.init_info = info
        return feature


def Kuu(feature, kern, jitter=0.0):
    """dispatch at conv_gp/kernels.py:172-174 (patch features); gpflow's default for InducingPoints + a plain kernel."""
    return (kern.base_kernel if hasattr(kern, "base_kernel") else kern)._gram(feature.Z, jitter)


def Kuf(feature, kern, Xnew):
    """dispatch at conv_gp/kernels.py:176-178."""
    return kern.Kzx(feature.Z, Xnew)

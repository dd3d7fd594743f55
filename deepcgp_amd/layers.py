"""Layers of the conv-GP path -- same surface as /root/reference/conv_gp/layers.py plus the two layer
classes the reference takes from doubly_stochastic_dgp (``Layer``, ``SVGP_Layer``), backed by HIP."""
import ctypes as C

import numpy as np

from . import device as dev
from .conditionals import conditional
from .kernels import JITTER, RBF, Kuu as _Kuu, Kuf as _Kuf
from .views import FullView


def _potrf(A):
    ctx = dev.get_context()
    A = np.ascontiguousarray(A, np.float64)
    M = A.shape[0]
    dA, info = ctx.to_device(A), C.c_int(0)
    ctx._check(dev.lib().dcgp_potrf_lower(ctx.handle, dA.ptr, M, C.byref(info)), info)
    return dA.numpy()


def gauss_kl(q_mu, q_sqrt, K=None):
    """gpflow.kullback_leiblers.gauss_kl (call sites conv_gp/layers.py:145,147)."""
    ctx = dev.get_context()
    q_mu = np.ascontiguousarray(q_mu, np.float64)
    M, R = q_mu.shape
    dmu, dsq = ctx.to_device(q_mu), ctx.to_device(q_sqrt)
    dK = ctx.to_device(K) if K is not None else None
    out, info = C.c_double(0.0), C.c_int(0)
    rc = dev.lib().dcgp_gauss_kl(ctx.handle, dmu.ptr, dsq.ptr, dK.ptr if dK else None, M, R, C.byref(out), C.byref(info))
    ctx._check(rc, info)
    return out.value


def reparameterize(mean, var, z, full_cov=False):
    """doubly_stochastic_dgp.utils.reparameterize: mean + z * sqrt(var + jitter); full_cov=True: mean S x N x D, var S x N x N x D,
    per (sample, output) mean + chol(var + jitter I) z (off the training path: one device factorisation per matrix)."""
    if var is None:
        return mean
    if full_cov:
        mean, var, z = (np.asarray(a, np.float64) for a in (mean, var, z))
        S, N, D = mean.shape
        out = np.empty_like(mean)
        for s_ in range(S):
            for d_ in range(D):
                out[s_, :, d_] = mean[s_, :, d_] + _potrf(var[s_, :, :, d_] + JITTER * np.eye(N)) @ z[s_, :, d_]
        return out
    ctx = dev.get_context()
    mean = np.ascontiguousarray(mean, np.float64)
    dm, dv, dz = ctx.to_device(mean), ctx.to_device(var), ctx.to_device(z)
    out = ctx.empty(mean.shape)
    ctx._check(dev.lib().dcgp_reparam(ctx.handle, dm.ptr, dv.ptr, dz.ptr, mean.size, JITTER, out.ptr))
    return out.numpy()


def reparameterize_full_cov(mean, var, z):
    """reparameterize(mean, var, z, full_cov=True) for all S x D matrices in one launch (dcgp_reparam_full_cov): mean, z S x N x D,
    var S x N x N x D.  N > 128 (a factor no longer fits one workgroup's LDS) takes the host loop of ``reparameterize``."""
    mean, var, z = (np.ascontiguousarray(a, np.float64) for a in (mean, var, z))
    S, N, D = mean.shape
    if var.shape != (S, N, N, D) or z.shape != (S, N, D):
        raise ValueError("expected var %s and z %s, got %s and %s" % ((S, N, N, D), (S, N, D), var.shape, z.shape))
    if S == 0 or N == 0 or D == 0:
        return mean.copy()
    if N > 128:
        return reparameterize(mean, var, z, full_cov=True)
    ctx = dev.get_context()
    dm, dv, dz, out, info = ctx.to_device(mean), ctx.to_device(var), ctx.to_device(z), ctx.empty((S, N, D)), C.c_int(0)
    ctx._check(dev.lib().dcgp_reparam_full_cov(ctx.handle, dm.ptr, dv.ptr, dz.ptr, S, N, D, JITTER, out.ptr, C.byref(info)), info)
    return out.numpy()


class MultiOutputConvKernel:
    """conv_gp/layers.py:12-50."""

    def __init__(self, base_kernel, input_dim, patch_count):
        self.base_kernel = base_kernel
        self.input_dim = input_dim
        self.patch_count = patch_count

    def Kuu(self, ML_Z):
        return self.base_kernel._gram(ML_Z, JITTER)

    def Kuf(self, ML_Z, PNL_patches):
        """patch_count x M x N.  PNL_patches may be the P x N x L array of the reference, or an
        ``(NHWC_X, view)`` pair -- the latter is the fused form that never materialises patches."""
        ctx = dev.get_context()
        Z = np.ascontiguousarray(ML_Z, np.float64)
        M = Z.shape[0]
        if isinstance(PNL_patches, tuple):
            X, view = PNL_patches
            X = np.ascontiguousarray(view.pad(X) if hasattr(view, "pad") else X, np.float64)
            N, H, W, Cc = X.shape
            f, s = view.filter_size, view.stride
        else:
            # every patch is a 1x1 "image" with L channels, filter 1: same sweep, no gather
            PNL = np.ascontiguousarray(PNL_patches, np.float64)
            P, N, L = PNL.shape
            X = np.ascontiguousarray(np.transpose(PNL, (1, 0, 2))).reshape(N, P, 1, L)
            H, W, Cc, f, s = P, 1, L, 1, 1
        P = ((H - f) // s + 1) * ((W - f) // s + 1)
        if N == 0:
            return np.zeros((P, M, 0))
        dX, dZ, out = ctx.to_device(X), ctx.to_device(Z), ctx.empty((P, M, N))
        self.base_kernel._kuf(ctx, dX, N, H, W, Cc, f, s, dZ, M, out, 0)
        return out.numpy()

    def Kff(self, PNL_patches):
        """P x N x N auto-covariance of the inputs, patch by patch (conv_gp/layers.py:34-41; full_cov=True only)."""
        PNL = np.ascontiguousarray(PNL_patches, np.float64)
        return np.stack([self.base_kernel._gram(PNL[p], 0.0) for p in range(PNL.shape[0])]) if PNL.shape[0] else np.zeros((0,) + PNL.shape[1:2] * 2)

    def Kdiag(self, PNL_patches):
        P, N = np.shape(PNL_patches)[:2]
        return np.full((P, N), self.base_kernel.variance)


def mixing_matrix(kind, G, R, seed=0):
    """A mixed ConvLayer's W [G, R]: ``"identity"`` (needs G == R), ``"random"`` (entries N(0, 1/G) from ``RandomState(seed)``: a map's
    variance is about a latent's), or an array [G, R] taken as it is."""
    G, R = int(G), int(R)
    if G < 1 or R < 1:
        raise ValueError("mixing_matrix: G and R must be >= 1, got %d and %d" % (G, R))
    if isinstance(kind, str):
        if kind == "identity":
            if G != R:
                raise ValueError("mixing_matrix('identity') needs G == R, got %d and %d" % (G, R))
            return np.eye(G)
        if kind == "random":
            return np.random.RandomState(int(seed)).standard_normal((G, R)) / np.sqrt(G)
        raise ValueError("mixing_matrix: kind %r, expected 'identity', 'random' or an array [G, R]" % (kind,))
    W = np.array(kind, np.float64)
    if W.shape != (G, R):
        raise ValueError("mixing_matrix: the array must be [%d, %d], got %r" % (G, R, W.shape))
    return W


def mix_forward(W, u, gm, gv):
    """(sample, mean, var) [K, R] of latent (u, gm, gv) [K, G] through W [G, R] on the device (dcgp_mix_forward); an input may be None, its
    output is then None."""
    ctx = dev.get_context()
    W = np.ascontiguousarray(W, np.float64)
    G, R = W.shape
    first = next(a for a in (u, gm, gv) if a is not None)
    cols = int(np.size(first)) // G
    ins = [None if a is None else ctx.to_device(np.reshape(np.asarray(a, np.float64), (cols, G))) for a in (u, gm, gv)]
    outs = [None if a is None else ctx.empty((cols, R)) for a in ins]
    dW = ctx.to_device(W)
    if cols:
        ctx._check(dev.lib().dcgp_mix_forward(ctx.handle, dW.ptr, G, R, *[a.ptr if a else None for a in ins], 0, cols, 1, 0, 0,
                                              *[a.ptr if a else None for a in outs]))
    shape = first.shape[:-1] + (first.shape[-1] // G * R,)
    return tuple(None if a is None else a.numpy().reshape(shape) for a in outs)


class Layer:
    """doubly_stochastic_dgp.layers.Layer: conditional_SND / sample_from_conditional on top of a
    subclass's conditional_ND (subclassed at conv_gp/layers.py:52)."""

    num_outputs = None

    def conditional_ND(self, X, full_cov=False):
        raise NotImplementedError

    def KL(self):
        return 0.0

    def conditional_SND(self, X, full_cov=False):
        """mean S x N x D and var S x N x D; full_cov=True: the samples one by one through conditional_ND(full_cov=True)
        (the reference's tf.map_fn branch), var S x N x N x D."""
        X = np.asarray(X, np.float64)
        S, N, D = X.shape
        if full_cov:
            mv = [self.conditional_ND(X[s_], full_cov=True) for s_ in range(S)]
            return np.stack([m for m, _ in mv]), np.stack([v for _, v in mv])
        mean, var = self.conditional_ND(X.reshape(S * N, D))
        return mean.reshape(S, N, self.num_outputs), var.reshape(S, N, self.num_outputs)

    def sample_from_conditional(self, X, z=None, full_cov=False):
        mean, var = self.conditional_SND(X, full_cov=full_cov)
        if z is None:
            z = np.random.standard_normal(mean.shape)
        samples = reparameterize(mean, var, np.reshape(z, mean.shape), full_cov=full_cov)
        return samples, mean, var


class ConvLayer(Layer):
    """conv_gp/layers.py:52-161.  ``mean_function``: a ``deepcgp_amd.mean_functions`` object as the reference builds them
    (``Conv2dMean(filter_size, feature_maps_in, feature_maps_out, stride)`` or ``Zero()``, conv_gp/models.py:95-99), any callable
    on the NHWC image returning N x num_outputs (or N x H' x W' x gp_count) values, or the aliases None / 'zero' / 'conv2d'.
    A ``Conv2dMean`` with the filter its constructor built is added inside the layer's own launch; a ``LinearConv2dMean`` (any filter,
    optionally trained) lives on the device model and is added behind the layer's launch (``filter_mean``; csrc/conv_mean.hip); any other
    callable through its ``__call__`` (the model-level one-call ELBO path takes the first two only).

    ``mixing``: None, or W [G, R] with G = ``gp_count``: the layer holds G latent GPs and emits R feature maps, a trainable linear mix of them
    (gpflow's SharedMixed... / LinearCoregionalization; csrc/mix.hip).  Sample, then mix: ``sample = (gm + z sqrt(gv + jitter)) W + m(x)`` with
    ``z`` of P * G values a row; ``conditional_ND`` returns the marginals ``gm W + m(x)``, ``gv W^2``.  The mean function then has
    ``feature_maps_out = R`` maps (a ``Conv2dMean`` runs as the frozen centre-pixel filter), the KL term stays the G latent GPs'."""

    def __init__(self, base_kernel, mean_function, feature=None, view=None, white=False, gp_count=1,
                 q_mu=None, q_sqrt=None, mixing=None, **kwargs):
        self.base_kernel = base_kernel
        self.view = view
        self.feature_maps_in = self.view.feature_maps
        self.gp_count = int(gp_count)
        self.patch_count = self.view.patch_count
        self.patch_length = self.view.patch_length
        self.mixing = None
        if mixing is not None:
            W = np.array(mixing, np.float64)
            if W.ndim != 2 or W.shape[0] != self.gp_count or W.shape[1] < 1:
                raise ValueError("mixing must be [gp_count, R] = [%d, R >= 1], got shape %r" % (self.gp_count, W.shape))
            self.mixing = W
        self.feature_maps_out = self.gp_count if self.mixing is None else int(self.mixing.shape[1])
        self.num_outputs = self.patch_count * self.feature_maps_out
        self.num_latent_outputs = self.patch_count * self.gp_count
        self.conv_kernel = MultiOutputConvKernel(base_kernel, int(np.prod(view.input_size)) * view.feature_maps,
                                                 patch_count=self.patch_count)
        self.white = bool(white)
        self.feature = feature
        self.num_inducing = len(feature)
        # the KL prior is built on the *initial* Z (conv_gp/layers.py:149-152)
        self.Z_prior = np.array(feature.Z, np.float64)
        if q_mu is None:
            q_mu = self._initial_q_mu()
        self.q_mu = np.array(q_mu, np.float64)
        if q_sqrt is None:
            if not self.white:
                q_sqrt = self._init_q_S()
            else:
                q_sqrt = np.tile(np.eye(self.num_inducing)[None, :, :], [self.gp_count, 1, 1])
        self.q_sqrt = np.array(q_sqrt, np.float64)
        self.mean_function = mean_function
        self.filter_mean                     # (a LinearConv2dMean of another geometry than the view's raises here)
        self._build_prior_cholesky()

    @property
    def filter_mean(self):
        """The ``LinearConv2dMean`` of this layer, or None: the mean the device model evaluates, differentiates and trains through its
        filter (csrc/conv_mean.hip).  Its geometry must be the view's: same filter size, stride, input channels, and gp_count maps."""
        mf = self.mean_function
        if not getattr(mf, 'is_linear_conv2d_mean', False):
            return None
        v = self.view
        have = (mf.filter_size, mf.stride, mf.feature_maps_in, mf.feature_maps_out)
        want = (v.filter_size, v.stride, v.feature_maps, self.feature_maps_out)
        if have != want:
            raise ValueError("LinearConv2dMean(filter_size, feature_maps_in, feature_maps_out, stride) = %r does not match the layer's view "
                             "and gp_count %r" % ((have[0], have[2], have[3], have[1]), (want[0], want[2], want[3], want[1])))
        return mf

    @property
    def identity_mean(self):
        """The mean the layer kernels add themselves: Conv2dMean's centre pixel of input channel 0 into output map 0
        (conv_gp/mean_functions.py:28-41), geometry equal to the view's.  Not on a mixed layer: see ``centre_mean``."""
        return self.mixing is None and self._conv2d_initial()

    @property
    def centre_mean(self):
        """A mixed layer's Conv2dMean: the same centre pixel into output map 0 of the R maps, which the layer's own launch cannot add (it
        writes the latent maps): the device model runs it as the frozen ``centre0`` filter (csrc/conv_mean.hip)."""
        return self.mixing is not None and self._conv2d_initial()

    def _conv2d_initial(self):
        mf = self.mean_function
        if isinstance(mf, str):
            return mf == 'conv2d'
        if mf is None or not getattr(mf, 'is_conv2d_mean', False):
            return False
        if hasattr(mf, 'has_initial_filter') and not mf.has_initial_filter():
            return False
        v = self.view
        return (getattr(mf, 'filter_size', v.filter_size) == v.filter_size and getattr(mf, 'stride', v.stride) == v.stride and
                getattr(mf, 'feature_maps_in', v.feature_maps) == v.feature_maps and
                getattr(mf, 'feature_maps_out', self.feature_maps_out) == self.feature_maps_out)

    @property
    def generic_mean(self):
        """A callable mean function the kernels do not add themselves (``mean + self.mean_function(mean_view)``, layers.py:133-134)."""
        mf = self.mean_function
        from .mean_functions import Zero
        if mf is None or isinstance(mf, (str, Zero)) or self._conv2d_initial() or self.filter_mean is not None:
            if isinstance(mf, str) and mf not in ('zero', 'conv2d'):
                raise ValueError("mean_function %r: expected a callable, None, 'zero' or 'conv2d'" % (mf,))
            return None
        if not callable(mf):
            raise ValueError("mean_function must be callable, None, 'zero' or 'conv2d'")
        return mf

    def _generic_mean_value(self, X4):
        mf = self.generic_mean
        N = X4.shape[0]
        if mf is None and self.filter_mean is not None:      # the layer's own window: the filter sees the zero-padded image
            return np.asarray(self.filter_mean(self.view.pad(X4)), np.float64).reshape(N, self.num_outputs)
        if mf is None and self.centre_mean:
            v = self.view
            c0, st = v.filter_size // 2, v.stride
            val = np.zeros((N, v.patch_count, self.feature_maps_out))
            val[:, :, 0] = v.pad(X4)[:, c0:c0 + (v.out_image_height - 1) * st + 1:st, c0:c0 + (v.out_image_width - 1) * st + 1:st, 0].reshape(N, v.patch_count)
            return val.reshape(N, self.num_outputs)
        if mf is None:
            return None
        val = np.asarray(mf(self.view.mean_view(X4, None)), np.float64)
        if val.size != N * self.num_outputs:
            raise ValueError("mean_function returned %s values for %d x %d outputs" % (val.shape, N, self.num_outputs))
        return val.reshape(N, self.num_outputs)

    def conditional_ND(self, ND_X, full_cov=False):
        """mean, var of q(f | m, S), each N x (patch_count * gp_count), HWC column order."""
        if full_cov:
            if self.mixing is not None:
                raise NotImplementedError("full_cov=True through a mixed layer (mixing W [%d, %d]) is not provided" % self.mixing.shape)
            return self._conditional_full_cov(ND_X)
        return self._forward(ND_X, None)[1:]

    def _refuse_dilated_full_cov(self):
        d = getattr(self.view, "dilation", 1)
        if d > 1:
            raise NotImplementedError("full_cov=True through a dilated layer (dilation %d) is not provided" % d)

    def _conditional_full_cov(self, ND_X):
        """conv_gp/layers.py:114-126 with full_cov=True: mean N x num_outputs, var N x N x num_outputs (per output = (patch, gp)
        an N x N covariance over the inputs; conditionals._conditional_full_cov documents the per-patch reading).  Off the training
        path (predict_f_full_cov-style calls): composed from the operator-level device calls."""
        self._refuse_dilated_full_cov()
        ND_X = np.ascontiguousarray(ND_X, np.float64)
        N, v = ND_X.shape[0], self.view
        X4 = ND_X.reshape(N, v.input_size[0], v.input_size[1], self.feature_maps_in)
        PNL = v.extract_patches_PNL(X4)
        mean, var = conditional(self.conv_kernel.Kuf(self.feature.Z, (X4, v)), self.conv_kernel.Kuu(self.feature.Z), self.conv_kernel.Kff(PNL),
                                self.q_mu, full_cov=True, q_sqrt=self.q_sqrt, white=self.white)      # N x P x R, R x P x N x N
        var = np.transpose(var, (2, 3, 1, 0)).reshape(N, N, self.num_outputs)
        mean = mean.reshape(N, self.num_outputs)
        if self.identity_mean:
            f, st = v.filter_size, v.stride
            Ho, Wo = v.out_image_height, v.out_image_width
            c0 = f // 2
            centre = v.pad(X4)[:, c0:c0 + (Ho - 1) * st + 1:st, c0:c0 + (Wo - 1) * st + 1:st, 0]
            mean = mean.copy()
            mean.reshape(N, v.patch_count, self.gp_count)[:, :, 0] += centre.reshape(N, v.patch_count)
        extra = self._generic_mean_value(X4)
        if extra is not None:
            mean = mean + extra
        return mean, var

    def _forward(self, ND_X, z):
        """(sample or None, mean, var), each N x num_outputs."""
        if getattr(self.view, "dilation", 1) > 1:
            return self._forward_dilated(ND_X, z)
        if self.mixing is None:
            return self._forward_gp(ND_X, z)
        # a mixed layer: the G latent GPs' conditional, the sample in the latent space, then the three mixes in one operator call (csrc/mix.hip)
        ND_X = np.ascontiguousarray(ND_X, np.float64)
        N, v = ND_X.shape[0], self.view
        _, gm, gv = self._forward_gp(ND_X, None)
        if N == 0:
            return (None if z is None else np.zeros((0, self.num_outputs))), np.zeros((0, self.num_outputs)), np.zeros((0, self.num_outputs))
        u = None if z is None else reparameterize(gm, gv, np.reshape(z, gm.shape))
        smp, mean, var = mix_forward(self.mixing, u, gm, gv)
        extra = self._generic_mean_value(ND_X.reshape(N, v.input_size[0], v.input_size[1], self.feature_maps_in))
        if extra is not None:
            mean = mean + extra
            smp = None if smp is None else smp + extra
        return smp, mean, var

    def _phase_twin(self):
        """This layer on the phase sub-images of a dilated view: the same parameters, kernel and mean function on an undilated, unpadded
        view of ``view.phase_size`` (a shallow copy; the centre tap of a sub-image patch is the centre tap of the dilated window)."""
        import copy
        from .views import FullView
        v = self.view
        twin = copy.copy(self)
        twin.view = FullView(v.phase_size, v.filter_size, v.feature_maps, 1)
        twin.patch_count = twin.view.patch_count
        twin.num_outputs = twin.patch_count * self.feature_maps_out
        twin.num_latent_outputs = twin.patch_count * self.gp_count
        twin.conv_kernel = MultiOutputConvKernel(self.base_kernel, int(np.prod(v.phase_size)) * v.feature_maps, patch_count=twin.patch_count)
        return twin

    def _forward_dilated(self, ND_X, z):
        """``_forward`` through a dilated view: pad, split into the d^2 phase sub-images on the host (``view.split``), the undilated layer
        on those (``_phase_twin``), and the outputs merged back into image order; a patch that touched the fill is dropped.  Noise arrives
        in image order [N, P * gp_count] and is split the same way."""
        v = self.view
        d, f = v.dilation, v.filter_size
        ND_X = np.ascontiguousarray(ND_X, np.float64)
        N = ND_X.shape[0]
        if ND_X.shape[1] != v.input_size[0] * v.input_size[1] * self.feature_maps_in:
            raise ValueError("expected N x %d inputs, got %s" % (v.input_size[0] * v.input_size[1] * self.feature_maps_in, ND_X.shape))
        Ho, Wo = v.out_image_height, v.out_image_width
        if N == 0:
            return (None if z is None else np.zeros((0, self.num_outputs))), np.zeros((0, self.num_outputs)), np.zeros((0, self.num_outputs))
        Xs = v.split(v.pad(ND_X.reshape(N, v.input_size[0], v.input_size[1], self.feature_maps_in)))
        zs = None if z is None else v.split(np.reshape(z, (N, Ho, Wo, self.gp_count))).reshape(N * d * d, -1)
        smp, mean, var = self._phase_twin()._forward(Xs.reshape(N * d * d, -1), zs)
        Hq, Wq = v.phase_size[0] - f + 1, v.phase_size[1] - f + 1

        def back(a):
            return None if a is None else v.merge(a.reshape(N * d * d, Hq, Wq, self.feature_maps_out), Ho, Wo).reshape(N, self.num_outputs)
        return back(smp), back(mean), back(var)

    def _forward_gp(self, ND_X, z):
        """The layer's gp_count GPs: (sample or None, mean, var), each N x num_latent_outputs -- with the mean function unless the layer is mixed."""
        ctx = dev.get_context()
        ND_X = np.ascontiguousarray(ND_X, np.float64)
        N = ND_X.shape[0]
        v = self.view
        H, W = v.input_size[0], v.input_size[1]
        if ND_X.shape[1] != H * W * self.feature_maps_in:
            raise ValueError("expected N x %d inputs, got %s" % (H * W * self.feature_maps_in, ND_X.shape))
        D = self.num_latent_outputs
        if N == 0:
            return np.zeros((0, D)), np.zeros((0, D)), np.zeros((0, D))
        if not isinstance(self.base_kernel, RBF) or self.base_kernel.ARD:    # (ARD: the one-call operator takes one lengthscale)
            return self._forward_composed(ND_X, z)
        Hp, Wp = v.padded_size
        dX, dZ = ctx.to_device(v.pad(ND_X.reshape(N, H, W, self.feature_maps_in))), ctx.to_device(self.feature.Z)
        dmu, dsq = ctx.to_device(self.q_mu), ctx.to_device(self.q_sqrt)
        dz = ctx.to_device(np.reshape(z, (N, D))) if z is not None else None
        ds = ctx.empty((N, D)) if z is not None else None
        dm, dv = ctx.empty((N, D)), ctx.empty((N, D))
        info = C.c_int(0)
        rc = dev.lib().dcgp_conv_layer_forward(
            ctx.handle, dX.ptr, N, Hp, Wp, self.feature_maps_in, v.filter_size, v.stride, dZ.ptr,
            self.num_inducing, self.gp_count, self.base_kernel.variance, self.base_kernel.lengthscales,
            dmu.ptr, dsq.ptr, int(self.white), int(self.identity_mean), dz.ptr if dz else None, JITTER,
            ds.ptr if ds else None, dm.ptr, dv.ptr, C.byref(info))
        ctx._check(rc, info)
        smp, mean, var = (ds.numpy() if ds else None), dm.numpy(), dv.numpy()
        extra = None if self.mixing is not None else self._generic_mean_value(ND_X.reshape(N, H, W, self.feature_maps_in))
        if extra is not None:
            mean = mean + extra
            smp = None if smp is None else smp + extra
        return smp, mean, var

    def _forward_composed(self, ND_X, z):
        """conditional_ND as the reference composes it (conv_gp/layers.py:108-135) from the operator-level calls --
        Kuu, fused patches + Kuf, Kdiag, conditional -- for base kernels the one-call layer operator has no
        signature for (ArcCosine, Matern32, Matern52); the model path (dcgp_elbo_forward) handles them natively."""
        N = ND_X.shape[0]
        v = self.view
        X4 = ND_X.reshape(N, v.input_size[0], v.input_size[1], self.feature_maps_in)
        MM_Kuu = self.conv_kernel.Kuu(self.feature.Z)
        PMN_Kuf = self.conv_kernel.Kuf(self.feature.Z, (X4, v))
        Knn = np.full((v.patch_count, N), self.base_kernel.variance)
        mean, var = conditional(PMN_Kuf, MM_Kuu, Knn, self.q_mu, q_sqrt=self.q_sqrt, white=self.white)   # N x P x R, R x P x N
        mean = mean.reshape(N, self.num_latent_outputs)
        var = np.transpose(var, (2, 1, 0)).reshape(N, self.num_latent_outputs)
        if self.identity_mean:
            f, st = v.filter_size, v.stride
            Ho, Wo = v.out_image_height, v.out_image_width
            c0 = f // 2
            centre = v.pad(X4)[:, c0:c0 + (Ho - 1) * st + 1:st, c0:c0 + (Wo - 1) * st + 1:st, 0]
            mean = mean.copy()
            mean.reshape(N, v.patch_count, self.gp_count)[:, :, 0] += centre.reshape(N, v.patch_count)
        extra = None if self.mixing is not None else self._generic_mean_value(X4)
        if extra is not None:
            mean = mean + extra
        sample = None if z is None else reparameterize(mean, var, np.reshape(z, mean.shape))
        return sample, mean, var

    def sample_from_conditional(self, X, z=None, full_cov=False):
        if full_cov:   # (the call shape of conv_gp/utils/tensorboard.py:73-81) off the one-launch path: Layer's generic route
            return Layer.sample_from_conditional(self, X, z=z, full_cov=True)
        X = np.asarray(X, np.float64)
        S, N, D = X.shape
        Dz = self.num_latent_outputs      # noise per row: one value per (patch, GP)
        if z is None:
            z = np.random.standard_normal((S, N, Dz))
        if np.size(z) != S * N * Dz:
            raise ValueError("z has %d values, the layer draws S x N x %d = %d" % (np.size(z), Dz, S * N * Dz))
        s, m, v = self._forward(X.reshape(S * N, D), np.reshape(z, (S * N, Dz)))
        shape = (S, N, self.num_outputs)
        return s.reshape(shape), m.reshape(shape), v.reshape(shape)

    def KL(self):
        """KL[q(u) || p(u)] summed over the gp_count GPs (conv_gp/layers.py:137-147)."""
        if self.white:
            return gauss_kl(self.q_mu, self.q_sqrt, K=None)
        return gauss_kl(self.q_mu, self.q_sqrt, self.conv_kernel.Kuu(self.Z_prior))

    def _build_prior_cholesky(self):
        self.MM_Ku_prior = self.conv_kernel.Kuu(self.Z_prior)

    def _init_q_S(self):
        MM_Lu = _potrf(self.conv_kernel.Kuu(self.feature.Z))
        return np.tile(MM_Lu[None, :, :], [self.gp_count, 1, 1])

    def _initial_q_mu(self):
        return np.zeros((self.num_inducing, self.gp_count))


class SVGP_Layer(Layer):
    """doubly_stochastic_dgp.layers.SVGP_Layer in the fork's signature (conv_gp/models.py:192-198)."""

    def __init__(self, kern, num_outputs, feature=None, mean_function=None, white=False, q_mu=None, q_sqrt=None):
        self.kern = kern
        self.num_outputs = int(num_outputs)
        self.feature = feature
        self.num_inducing = len(feature)
        self.white = bool(white)
        self.mean_function = mean_function
        if q_mu is None:
            q_mu = np.zeros((self.num_inducing, self.num_outputs))
        self.q_mu = np.array(q_mu, np.float64)
        if q_sqrt is None:
            if self.white:
                q_sqrt = np.tile(np.eye(self.num_inducing)[None], [self.num_outputs, 1, 1])
            else:
                Lu = _potrf(_Kuu(self.feature, self.kern, jitter=JITTER))
                q_sqrt = np.tile(Lu[None], [self.num_outputs, 1, 1])
        self.q_sqrt = np.array(q_sqrt, np.float64)

    def conditional_ND(self, X, full_cov=False):
        if full_cov:
            mean, var = self._conditional_full_cov(np.asarray(X, np.float64)[None])
            return mean[0], var[0]
        ctx = dev.get_context()
        X = np.ascontiguousarray(X, np.float64)
        N, M, R = X.shape[0], self.num_inducing, self.num_outputs
        if N == 0:
            return np.zeros((0, R)), np.zeros((0, R))
        Ku = _Kuu(self.feature, self.kern, jitter=JITTER)
        Kuf = _Kuf(self.feature, self.kern, X)
        Kdiag = self.kern.Kdiag(X)
        d = [ctx.to_device(a) for a in (Kuf, Ku, Kdiag, self.q_mu, self.q_sqrt)]
        mean, var, info = ctx.empty((N, R)), ctx.empty((N, R)), C.c_int(0)
        rc = dev.lib().dcgp_svgp_conditional(ctx.handle, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr,
                                             int(self.white), M, N, R, mean.ptr, var.ptr, C.byref(info))
        ctx._check(rc, info)
        return mean.numpy(), var.numpy()

    def patch_contributions(self, X):
        """[N, P, R]: the posterior mean of ``conditional_ND(X)`` split over the P patches of each image (the mean function of a
        head is Zero, so ``patch_contributions(X).sum(1) == conditional_ND(X)[0]``).  beta = L^-T q_mu (white) or Kuu^-1 q_mu from
        the operator entry points, then ``kern.patch_mean``.  Patch heads only."""
        if not hasattr(self.kern, "patch_mean"):
            raise TypeError("patch_contributions needs a patch kernel (ConvKernel / AdditivePatchKernel); a dense head has no patches")
        M, R = self.num_inducing, self.num_outputs
        X = np.ascontiguousarray(X, np.float64)
        if X.shape[0] == 0:
            return np.zeros((0, self.kern.patch_count, R))
        ctx = dev.get_context()
        Lm = _potrf(_Kuu(self.feature, self.kern, jitter=JITTER))
        dL, dLinv = ctx.to_device(Lm), ctx.empty((M, M))
        ctx._check(dev.lib().dcgp_trtri_lower(ctx.handle, dL.ptr, M, dLinv.ptr))
        da = ctx.to_device(self.q_mu)
        if not self.white:
            dq, da = da, ctx.empty((M, R))
            ctx.gemm(dLinv, (M, 1, 0), dq, (R, 1, 0), da, R, M * R, M, R, M)        # inv(L) q_mu
        dbeta = ctx.empty((M, R))
        ctx.gemm(dLinv, (1, M, 0), da, (R, 1, 0), dbeta, R, M * R, M, R, M)         # inv(L)^T ...
        return self.kern.patch_mean(self.feature.Z, X, dbeta.numpy())

    def _conditional_full_cov(self, X):
        """conditional_ND(full_cov=True) of B input sets at once: X [B, N, D] -> mean [B, N, R], var [B, N, N, R] (DS-DGP's
        [N, N, R] layout per set).  Patch heads: Kff by the image-pair kernel, one launch for all B; the dense RBF-ARD head: RBF.K.
        The conditional itself is one device call (dcgp_svgp_conditional_full_cov)."""
        X = np.ascontiguousarray(X, np.float64)
        B, N = X.shape[:2]
        M, R = self.num_inducing, self.num_outputs
        if B == 0 or N == 0:
            return np.zeros((B, N, R)), np.zeros((B, N, N, R))
        Xf = X.reshape(B * N, -1)
        Ku = _Kuu(self.feature, self.kern, jitter=JITTER)
        Kuf = np.ascontiguousarray(np.transpose(_Kuf(self.feature, self.kern, Xf).reshape(M, B, N), (1, 0, 2)))
        if hasattr(self.kern, "_K_batched"):
            X4 = self.kern._reshape_X(Xf)
            Kff = self.kern._K_batched(X4.reshape((B, N) + X4.shape[1:]))
        else:
            Kff = np.stack([self.kern.K(X[b]) for b in range(B)])
        ctx = dev.get_context()
        d = [ctx.to_device(a) for a in (Kuf, Ku, Kff, self.q_mu, self.q_sqrt)]
        mean, var, info = ctx.empty((B, N, R)), ctx.empty((B, N, N, R)), C.c_int(0)
        rc = dev.lib().dcgp_svgp_conditional_full_cov(ctx.handle, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, int(self.white),
                                                      B, M, N, R, mean.ptr, var.ptr, C.byref(info))
        ctx._check(rc, info)
        return mean.numpy(), var.numpy()

    def KL(self):
        if self.white:
            return gauss_kl(self.q_mu, self.q_sqrt, K=None)
        return gauss_kl(self.q_mu, self.q_sqrt, _Kuu(self.feature, self.kern, jitter=JITTER))

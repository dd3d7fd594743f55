"""Mean functions of the conv layers -- same surface as /root/reference/conv_gp/mean_functions.py:6-41
(``IdentityConv2dMean``, ``Conv2dMean``; constructed at conv_gp/models.py:29-33,95-99 and imported flat at models.py:11), plus the
``Zero`` the reference takes from gpflow (models.py:98).

A mean function is a callable on the NHWC image (``View.mean_view``, conv_gp/views.py:12-16, hands the image through).  The
convolution runs on the device: patches through ``dcgp_extract_patches``, the filter as one MFMA GEMM (``dcgp_gemm_strided``).
``ConvLayer`` recognises a ``Conv2dMean`` whose filter is still the one its constructor built (the reference freezes it:
``conv_mean.set_trainable(False)``, models.py:100) and adds the centre pixel inside its own launch instead
(``csrc/cond.hip`` finalize / ``csrc/conv_fused.hip`` epilogue); any other callable is evaluated through ``__call__`` and added.

``LinearConv2dMean`` is this repository's own: the same convolution with ANY filter, evaluated, differentiated and optionally trained on
the device inside every model-level call (``csrc/conv_mean.hip``, dcgp_model_set_mean_filter) -- the skip path of a deep stack.
"""
import numpy as np

from . import device as dev


class MeanFunction:
    """Stand-in for gpflow.mean_functions.MeanFunction (base class of conv_gp/mean_functions.py:6)."""

    def __call__(self, X):
        raise NotImplementedError

    def set_trainable(self, flag):
        """The reference calls ``conv_mean.set_trainable(False)`` (models.py:100).  Only a ``LinearConv2dMean``'s filter is ever trained
        (the device optimiser steps move it while the flag is set when the model is built; ``DGP_Base.set_trainable(li, "mean_filter",
        on)`` switches a built model); on the other classes the flag is recorded and nothing reads it."""
        self.trainable = bool(flag)


class Zero(MeanFunction):
    """gpflow.mean_functions.Zero (conv_gp/models.py:98)."""

    def __call__(self, X):
        X = np.asarray(X)
        return np.zeros((X.shape[0], 1))


class IdentityConv2dMean(MeanFunction):
    """conv_gp/mean_functions.py:6-26: VALID convolution, NHWC in, NHWC out; the initial filter copies the centre pixel of every
    input channel into every output map (the sum over input channels)."""

    def __init__(self, filter_size, feature_maps_in, feature_maps_out=1, stride=1):
        self.filter_size = int(filter_size)
        self.feature_maps_in = int(feature_maps_in)
        self.feature_maps_out = int(feature_maps_out)
        self.stride = int(stride)
        self.trainable = True
        self.conv_filter = self._init_filter()

    def _init_filter(self):
        f = np.zeros((self.filter_size, self.filter_size, self.feature_maps_in, self.feature_maps_out))
        f[self.filter_size // 2, self.filter_size // 2, :, :] = 1.0
        return f

    def _conv(self, NHWC_X):
        """tf.nn.conv2d(X, conv_filter, strides=[1, s, s, 1], 'VALID', 'NHWC') (mean_functions.py:16-20) -> N x Ho x Wo x Cout."""
        X = np.ascontiguousarray(NHWC_X, np.float64)
        if X.ndim != 4 or X.shape[3] != self.feature_maps_in:
            raise ValueError("expected N x H x W x %d images, got %s" % (self.feature_maps_in, X.shape))
        N, H, W, Cin = X.shape
        f, s, Cout = self.filter_size, self.stride, self.feature_maps_out
        if f > H or f > W:
            raise ValueError("filter_size %d does not fit %d x %d images" % (f, H, W))
        Ho, Wo = (H - f) // s + 1, (W - f) // s + 1
        if N == 0:
            return np.zeros((0, Ho, Wo, Cout))
        filt = np.ascontiguousarray(self.conv_filter, np.float64)
        if filt.shape != (f, f, Cin, Cout):
            raise ValueError("conv_filter must be %s, got %s" % ((f, f, Cin, Cout), filt.shape))
        ctx = dev.get_context()
        L, P = f * f * Cin, Ho * Wo
        dX = ctx.to_device(X)
        patches = ctx.empty((N * P, L))          # l = (kh f + kw) C + c: the filter's own C-order flattening
        ctx._check(dev.lib().dcgp_extract_patches(ctx.handle, dX.ptr, N, H, W, Cin, f, s, patches.ptr, 0))
        dF = ctx.to_device(filt.reshape(L, Cout))
        out = ctx.empty((N * P, Cout))
        ctx.gemm(patches, (L, 1, 0), dF, (Cout, 1, 0), out, Cout, 0, N * P, Cout, L)
        return out.numpy().reshape(N, Ho, Wo, Cout)

    def __call__(self, NHWC_X):
        return self._conv(NHWC_X)


class Conv2dMean(IdentityConv2dMean):
    """conv_gp/mean_functions.py:28-41: the first output map copies the centre pixel of input channel 0, the others are zero
    mean; the result is flattened to N x (P * feature_maps_out), patch-major like ``ConvLayer``'s mean (layers.py:131)."""

    is_conv2d_mean = True     # what ConvLayer looks for (kept for objects that only quack like one)

    def _init_filter(self):
        f = np.zeros((self.filter_size, self.filter_size, self.feature_maps_in, self.feature_maps_out))
        f[self.filter_size // 2, self.filter_size // 2, 0, 0] = 1.0
        return f

    def has_initial_filter(self):
        """True while ``conv_filter`` is what ``_init_filter`` built: the case the layer kernels add themselves."""
        return np.array_equal(np.asarray(self.conv_filter), self._init_filter())

    def __call__(self, NHWC_X):
        value = self._conv(NHWC_X)
        return value.reshape(value.shape[0], -1)


MEAN_FILTERS = ("centre0", "channels", "sum")


def conv_mean_filter(kind, filter_size, feature_maps_in, feature_maps_out):
    """The named filters [f, f, Cin, Cout] of ``LinearConv2dMean``: ``"centre0"`` Conv2dMean's (the centre pixel of channel 0 into map 0),
    ``"channels"`` the centre pixel of channel c into map c for c < min(Cin, Cout) -- every channel skips to its own map; with Cin == Cout,
    stride 1 and a padding of f // 2 a true residual block -- and ``"sum"`` IdentityConv2dMean's (every channel's centre into every map).
    They have a centre, so ``filter_size`` must be odd (ValueError)."""
    f, Cin, Cout = int(filter_size), int(feature_maps_in), int(feature_maps_out)
    if kind not in MEAN_FILTERS:
        raise ValueError("mean filter %r: expected one of %s or an array [f, f, Cin, Cout]" % (kind, ", ".join(MEAN_FILTERS)))
    if f % 2 == 0:
        raise ValueError("mean filter %r: a named filter copies the centre pixel and needs an odd filter_size, got %d" % (kind, f))
    W = np.zeros((f, f, Cin, Cout))
    c0 = f // 2
    if kind == "centre0":
        W[c0, c0, 0, 0] = 1.0
    elif kind == "channels":
        for c in range(min(Cin, Cout)):
            W[c0, c0, c, c] = 1.0
    else:
        W[c0, c0, :, :] = 1.0
    return W


class LinearConv2dMean(IdentityConv2dMean):
    """m(x)[n, p, r] = sum_l patch_p(x_n)[l] W[l, r]: a VALID convolution of the image the layer's window sees with ``conv_filter``
    [f, f, Cin, Cout] (``filter``: one of ``MEAN_FILTERS`` or an array of that shape, any f), flattened to N x (P * Cout), patch-major like
    ``Conv2dMean``.  On a ``ConvLayer`` whose view has the same geometry (anything else raises ValueError there) the model-level calls run
    it on the device -- forward, reverse pass, input gradient, and with ``trainable`` the optimiser steps; the layer-level calls add
    ``__call__``'s value."""

    is_linear_conv2d_mean = True

    def __init__(self, filter_size, feature_maps_in, feature_maps_out, stride=1, filter="channels", trainable=False):
        self.filter_size = int(filter_size)
        self.feature_maps_in = int(feature_maps_in)
        self.feature_maps_out = int(feature_maps_out)
        self.stride = int(stride)
        self.trainable = bool(trainable)
        shape = (self.filter_size, self.filter_size, self.feature_maps_in, self.feature_maps_out)
        if isinstance(filter, str):
            self.conv_filter = conv_mean_filter(filter, *shape[1:])
        else:
            W = np.array(filter, np.float64)
            if W.shape != shape:
                raise ValueError("filter must be one of %s or an array %s, got shape %s" % (", ".join(MEAN_FILTERS), shape, W.shape))
            self.conv_filter = W

    def _init_filter(self):
        return np.array(self.conv_filter, np.float64)

    def __call__(self, NHWC_X):
        value = self._conv(NHWC_X)
        return value.reshape(value.shape[0], -1)

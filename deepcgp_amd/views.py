"""Patch views -- same surface as /root/reference/conv_gp/views.py (FullView), backed by HIP.

The hot path never materialises patches (the patch gather is fused into the K_uf sweep,
``csrc/rbf.hip``); ``extract_patches`` / ``extract_patches_PNL`` exist for API parity and tests.
"""
import ctypes as C

import numpy as np

from . import device as dev


class View:
    """conv_gp/views.py:6-16."""

    def mean_view(self, NHWC_X, PNL_patches):
        return NHWC_X


class FullView(View):
    """The full view uses all patches of the image (conv_gp/views.py:18-68).  ``padding`` p >= 0: the patches of the image with p zero
    pixels added on all four sides, across all channels; ``input_size`` stays the unpadded size, ``padded_size`` is the geometry the
    sliding window (and the device layer) sees, and ``out_image_*``, ``patch_count`` and ``as_maps`` follow it.  ``dilation`` d >= 1
    (stride 1 only): the window's taps sit d pixels apart -- ``rates`` of tf.extract_image_patches, conv_gp/views.py:24,37 -- so the
    output is ``padded_size - d (f - 1)``; ``phase_size`` is ceil(padded_size / d), the geometry of the d^2 phase sub-images the device
    layer runs on (``split`` / ``merge``: space-to-batch and its inverse on the host)."""

    def __init__(self, input_size, filter_size, feature_maps, stride=1, padding=0, dilation=1):
        self.input_size = list(input_size)
        self.padding = int(padding)
        if self.padding < 0:
            raise ValueError("padding must be >= 0, got %d" % self.padding)
        self.padded_size = [self.input_size[0] + 2 * self.padding, self.input_size[1] + 2 * self.padding]
        self.stride = int(stride)
        if int(dilation) != dilation or int(dilation) < 1:
            raise ValueError("dilation must be an integer >= 1, got %r" % (dilation,))
        self.dilation = int(dilation)
        if self.dilation > 1 and self.stride != 1:
            raise ValueError("dilation %d needs stride 1, got stride %d" % (self.dilation, self.stride))
        self.filter_size = int(filter_size)
        self.feature_maps = int(feature_maps)
        self.patch_shape = [self.filter_size, self.filter_size]
        self.out_image_height, self.out_image_width = self._out_image_size()
        self.patch_count = self._patch_count()
        self.patch_length = self._patch_length()
        if self.out_image_height <= 0 or self.out_image_width <= 0:
            raise ValueError("filter_size %d%s does not fit input_size %s" % (
                filter_size, " with dilation %d" % self.dilation if self.dilation > 1 else "", self.input_size))
        d = self.dilation
        self.phase_size = [-(-self.padded_size[0] // d), -(-self.padded_size[1] // d)]

    def _patch_length(self):
        return self.feature_maps * int(np.prod(self.patch_shape))

    def _patch_count(self):
        return self.out_image_height * self.out_image_width

    def _out_image_size(self):
        span = [self.dilation * (f - 1) + 1 for f in self.patch_shape]
        h = (self.padded_size[0] - span[0]) // self.stride + 1
        w = (self.padded_size[1] - span[1]) // self.stride + 1
        return h, w

    def split(self, NHWC):
        """Space-to-batch: [N, H, W, C] -> [N d^2, ceil(H / d), ceil(W / d), C], sub-image (n d + a) d + b = x[n, a::d, b::d], zero
        where a sub-image is shorter than the largest (the array itself when d == 1)."""
        d = self.dilation
        if d == 1:
            return NHWC
        x = np.asarray(NHWC, np.float64)
        N, H, W, Cc = x.shape
        Hs, Ws = -(-H // d), -(-W // d)
        out = np.zeros((N, d, d, Hs, Ws, Cc))
        for a in range(d):
            for b in range(d):
                sub = x[:, a::d, b::d]
                out[:, a, b, :sub.shape[1], :sub.shape[2]] = sub
        return out.reshape(N * d * d, Hs, Ws, Cc)

    def merge(self, sub, H, W):
        """Batch-to-space, the inverse of ``split`` on an H x W image: [N d^2, ceil(H / d), ceil(W / d), C] -> [N, H, W, C]; the
        entries ``split`` filled are dropped."""
        d = self.dilation
        if d == 1:
            return sub
        sub = np.asarray(sub, np.float64)
        Hs, Ws = -(-H // d), -(-W // d)
        sub = sub.reshape(-1, d, d, Hs, Ws, sub.shape[-1])
        out = np.empty((sub.shape[0], H, W, sub.shape[-1]))
        for a in range(d):
            for b in range(d):
                t = out[:, a::d, b::d]
                t[...] = sub[:, a, b, :t.shape[1], :t.shape[2]]
        return out

    def pad(self, NHWC_X):
        """[N, H, W, C] -> [N, H + 2p, W + 2p, C] with the zero border (the array itself when p == 0)."""
        p = self.padding
        if p == 0:
            return NHWC_X
        return np.ascontiguousarray(np.pad(np.asarray(NHWC_X, np.float64), ((0, 0), (p, p), (p, p), (0, 0))))

    def _extract(self, NHWC_X, pnl):
        ctx = dev.get_context()
        X = np.ascontiguousarray(NHWC_X, np.float64)
        N, H, W, Cc = X.shape
        if [H, W] != self.input_size[:2] or Cc != self.feature_maps:
            raise ValueError("expected N x %s x %d images, got %s" % (self.input_size[:2], self.feature_maps, X.shape))
        P, L = self.patch_count, self.patch_length
        if N == 0:
            return np.zeros((P, 0, L) if pnl else (0, P, L))
        X = self.pad(X)
        H, W = self.padded_size
        if self.dilation > 1:
            # the dilated patches are the ordinary patches of the phase sub-images, put back in image order: patch (y, x) is patch
            # (y // d, x // d) of phase (y % d, x % d)
            Hs, Ws = self.phase_size
            f, d = self.filter_size, self.dilation
            Xs = np.ascontiguousarray(self.split(X))
            dX = ctx.to_device(Xs)
            Ps = (Hs - f + 1) * (Ws - f + 1)
            sub = ctx.empty((N * d * d, Ps, L))
            ctx._check(dev.lib().dcgp_extract_patches(ctx.handle, dX.ptr, N * d * d, Hs, Ws, Cc, f, 1, sub.ptr, 0))
            pat = self.merge(sub.numpy().reshape(N * d * d, Hs - f + 1, Ws - f + 1, L), self.out_image_height, self.out_image_width)
            pat = pat.reshape(N, P, L)
            return np.ascontiguousarray(pat.transpose(1, 0, 2)) if pnl else pat
        dX = ctx.to_device(X)
        out = ctx.empty((P, N, L) if pnl else (N, P, L))
        ctx._check(dev.lib().dcgp_extract_patches(ctx.handle, dX.ptr, N, H, W, Cc, self.filter_size, self.stride,
                                                  out.ptr, int(pnl)))
        return out.numpy()

    def as_maps(self, a):
        """[..., patch_count, R] -> [..., out_image_height, out_image_width, R]: per-patch values (``patch_mean``,
        ``predict_patch_contributions``) as images, patch p = (row p // width, column p % width).  Host only."""
        a = np.asarray(a)
        if a.ndim < 2 or a.shape[-2] != self.patch_count:
            raise ValueError("expected [..., %d, R], got %s" % (self.patch_count, a.shape))
        return a.reshape(a.shape[:-2] + (self.out_image_height, self.out_image_width, a.shape[-1]))

    def extract_patches(self, NHWC_X):
        """N x patch_count x patch_length (conv_gp/views.py:46-54)."""
        return self._extract(NHWC_X, False)

    def extract_patches_PNL(self, NHWC_X):
        """patch_count x N x patch_length (conv_gp/views.py:40-44)."""
        return self._extract(NHWC_X, True)


class RandomPartialView(View):
    """Name kept so that ``from views import FullView, RandomPartialView`` (conv_gp/models.py:10) resolves under the flat shim.
    The view itself (a random subset of patches, conv_gp/views.py:70-124) is outside this build's scope: it is
    never constructed by ``ModelBuilder``'s flags; constructing it says so."""

    def __init__(self, input_size, filter_size, feature_maps, patch_count):
        raise NotImplementedError("RandomPartialView is out of scope of the MI355X path (no reference flag selects it); use FullView")

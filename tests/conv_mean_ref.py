"""Test helper for the linear convolutional mean function (``deepcgp_amd.mean_functions.LinearConv2dMean``, csrc/conv_mean.hip;
tests/test_host_conv_mean.py, tests/test_gpu_conv_mean.py).

* ``RefConvMean``: the mean function in NumPy, a callable the UNMODIFIED oracle takes -- ``oracle.layers.ConvLayer.conditional_ND`` adds
  ``mean_function(view.mean_view(NHWC_X, PNL))`` and ``oracle.grad.conv_layer_backward`` adds ``mean_function.backward(NHWC, gmean)`` to dX.
  ``backward`` also records (X, g); ``filter_grad()`` is the filter's gradient summed over the recorded calls (``reset()`` forgets them), so
  ``elbo_and_grad`` plus ``filter_grad()`` is the whole gradient of a model with such means.
* ``oracle_model``: tests/padding_ref.py's padded oracle with a ``RefConvMean`` put on every conv layer whose spec entry has ``mean_filter``
  (a padded layer is the oracle layer on the padded geometry behind np.pad: the mean sees the padded image, as the device's does).
* tests/torch_ref.py's forward has the mean as ``patches @ W`` with W a leaf: autograd gives every group including ``mean_filter``, and dX.
  ``oracle.grad.elbo_and_grad`` knows no padded layer (it scatters patch gradients into the layer's own geometry), so the padded stacks take
  their gradients from there; the two references agree on an unpadded stack (tests/test_host_conv_mean.py).
* ``CASES`` / ``make_case``: the stacks of the GPU tests.  Test infrastructure only."""
import copy

import numpy as np

from deepcgp_amd import synthetic as syn
import padding_ref as pr
import stack_specs as ss


class RefConvMean:
    """m(x)[n, p, r] = sum_l patch_p(x_n)[l] W[l, r] on NHWC images, VALID: W [f, f, Cin, Cout], l = (kh f + kw) Cin + c."""

    def __init__(self, conv_filter, stride):
        self.W = np.array(conv_filter, np.float64)
        self.f, _, self.Cin, self.Cout = self.W.shape
        self.stride = int(stride)
        self.calls = []

    def _patches(self, X):
        """[N, H, W, C] -> [N, Ho, Wo, f f C]"""
        X = np.asarray(X, np.float64)
        N, H, Wd, C = X.shape
        f, s = self.f, self.stride
        Ho, Wo = (H - f) // s + 1, (Wd - f) // s + 1
        out = np.empty((N, Ho, Wo, f, f, C))
        for kh in range(f):
            for kw in range(f):
                out[:, :, :, kh, kw, :] = X[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s, :]
        return out.reshape(N, Ho, Wo, f * f * C)

    def __call__(self, NHWC_X):
        p = self._patches(NHWC_X)
        return (p @ self.W.reshape(-1, self.Cout)).reshape(p.shape[0], -1)

    def backward(self, NHWC_X, g):
        """g [N, P Cout] = d / d mean -> dX [N, H, W, C]; records (X, g) for ``filter_grad``."""
        X = np.asarray(NHWC_X, np.float64)
        N, H, Wd, C = X.shape
        f, s = self.f, self.stride
        Ho, Wo = (H - f) // s + 1, (Wd - f) // s + 1
        g = np.asarray(g, np.float64).reshape(N, Ho, Wo, self.Cout)
        self.calls.append((X.copy(), g.copy()))
        dp = (g @ self.W.reshape(-1, self.Cout).T).reshape(N, Ho, Wo, f, f, C)
        dX = np.zeros_like(X)
        for kh in range(f):
            for kw in range(f):
                dX[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s, :] += dp[:, :, :, kh, kw, :]
        return dX

    def filter_grad(self):
        out = np.zeros_like(self.W)
        for X, g in self.calls:
            out += np.einsum("nhwl,nhwr->lr", self._patches(X), g).reshape(self.W.shape)
        return out

    def reset(self):
        self.calls = []


def oracle_model(spec, X, Y):
    """(padded oracle model, [RefConvMean or None per conv layer])"""
    ref = pr.oracle_model(spec, X, Y)
    means = []
    for layer, c in zip(ref.layers, spec["convs"]):
        m = None
        if c.get("mean_filter") is not None:
            m = RefConvMean(np.reshape(c["mean_filter"], (c["f"], c["f"], c["C"], c["R"])), c["s"])
            (layer.inner if isinstance(layer, pr.PaddedLayer) else layer).mean_function = m
        means.append(m)
    return ref, means


def oracle_gradient(spec, X, Y, zs):
    """(ELBO, [per-layer {group: gradient}]) of an UNPADDED spec: oracle.grad.elbo_and_grad plus every RefConvMean's filter_grad()."""
    from oracle.grad import elbo_and_grad
    assert not any(l.get("pad", 0) for l in spec["convs"] + [spec["head"]])
    ref, means = oracle_model(spec, X, Y)
    e, grads = elbo_and_grad(ref, X, Y, zs)
    for g, m in zip(grads, means):
        if m is not None:
            g["mean_filter"] = m.filter_grad()
    return e, grads


# ---- the stacks of the GPU tests ----------------------------------------------------------------------------------------------------
# name -> stack_specs.stack_spec arguments (convs [(f, s, R, pad, dil)]), N, and the mean filter of every conv layer ("channels" | "centre0" | "random").  S = 2, seed 7.
#   ch_res   10 x 10 x 1 -> conv f3 s1 p1 R2 -> conv f3 s1 p1 R2 (C = R = 2: both maps skip, a residual block) -> head f3 p1; M = 12
#   even_s2  9 x 7 x 3, f4 s2 R3, M = 5: an even filter, H != W, stride 2, L = 48
#   wide_R   8 x 8 x 1, f3 s1 R17, M = 4: L = 9 is no multiple of 4, R crosses a 16-column fragment
#   m264     padding_ref.STACKS["ch_264_72"]'s geometry: the conv layer on the sweep + GEMM route (M = 264) with finalize
#   valid2   12 x 12 x 1 -> conv f3 s1 R2 -> conv f3 s2 R2 -> head f3 (P = 4), no padding: the stack oracle.grad.elbo_and_grad can differentiate
#            (on 10 x 10 the head has one patch and d / d patch_weights is dead, 4e-11)
CASES = {
    "ch_res": dict(hwc=(10, 10, 1), convs=[(3, 1, 2, 1, 1), (3, 1, 2, 1, 1)], head=(3, 1, 1), Ms=12, N=3, filters="channels"),
    "ch_res_white": dict(hwc=(10, 10, 1), convs=[(3, 1, 2, 1, 1), (3, 1, 2, 1, 1)], head=(3, 1, 1), Ms=12, N=3, filters="channels", whites=(True, True, True)),
    "even_s2": dict(hwc=(9, 7, 3), convs=[(4, 2, 3, 0, 1)], head=(2, 1, 0), Ms=5, N=3, filters="random"),
    "wide_R": dict(hwc=(8, 8, 1), convs=[(3, 1, 17, 0, 1)], head=(3, 1, 0), Ms=4, N=3, filters="random"),
    "m264": dict(pr.STACKS["ch_264_72"], filters="random"),
    "valid2": dict(hwc=(12, 12, 1), convs=[(3, 1, 2, 0, 1), (3, 2, 2, 0, 1)], head=(3, 1, 0), Ms=12, N=3, filters="random"),
}


def add_filters(spec, kind, trainable=False, seed=7):
    """``mean_filter`` [f, f, C, R] and ``mean_trainable`` on every conv entry: a name of mean_functions.MEAN_FILTERS, or "random" (0.3 N(0, 1))."""
    from deepcgp_amd.mean_functions import conv_mean_filter
    rng = np.random.default_rng(1000 + seed)
    for c in spec["convs"]:
        shape = (c["f"], c["f"], c["C"], c["R"])
        c["mean_filter"] = 0.3 * rng.standard_normal(shape) if kind == "random" else conv_mean_filter(kind, *shape[1:])
        c["mean_trainable"] = bool(trainable)
        c.pop("mean_function", None)
    return spec


def make_case(name, base=None, trainable=True, **overrides):
    """(spec, X, Y, zs) of CASES[name]; ``base``: the conv layers' base kernel ('acos' with gpflow's defaults, 'matern32' | 'matern52')."""
    k = dict(CASES[name])
    k.update(overrides)
    N, kind = k.pop("N"), k.pop("filters")
    spec = add_filters(ss.stack_spec(**k), kind, trainable=trainable)
    if base is not None:
        for c in spec["convs"]:
            c["base"] = base
            if base == "acos":      # (variance, weight_variances, bias_variance): none of them gpflow's default 1
                c["acos"] = (1.7, 0.8, 0.5)
                c["variance"] = 1.7
    X, Y = syn.make_batch(k["hwc"], N, seed=7)
    return spec, X, Y, ss.make_noise(spec, N, seed=7)


def without_filters(spec, mean_function=None):
    """The spec with its mean filters taken off (and ``mean_function`` put on every conv entry, e.g. "conv2d")."""
    out = copy.deepcopy(spec)
    for c in out["convs"]:
        c.pop("mean_filter", None)
        c.pop("mean_trainable", None)
        if mean_function is not None:
            c["mean_function"] = mean_function
    return out

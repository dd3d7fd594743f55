"""Test helper for dilated conv layers (tests/test_host_dilation.py, tests/test_gpu_dilation.py): dilated patch extraction in torch,
NumPy space-to-batch and the dilated stacks.

A conv spec entry carries ``dil`` next to ``pad`` and its unpadded ``H``, ``W`` -- the form ``ModelBuilder.spec()`` writes and
``build_layers_from_spec`` reads; tests/stack_specs.py builds such specs (a dilated layer's inducing patches are cut from images of its PHASE
size, whose ordinary patches are dilated windows of the image).

* ``torch_patches``: ``torch.nn.functional.unfold(..., dilation=d)`` in the model's patch order -- the patch extraction of
  tests/torch_ref.py's forward, which knows nothing of phase sub-images.
* ``s2b`` / ``b2s`` / ``numpy_patches`` in NumPy, for the device-against-device identity.

Test infrastructure only."""
import numpy as np

from deepcgp_amd import synthetic as syn
import stack_specs as ss


# ---- NumPy space-to-batch ------------------------------------------------------------------------------------------------------------
def s2b(x, d):
    """[n, H, W, C] -> [n d^2, ceil(H / d), ceil(W / d), C]: sub-image (n d + a) d + b is x[n, a::d, b::d], zero filled to the largest."""
    x = np.asarray(x, np.float64)
    n, H, W, C = x.shape
    Hs, Ws = -(-H // d), -(-W // d)
    out = np.zeros((n, d, d, Hs, Ws, C))
    for a in range(d):
        for b in range(d):
            t = x[:, a::d, b::d]
            out[:, a, b, :t.shape[1], :t.shape[2]] = t
    return out.reshape(n * d * d, Hs, Ws, C)


def b2s(sub, d, H, W):
    """The inverse on an H x W image: [n d^2, ceil(H / d), ceil(W / d), C] -> [n, H, W, C]; the fill entries are dropped."""
    sub = np.asarray(sub, np.float64)
    Hs, Ws = -(-H // d), -(-W // d)
    sub = sub.reshape(-1, d, d, Hs, Ws, sub.shape[-1])
    out = np.empty((sub.shape[0], H, W, sub.shape[-1]))
    for a in range(d):
        for b in range(d):
            t = out[:, a::d, b::d]
            t[...] = sub[:, a, b, :t.shape[1], :t.shape[2]]
    return out


def numpy_patches(x, f, d=1):
    """[n, H, W, C] -> [n, Ho, Wo, f f C], stride 1, taps d apart, l = (kh f + kw) C + c."""
    n, H, W, C = x.shape
    Ho, Wo = H - d * (f - 1), W - d * (f - 1)
    out = np.empty((n, Ho, Wo, f, f, C))
    for kh in range(f):
        for kw in range(f):
            out[:, :, :, kh, kw] = x[:, d * kh:d * kh + Ho, d * kw:d * kw + Wo]
    return out.reshape(n, Ho, Wo, f * f * C)


# ---- torch ---------------------------------------------------------------------------------------------------------------------------
def torch_patches(x_nhwc, f, s, d):
    """[N, H, W, C] -> [N, P, L] with l = (kh f + kw) C + c, p = oh Wo + ow: F.unfold with ``dilation=d``."""
    import torch
    N, H, W, C = x_nhwc.shape
    u = torch.nn.functional.unfold(x_nhwc.permute(0, 3, 1, 2), kernel_size=f, stride=s, dilation=d)      # [N, C f f, P], channel-major rows
    P = u.shape[-1]
    return u.reshape(N, C, f * f, P).permute(0, 3, 2, 1).reshape(N, P, f * f * C)


# ---- the stacks of the issue ---------------------------------------------------------------------------------------------------------
# stack_specs.stack_spec arguments: convs [(f, s, R, pad, dil)], head (f, s, pad).
#   dil2          10 x 10 x 1 -> conv f3 d2 R2 with Conv2dMean (6 x 6) -> conv f3 d1 R2 (4 x 4) -> ConvKernel head f3 (P = 4): d divides both sides
#   dil2_odd      9 x 7 x 3 -> conv f3 d2 R2 (5 x 3) -> additive head f3 (P = 3): non-square, C > 1, phantoms in both axes (d^2 P' / P = 1.6)
#   dil3_pad      11 x 11 x 1, pad 3 (17 x 17) -> conv f3 d3 R2 with Conv2dMean (11 x 11: resolution kept) -> head f5 s2 (P = 16): 17 % 3 != 0
#   two_dilated   12 x 12 x 2 -> conv f3 d2 R2 (8 x 8) -> conv f3 d2 R2 (4 x 4) -> head f3 (P = 4): a dilated layer above layer 0, one feeding the head
#   ch_264_72_d2  28 x 28 x 1 -> conv f5 d2 R4, M 264 (20 x 20) -> head f5, M 72 (P = 256), N = 2: the sweep + GEMM route above M = 256
STACKS = {
    "dil2": dict(hwc=(10, 10, 1), convs=[(3, 1, 2, 0, 2), (3, 1, 2, 0, 1)], head=(3, 1, 0), Ms=12, N=3, conv2d_mean=(0,)),
    "dil2_odd": dict(hwc=(9, 7, 3), convs=[(3, 1, 2, 0, 2)], head=(3, 1, 0), Ms=12, N=3, additive=True),
    "dil3_pad": dict(hwc=(11, 11, 1), convs=[(3, 1, 2, 3, 3)], head=(5, 2, 0), Ms=12, N=3, conv2d_mean=(0,)),
    "two_dilated": dict(hwc=(12, 12, 2), convs=[(3, 1, 2, 0, 2), (3, 1, 2, 0, 2)], head=(3, 1, 0), Ms=12, N=3),
    "two_dilated_white": dict(hwc=(12, 12, 2), convs=[(3, 1, 2, 0, 2), (3, 1, 2, 0, 2)], head=(3, 1, 0), Ms=12, N=3, whites=(True, True, True)),
    "ch_264_72_d2": dict(hwc=(28, 28, 1), convs=[(5, 1, 4, 0, 2)], head=(5, 1, 0), Ms=(264, 72), N=2),
}


def make_stack(name, **overrides):
    """(spec, X, Y, zs) of STACKS[name]; S = 2, seed 7."""
    k = dict(STACKS[name])
    k.update(overrides)
    N = k.pop("N")
    spec = ss.stack_spec(**k)
    X, Y = syn.make_batch(k["hwc"], N, seed=7)
    return spec, X, Y, ss.make_noise(spec, N, seed=7)

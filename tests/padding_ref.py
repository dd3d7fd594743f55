"""Test helper for zero padding (tests/test_host_padding.py, tests/test_gpu_padding.py): the padded CPU oracle and the padded stacks.

A spec entry (conv layer or head) carries ``pad`` next to its UNPADDED ``H``, ``W`` -- the form ``ModelBuilder.spec()`` writes and
``build_layers_from_spec`` reads; tests/stack_specs.py builds such specs.  Two references here know no padded layer (the third, the torch
forward with ``F.pad`` in front of every patch extraction, is tests/torch_ref.py's):

* ``oracle_model``: the unmodified oracle layers built on the PADDED geometry (``physical``), each inside ``PaddedLayer``, whose
  ``conditional_ND`` applies ``np.pad`` to its input first.  The oracle package itself is untouched.
* ``physical`` alone: the spec of the VALID model that the device runs on padded images -- for the layer-0 identity test.

Test infrastructure only."""
import copy

import numpy as np

from deepcgp_amd import synthetic as syn
import stack_specs as ss


def physical(spec):
    """The same parameters as a VALID model: H, W of every entry with the border added, no ``pad``.  (Only the first layer of this spec may be
    fed as is: its later layers expect inputs that somebody padded.)"""
    out = copy.deepcopy(spec)
    for l in out["convs"] + [out["head"]]:
        p = l.pop("pad", 0)
        l["H"], l["W"] = l["H"] + 2 * p, l["W"] + 2 * p
    return out


def pad_images(X, hwc, p):
    """[n, H W C] -> [n, (H + 2p)(W + 2p) C] by np.pad."""
    H, W, C = hwc
    X4 = np.asarray(X, np.float64).reshape(-1, H, W, C)
    return np.ascontiguousarray(np.pad(X4, ((0, 0), (p, p), (p, p), (0, 0)))).reshape(X4.shape[0], -1)


class PaddedLayer:
    """An oracle layer built on the padded view, fed unpadded inputs: ``conditional_ND`` pads first; everything else is the inner layer's."""

    def __init__(self, inner, hwc, pad):
        self.inner, self.hwc, self.pad = inner, tuple(hwc), int(pad)

    def __getattr__(self, name):
        return getattr(self.__dict__["inner"], name)

    def conditional_ND(self, X, full_cov=False):
        return self.inner.conditional_ND(pad_images(X, self.hwc, self.pad), full_cov=full_cov)


def oracle_model(spec, X, Y):
    from oracle_build import oracle_model as build
    ref = build(physical(spec), X, Y)
    if spec["head"].get("kernel", "conv") == "add":
        from oracle.kernels import AdditivePatchKernel
        k = ref.layers[-1].kern
        ref.layers[-1].kern = AdditivePatchKernel(k.base_kernel, k.view, k.patch_weights)
    entries = spec["convs"] + [spec["head"]]
    ref.layers = [PaddedLayer(l, (e["H"], e["W"], e["C"]), e["pad"]) if e.get("pad", 0) else l for l, e in zip(ref.layers, entries)]
    return ref


# ---- the stacks of the issue ------------------------------------------------------------------------------------------------------------
# name -> stack_specs.stack_spec arguments (convs [(f, s, R, pad, dil)]) and N.  "res3": 10 x 10 x 1 -> conv f3 s1 p1 R2 with Conv2dMean (a residual block: same resolution) -> conv f3 s2
# p1 R2 ((10 + 2 - 3) % 2 != 0) -> ConvKernel head f3 p1, P = 25.  "wide_pad": 9 x 7 x 3 -> conv f3 s1 p2 R2 (a border wider than f // 2, a
# non-square image, C > 1) -> additive head without padding.  "ch_264_72": the smallest shape of tests/live_specs.py above M = 256 (CASES_MIXED),
# the conv layer (M = 264, the sweep + GEMM route) padded by 2: 28 -> 32, (32 - 5) % 2 != 0.
STACKS = {
    "res3": dict(hwc=(10, 10, 1), convs=[(3, 1, 2, 1, 1), (3, 2, 2, 1, 1)], head=(3, 1, 1), Ms=12, N=3, conv2d_mean=(0,)),
    "res3_white": dict(hwc=(10, 10, 1), convs=[(3, 1, 2, 1, 1), (3, 2, 2, 1, 1)], head=(3, 1, 1), Ms=12, N=3, conv2d_mean=(0,), whites=(True, True, True)),
    "wide_pad": dict(hwc=(9, 7, 3), convs=[(3, 1, 2, 2, 1)], head=(3, 1, 0), Ms=12, N=3, additive=True),
    "ch_264_72": dict(hwc=(28, 28, 1), convs=[(5, 2, 10, 2, 1)], head=(5, 1, 0), Ms=(264, 72), N=3),
}


def make_stack(name, **overrides):
    """(spec, X, Y, zs) of STACKS[name]; S = 2, seed 7."""
    k = dict(STACKS[name])
    k.update(overrides)
    N = k.pop("N")
    spec = ss.stack_spec(**k)
    X, Y = syn.make_batch(k["hwc"], N, seed=7)
    return spec, X, Y, ss.make_noise(spec, N, seed=7)

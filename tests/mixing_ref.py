"""Test helper for mixed conv layers (``ConvLayer(..., mixing=W)``, csrc/mix.hip; tests/test_host_mixing.py, tests/test_gpu_mixing.py).

* ``mirror_forward`` / ``mirror_backward_latent`` / ``mirror_backward_w``: the three kernels in NumPy with the kernels' summation order (the sums
  over g and r as chains from 0.0; gW as mix_w_plan's per-workgroup, per-slice partial sums added in slice order, then stage 2's tree).
* tests/torch_ref.py's forward takes conv entries with ``mix_W`` [R, Rout]: the sample is drawn in the latent space (``u = gm + z sqrt(gv + jitter)``,
  z of P * R values a row), mixed (``u @ W``) and only then given the mean function, which has Rout maps; ``W`` is a leaf (``mixing``) and
  ``Fmeans`` / ``Fvars`` are the marginals ``gm W + m(x)``, ``gv W^2``.  ``test_host_mixing.py`` pins W = I to the unmixed layer.
* ``CASES`` / ``make_case``: the stacks of the GPU tests, on live_specs.live_spec's per-layer construction and conv_mean_ref.add_filters.
Test infrastructure only."""
import copy

import numpy as np

from deepcgp_amd import synthetic as syn
from deepcgp_amd.layers import mixing_matrix
import conv_mean_ref as cmr
import live_specs as ls
import padding_ref as pr
import stack_specs as ss

TILE = 32      # csrc/mix.hip: kTile


# ---- NumPy mirror of the kernels ----------------------------------------------------------------------------------------------------------
def mirror_forward(W, u, gm, gv):
    """(sample, mean, var) [K, R] of (u, gm, gv) [K, G] (any may be None): sums over g = 0 .. G-1 in that order, from 0.0."""
    W = np.asarray(W, np.float64)
    out = []
    for a, sq in ((u, False), (gm, False), (gv, True)):
        if a is None:
            out.append(None)
            continue
        a = np.asarray(a, np.float64)
        acc = np.zeros((a.shape[0], W.shape[1]))
        for g in range(W.shape[0]):
            acc = acc + a[:, g, None] * ((W[g] * W[g]) if sq else W[g])[None]
        out.append(acc)
    return tuple(out)


def mirror_backward_latent(W, gF):
    """gu [K, G] = sum_r gF[:, r] W[g, r], r in order."""
    W, gF = np.asarray(W, np.float64), np.asarray(gF, np.float64)
    gu = np.zeros((gF.shape[0], W.shape[0]))
    for r in range(W.shape[1]):
        gu = gu + gF[:, r, None] * W[None, :, r]
    return gu


def w_plan(K):
    """(workgroups, columns per workgroup) of mix_backward_w on K columns (csrc/mix.hip: mix_w_plan)."""
    c = (K + 1023) // 1024
    c = max((c + TILE - 1) // TILE * TILE, TILE)
    return (K + c - 1) // c, c


def mirror_backward_w(u, gF):
    """gW [G, R] = sum_j u[j, g] gF[j, r] in the kernels' order."""
    u, gF = np.asarray(u, np.float64), np.asarray(gF, np.float64)
    K, G = u.shape
    R = gF.shape[1]
    nwg, cpw = w_plan(max(K, 1))
    nsl = 256 // min(G * R, 256)
    parts = np.zeros((256 * ((nwg + 255) // 256), G, R))      # stage 2: thread t adds workgroups t, t + 256, ..., then a tree by halves
    for x in range(nwg if K else 0):
        c1 = min((x + 1) * cpw, K)
        acc = np.zeros((nsl, G, R))
        for b in range(x * cpw, c1, TILE):
            nt = min(c1 - b, TILE)
            for q in range(nsl):
                for c in range(q, nt, nsl):
                    acc[q] = acc[q] + u[b + c, :, None] * gF[b + c, None, :]
        part = np.zeros((G, R))
        for q in range(nsl):
            part = part + acc[q]
        parts[x] = part
    red = np.zeros((256, G, R))
    for k in range(parts.shape[0] // 256):
        red = red + parts[256 * k:256 * (k + 1)]
    h = 128
    while h:
        red[:h] = red[:h] + red[h:2 * h]
        h //= 2
    return red[0]


# ---- the stacks of the GPU tests ------------------------------------------------------------------------------------------------------------
# name -> stack_specs.stack_spec arguments (convs [(f, s, Rout, pad, dil)]), N, S, `mix`: per conv layer G or 0 (unmixed), `mean`: per conv layer
# None | "conv2d" | "random" (a trained LinearConv2dMean), the seed of the mixing matrices.  M = 16 but for the large case.
#   a_*      8 x 8 x 2, f3 s1 (P = 36): one mixed layer under the head, N = 3, S = 2 (216 columns)
#   b_*      9 x 7 x 2, f3 s1 (P = 35), N = 5, S = 3 (525 columns: workgroup and wave boundaries, no multiple of 64)
#   deep     8 x 8 x 2 -> unmixed R2 (pad 1) -> mixed 3 into 2 at depth 1 (pad 1) -> head
#   pad_c2d  a mixed first layer with padding and Conv2dMean;  pad_lin: ... and a trained LinearConv2dMean on its 5 maps
#   m264     padding_ref.STACKS["ch_264_72"]'s geometry: the conv layer on the sweep + GEMM route (M = 264), 3 latent GPs into its 10 maps
# q_mu scale a = 1 (b_3_5, b_1_3_white: 2), tuned on the CPU (tests/test_host_mixing.py::test_gpu_cases_are_live): at live_specs' 0.1 the head
# hardly reads its input and another W moves the ELBO by 1e-4 only.
_A, _B = dict(hwc=(8, 8, 2), N=3, S=2, a=1.0), dict(hwc=(9, 7, 2), N=5, S=3, a=1.0)
CASES = {
    "a_3_5": dict(_A, convs=[(3, 1, 5, 0, 1)], head=(3, 1, 0), Ms=16, mix=(3,)),
    "a_4_2": dict(_A, convs=[(3, 1, 2, 0, 1)], head=(3, 1, 0), Ms=16, mix=(4,)),
    "a_1_3": dict(_A, convs=[(3, 1, 3, 0, 1)], head=(3, 1, 0), Ms=16, mix=(1,)),
    "a_3_3": dict(_A, convs=[(3, 1, 3, 0, 1)], head=(3, 1, 0), Ms=16, mix=(3,)),
    "a_3_5_white": dict(_A, convs=[(3, 1, 5, 0, 1)], head=(3, 1, 0), Ms=16, mix=(3,), whites=(True, True)),
    "b_3_5": dict(_B, convs=[(3, 1, 5, 0, 1)], head=(3, 1, 0), Ms=16, mix=(3,), a=2.0),
    "b_4_2": dict(_B, convs=[(3, 1, 2, 0, 1)], head=(3, 1, 0), Ms=16, mix=(4,)),
    "b_1_3_white": dict(_B, convs=[(3, 1, 3, 0, 1)], head=(3, 1, 0), Ms=16, mix=(1,), whites=(True, False), a=2.0),
    "b_3_3": dict(_B, convs=[(3, 1, 3, 0, 1)], head=(3, 1, 0), Ms=16, mix=(3,)),
    "deep": dict(_A, convs=[(3, 1, 2, 1, 1), (3, 1, 2, 1, 1)], head=(3, 1, 0), Ms=16, mix=(0, 3)),
    "pad_c2d": dict(_A, convs=[(3, 1, 5, 1, 1)], head=(3, 1, 0), Ms=16, mix=(3,), mean=("conv2d",)),
    "pad_lin": dict(_B, convs=[(3, 1, 5, 1, 1)], head=(3, 1, 1), Ms=16, mix=(3,), mean=("random",)),
    "m264": dict(pr.STACKS["ch_264_72"], S=2, mix=(3,), a=1.0),
}
BASES = {"a_3_5": ("matern32", "acos"), "a_4_2": ("matern52",)}      # each base kernel once (rbf: everywhere else)


def make_case(name, G=None, Rout=None, base=None, w_seed=0, w_scale=1.0, **overrides):
    """(spec, X, Y, zs) of CASES[name]; zs[l] is [S, N, P * R_l] with R_l the layer's GP count.  ``G`` / ``Rout`` override a single-conv case's
    mixing; ``w_seed``: the mixing matrices are ``w_scale * mixing_matrix("random", G, Rout, seed=w_seed + layer)``."""
    k = dict(CASES[name])
    k.update(overrides)
    N, mix, means = k.pop("N"), list(k.pop("mix")), k.pop("mean", None)
    convs = [tuple(c) for c in k["convs"]]
    if G is not None:
        mix = [int(G)]
    if Rout is not None:
        convs = [convs[0][:2] + (int(Rout),) + convs[0][3:]]
        k["convs"] = convs
    spec = ss.stack_spec(**k)
    means = means or (None,) * len(convs)
    if any(m == "random" for m in means):      # conv_mean_ref's filters, on the maps the layers emit
        filt = cmr.add_filters(copy.deepcopy(spec), "random", trainable=True)
        for c, cf, m in zip(spec["convs"], filt["convs"], means):
            if m == "random":
                c.update(mean_filter=cf["mean_filter"], mean_trainable=True)
    Ms = [k["Ms"]] * (len(convs) + 1) if np.ndim(k["Ms"]) == 0 else list(k["Ms"])
    whites = list(k.get("whites") or [False] * (len(convs) + 1))
    for li, (c, g) in enumerate(zip(spec["convs"], mix)):
        if means[li] == "conv2d":
            c["mean_function"] = "conv2d"
        if base is not None:
            c["base"] = base
            if base == "acos":
                c["acos"] = (1.7, 0.8, 0.5)
                c["variance"] = 1.7
        if not g:
            continue
        Ro, p = c["R"], c.get("pad", 0)
        # the layer's own G GPs: stack_specs.stack_spec's per-layer construction (live_specs.live_spec on the padded geometry) with R = G
        one = ls.live_spec((c["H"] + 2 * p, c["W"] + 2 * p, c["C"]), [(c["f"], c["s"], g)], (1, 1), Ms[li], k.get("c", 1.0), k.get("a", 0.1),
                           S=k.get("S", 2), seed=k.get("seed", 7) + li, white=whites[li], num_data=k.get("num_data", 60000))["convs"][0]
        assert np.array_equal(one["Z"], c["Z"])
        c.update(R=g, q_mu=one["q_mu"], q_sqrt=one["q_sqrt"], mix_W=w_scale * mixing_matrix("random", g, Ro, seed=w_seed + li), mix_trainable=True)
    X, Y = syn.make_batch(k["hwc"], N, seed=7)
    return spec, X, Y, ss.make_noise(spec, N)


def with_mixing(spec, Ws):
    """The spec with its mixed layers' W replaced (Ws: one array or None per conv layer)."""
    out = copy.deepcopy(spec)
    for c, W in zip(out["convs"], Ws):
        if W is not None:
            assert c.get("mix_W") is not None and np.shape(W) == np.shape(c["mix_W"])
            c["mix_W"] = np.array(W, np.float64)
    return out


def reseeded(spec, shift=1, w_seed=0, w_scale=1.0):
    """The spec with every mixing matrix drawn from the next seed."""
    return with_mixing(spec, [None if c.get("mix_W") is None else w_scale * mixing_matrix("random", *np.shape(c["mix_W"]), seed=w_seed + li + shift)
                              for li, c in enumerate(spec["convs"])])

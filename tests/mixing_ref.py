"""Test helper for mixed conv layers (``ConvLayer(..., mixing=W)``, csrc/mix.hip; tests/test_host_mixing.py, tests/test_gpu_mixing.py).

* ``mirror_forward`` / ``mirror_backward_latent`` / ``mirror_backward_w``: the three kernels in NumPy with the kernels' summation order (the sums
  over g and r as chains from 0.0; gW as mix_w_plan's per-workgroup, per-slice partial sums added in slice order, then stage 2's tree).
* ``torch_forward`` / ``torch_reference`` / ``torch_input_gradient``: the forward of tests/conv_mean_ref.py for specs whose conv entries may carry
  ``mix_W`` [R, Rout].  A spec without any goes to ``conv_mean_ref.torch_forward`` itself; one with a mixed layer runs the same layer loop from the
  same imported pieces (test_oracle_autograd's ``_patches`` / ``_rbf`` / ``_conditional`` / ``_gauss_kl`` / ``_robustmax_ve``, the Gram matrices of
  matern_ref and acos_ref) with the three lines a mixing changes: the sample is drawn in the latent space (``u = gm + z sqrt(gv + jitter)``, z of
  P * R values a row), mixed (``u @ W``) and only then given the mean function, which has Rout maps; ``W`` is a leaf (``mixing``).  The returned
  ``Fmeans`` / ``Fvars`` are the marginals ``gm W + m(x)``, ``gv W^2``.  ``test_host_mixing.py`` pins the two loops to each other on unmixed specs.
* ``CASES`` / ``make_case``: the stacks of the GPU tests, on live_specs.live_spec's per-layer construction and conv_mean_ref.add_filters.
Test infrastructure only."""
import copy

import numpy as np

from deepcgp_amd import synthetic as syn
from deepcgp_amd.layers import mixing_matrix
import conv_mean_ref as cmr
import live_specs as ls
import padding_ref as pr

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


# ---- torch --------------------------------------------------------------------------------------------------------------------------------
def is_mixed(spec):
    return any(c.get("mix_W") is not None for c in spec["convs"])


def torch_forward(spec, X, Y, zs, x_leaf=False, ve=None):
    """conv_mean_ref.torch_forward's dict (and its arguments), plus ``Fmeans`` / ``Fvars`` [per conv layer, S N x P Rout]: the layers' marginals."""
    if not is_mixed(spec):
        return cmr.torch_forward(spec, X, Y, zs, x_leaf=x_leaf, ve=ve)
    import torch
    import test_oracle_autograd as toa
    from matern_ref import NU2, torch_gram
    T, JITTER = toa.T, toa.JITTER
    S, N = spec["S"], np.shape(X)[0]
    Xt = torch.tensor(np.asarray(X, np.float64).reshape(N, -1), dtype=T, requires_grad=bool(x_leaf))
    F = Xt.repeat(S, 1)
    kl = torch.zeros((), dtype=T)
    leaves, samples, Fmeans, Fvars = [], [], [], []

    def leaf(a):
        return torch.tensor(np.array(a, np.float64), dtype=T, requires_grad=True)

    def window(F, e):
        p = e.get("pad", 0)
        x = F.reshape(S * N, e["H"], e["W"], e["C"])
        return toa._patches(torch.nn.functional.pad(x, (0, 0, p, p, p, p)), e["f"], e["s"])
    for li, c in enumerate(spec["convs"]):
        p = dict(Z=leaf(c["Z"]), q_mu=leaf(c["q_mu"]), q_sqrt=leaf(c["q_sqrt"]), variance=leaf(c["variance"]), lengthscales=leaf(c["ls"]))
        leaves.append(p)
        M, R = c["M"], c["R"]
        pt = window(F, c)
        P = pt.shape[1]
        cols = pt.reshape(S * N * P, -1)
        base = c.get("base", "rbf")
        if base in NU2:
            kern = lambda A, B, same=False, p=p, nu2=NU2[base]: torch_gram(A, B, p["variance"], p["lengthscales"], nu2)   # noqa: E731
        elif base == "acos":
            import acos_ref
            av, aw, ab = c.get("acos", (1.0, 1.0, 1.0))
            del p["lengthscales"]
            p.update(variance=leaf(av), weight_variances=leaf(aw), bias_variance=leaf(ab))
            kern = lambda A, B, same=False, p=p: acos_ref.torch_gram(A, B, p["variance"], p["weight_variances"], p["bias_variance"], same=same)   # noqa: E731
        else:
            assert base == "rbf", base
            kern = lambda A, B, same=False, p=p: toa._rbf(A, B, p["variance"], p["lengthscales"])               # noqa: E731
        Kuu = kern(p["Z"], p["Z"], True) + JITTER * torch.eye(M, dtype=T)
        Kuf = kern(p["Z"], cols)
        kff = p["variance"] * torch.ones(cols.shape[0], dtype=T)
        gm, gv = toa._conditional(Kuu, Kuf, kff, p["q_mu"], p["q_sqrt"], c["white"])      # [S N P, R] each
        gm, gv = gm.reshape(S * N * P, R), gv.reshape(S * N * P, R)
        z = torch.tensor(np.asarray(zs[li]).reshape(S * N * P, R), dtype=T)               # P * R values a row: one per (patch, latent GP)
        u = gm + z * torch.sqrt(gv + JITTER)
        if c.get("mix_W") is not None:
            p["mixing"] = leaf(np.reshape(c["mix_W"], (R, -1)))
            Wm = p["mixing"]
        else:
            Wm = torch.eye(R, dtype=T)
        Ro = Wm.shape[1]
        smp, mean, var = u @ Wm, gm @ Wm, gv @ (Wm * Wm)
        assert c.get("mean_function") in (None, "conv2d") and not (c.get("mean_function") and c.get("mean_filter") is not None)
        m = torch.zeros(S * N * P, Ro, dtype=T)
        if c.get("mean_function") == "conv2d":      # Conv2dMean: the centre pixel of the (padded) patch's channel 0 into map 0
            centre = pt.reshape(S * N * P, c["f"], c["f"], c["C"])[:, c["f"] // 2, c["f"] // 2, 0]
            m = torch.cat([centre[:, None], torch.zeros(S * N * P, Ro - 1, dtype=T)], 1)
        if c.get("mean_filter") is not None:
            p["mean_filter"] = leaf(np.reshape(c["mean_filter"], (c["f"], c["f"], c["C"], Ro)))
            m = cols @ p["mean_filter"].reshape(-1, Ro)
        F = (smp + m).reshape(S * N, P * Ro)
        samples.append(F)
        Fmeans.append((mean + m).reshape(S * N, P * Ro))
        Fvars.append(var.reshape(S * N, P * Ro))
        Z0 = torch.tensor(np.array(c["Z0"], np.float64), dtype=T)
        Kp = None if c["white"] else kern(Z0, Z0, True) + JITTER * torch.eye(M, dtype=T)
        kl = kl + toa._gauss_kl(p["q_mu"], p["q_sqrt"], Kp)
    h = spec["head"]
    assert h.get("kernel", "conv") == "conv"
    M = h["M"]
    p = dict(Z=leaf(h["Z"]), q_mu=leaf(h["q_mu"]), q_sqrt=leaf(h["q_sqrt"]), variance=leaf(h["variance"]), lengthscales=leaf(h["ls"]),
             patch_weights=leaf(h["w"]))
    leaves.append(p)
    pt = window(F, h)
    P = pt.shape[1]
    w = p["patch_weights"]
    Kall = toa._rbf(p["Z"], pt.reshape(S * N * P, -1), p["variance"], p["lengthscales"]).reshape(M, S * N, P)
    Kzx = (Kall * w[None, None, :]).sum(2) / P
    q = pt / p["lengthscales"]
    Kpp = p["variance"] * torch.exp(-0.5 * torch.cdist(q, q, compute_mode="donot_use_mm_for_euclid_dist") ** 2)
    kdiag = torch.einsum("npq,p,q->n", Kpp, w, w) / P ** 2
    Kuu = toa._rbf(p["Z"], p["Z"], p["variance"], p["lengthscales"]) + JITTER * torch.eye(M, dtype=T)
    mean, var = toa._conditional(Kuu, Kzx, kdiag, p["q_mu"], p["q_sqrt"], h["white"])
    kl = kl + toa._gauss_kl(p["q_mu"], p["q_sqrt"], None if h["white"] else Kuu)
    if ve is None:
        y = torch.tensor(np.tile(np.asarray(Y).reshape(1, N), [S, 1]).reshape(S * N), dtype=torch.long)
        data = toa._robustmax_ve(mean, var, y).reshape(S, N).mean(0)
    else:
        data = ve(mean.reshape(S, N, -1), var.reshape(S, N, -1))
        data = data if data.dim() == 1 else data.reshape(S, N, -1).sum(2).mean(0)
    elbo = data.sum() * (spec["num_data"] / N) - kl
    return dict(elbo=elbo, kl=kl, leaves=leaves, mean=mean.reshape(S, N, -1), var=var.reshape(S, N, -1), data=data, X=Xt, F=samples,
                Fmeans=Fmeans, Fvars=Fvars)


def torch_reference(spec, X, Y, zs):
    """((ELBO, data term, KL), [per-layer {group: gradient}] -- ``mixing`` [R, Rout] among a mixed layer's); q_sqrt's cut to the lower triangle."""
    import torch
    out = torch_forward(spec, X, Y, zs)
    flat = [(li, k, t) for li, p in enumerate(out["leaves"]) for k, t in p.items()]
    tg = torch.autograd.grad(out["elbo"], [t for _, _, t in flat])
    want = [{} for _ in out["leaves"]]
    for (li, k, _), g in zip(flat, tg):
        want[li][k] = np.tril(g.numpy()) if k == "q_sqrt" else g.numpy().copy()
    return (out["elbo"].item(), out["data"].sum().item(), out["kl"].item()), want


def torch_input_gradient(spec, X, Y, zs, objective="elbo", eps=1e-3):
    """(J [N], dX [N, H W C]) of DGP_Base.input_gradient: "elbo" J_n = 1/S sum_s E_q[log p(y_n | f_sn)]; "density" J_n = log 1/S sum_s p(y_n | f_sn)
    with tests/input_grad_ref.py's per-row RobustMax quantity (test_oracle_autograd._robustmax_predict's probabilities)."""
    import torch
    if objective == "elbo":
        out = torch_forward(spec, X, Y, zs, x_leaf=True)
        J = out["data"]
    else:
        import test_oracle_autograd as toa
        S, N = spec["S"], np.shape(X)[0]
        yy = torch.tensor(np.asarray(Y).reshape(N), dtype=torch.long)

        def ve(m, v):
            p = toa._robustmax_predict(m.reshape(S * N, -1), v.reshape(S * N, -1)).reshape(S, N, -1)
            return torch.log(p[:, torch.arange(N), yy].mean(0))
        out = torch_forward(spec, X, Y, zs, x_leaf=True, ve=ve)
        J = out["data"]
    (g,) = torch.autograd.grad(J.sum(), out["X"])
    return J.detach().numpy(), g.numpy()


# ---- the stacks of the GPU tests ------------------------------------------------------------------------------------------------------------
# name -> padding_ref.padded_spec arguments (convs [(f, s, Rout, pad)]), N, S, `mix`: per conv layer G or 0 (unmixed), `mean`: per conv layer
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
    "a_3_5": dict(_A, convs=[(3, 1, 5, 0)], head=(3, 1, 0), Ms=16, mix=(3,)),
    "a_4_2": dict(_A, convs=[(3, 1, 2, 0)], head=(3, 1, 0), Ms=16, mix=(4,)),
    "a_1_3": dict(_A, convs=[(3, 1, 3, 0)], head=(3, 1, 0), Ms=16, mix=(1,)),
    "a_3_3": dict(_A, convs=[(3, 1, 3, 0)], head=(3, 1, 0), Ms=16, mix=(3,)),
    "a_3_5_white": dict(_A, convs=[(3, 1, 5, 0)], head=(3, 1, 0), Ms=16, mix=(3,), whites=(True, True)),
    "b_3_5": dict(_B, convs=[(3, 1, 5, 0)], head=(3, 1, 0), Ms=16, mix=(3,), a=2.0),
    "b_4_2": dict(_B, convs=[(3, 1, 2, 0)], head=(3, 1, 0), Ms=16, mix=(4,)),
    "b_1_3_white": dict(_B, convs=[(3, 1, 3, 0)], head=(3, 1, 0), Ms=16, mix=(1,), whites=(True, False), a=2.0),
    "b_3_3": dict(_B, convs=[(3, 1, 3, 0)], head=(3, 1, 0), Ms=16, mix=(3,)),
    "deep": dict(_A, convs=[(3, 1, 2, 1), (3, 1, 2, 1)], head=(3, 1, 0), Ms=16, mix=(0, 3)),
    "pad_c2d": dict(_A, convs=[(3, 1, 5, 1)], head=(3, 1, 0), Ms=16, mix=(3,), mean=("conv2d",)),
    "pad_lin": dict(_B, convs=[(3, 1, 5, 1)], head=(3, 1, 1), Ms=16, mix=(3,), mean=("random",)),
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
        convs = [(convs[0][0], convs[0][1], int(Rout), convs[0][3])]
        k["convs"] = convs
    spec = pr.padded_spec(**k)
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
        # the layer's own G GPs: padding_ref.padded_spec's per-layer construction (live_specs.live_spec on the padded geometry) with R = G
        one = ls.live_spec((c["H"] + 2 * p, c["W"] + 2 * p, c["C"]), [(c["f"], c["s"], g)], (1, 1), Ms[li], k.get("c", 1.0), k.get("a", 0.1),
                           S=k.get("S", 2), seed=k.get("seed", 7) + li, white=whites[li], num_data=k.get("num_data", 60000))["convs"][0]
        assert np.array_equal(one["Z"], c["Z"])
        c.update(R=g, q_mu=one["q_mu"], q_sqrt=one["q_sqrt"], mix_W=w_scale * mixing_matrix("random", g, Ro, seed=w_seed + li), mix_trainable=True)
    X, Y = syn.make_batch(k["hwc"], N, seed=7)
    return spec, X, Y, make_noise(spec, N)


def output_dims(spec):
    """Noise values per row and layer: P * R (the GP count) for a conv layer, R for the head."""
    dims = []
    for c in spec["convs"]:
        ho, wo = pr.out_size(c["H"], c["W"], c["f"], c["s"], c.get("pad", 0))
        dims.append(ho * wo * c["R"])
    dims.append(spec["head"]["R"])
    return dims


def make_noise(spec, N, seed=7):
    rng = np.random.default_rng(20_000 + seed)
    return [rng.standard_normal((spec["S"], N, d)) for d in output_dims(spec)]


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

"""Test helper for zero padding (tests/test_host_padding.py, tests/test_gpu_padding.py): padded model specs, the padded CPU oracle and a
torch forward.

A spec entry (conv layer or head) carries ``pad`` next to its UNPADDED ``H``, ``W`` -- the form ``ModelBuilder.spec()`` writes and
``build_layers_from_spec`` reads.  Three references are built from it, none of which knows a padded layer:

* ``oracle_model``: the unmodified oracle layers built on the PADDED geometry (``physical``), each inside ``PaddedLayer``, whose
  ``conditional_ND`` applies ``np.pad`` to its input first.  The oracle package itself is untouched.
* ``torch_elbo`` / ``torch_reference`` / ``torch_input_gradient``: the textbook forward of tests/test_oracle_autograd.py (its helper functions,
  imported) with ``torch.nn.functional.pad`` in front of every patch extraction; autograd differentiates through the pad.
* ``physical`` alone: the spec of the VALID model that the device runs on padded images -- for the layer-0 identity test.

``chain`` walks the geometry, ``padded_spec`` draws live parameters (tests/live_specs.py's recipe, per layer on that layer's padded geometry:
the inducing patches are cut from images of the size the sliding window sees).  Test infrastructure only."""
import copy

import numpy as np

from deepcgp_amd import synthetic as syn
import live_specs as ls


def out_size(H, W, f, s, p):
    return (H + 2 * p - f) // s + 1, (W + 2 * p - f) // s + 1


def chain(hwc, convs, head):
    """convs [(f, s, R, pad)], head (f, s, pad) -> ([(H, W, C) entering each layer, unpadded, the head last], head patch count)."""
    H, W, C = hwc
    sizes = []
    for f, s, R, p in convs:
        sizes.append((H, W, C))
        H, W = out_size(H, W, f, s, p)
        C = R
    sizes.append((H, W, C))
    ho, wo = out_size(H, W, head[0], head[1], head[2])
    return sizes, ho * wo


def padded_spec(hwc, convs, head, Ms, S=2, seed=7, whites=None, c=1.0, a=0.1, num_data=60000, additive=False, conv2d_mean=()):
    """convs [(f, s, R, pad)], head (f, s, pad); Ms one count per layer (or one int); conv2d_mean: indices of the conv layers with Conv2dMean."""
    nl = len(convs) + 1
    Ms = [Ms] * nl if np.ndim(Ms) == 0 else list(Ms)
    whites = [False] * nl if whites is None else list(whites)
    sizes, _ = chain(hwc, convs, head)
    spec = {"S": int(S), "num_data": int(num_data), "convs": []}
    for li, (f, s, R, p) in enumerate(convs):
        H, W, C = sizes[li]
        one = ls.live_spec((H + 2 * p, W + 2 * p, C), [(f, s, R)], (1, 1), Ms[li], c, a, S=S, seed=seed + li, white=whites[li], num_data=num_data)
        layer = one["convs"][0]
        layer.update(H=H, W=W, pad=p)
        if li in conv2d_mean:
            layer["mean_function"] = "conv2d"
        spec["convs"].append(layer)
    f, s, p = head
    H, W, C = sizes[-1]
    one = ls.live_spec((H + 2 * p, W + 2 * p, C), [], (f, s), Ms[-1], c, a, S=S, seed=seed + nl, white=whites[-1], num_data=num_data)
    h = one["head"]
    h.update(H=H, W=W, pad=p)
    if additive:
        h["kernel"] = "add"
    spec["head"] = h
    return spec


def physical(spec):
    """The same parameters as a VALID model: H, W of every entry with the border added, no ``pad``.  (Only the first layer of this spec may be
    fed as is: its later layers expect inputs that somebody padded.)"""
    out = copy.deepcopy(spec)
    for l in out["convs"] + [out["head"]]:
        p = l.pop("pad", 0)
        l["H"], l["W"] = l["H"] + 2 * p, l["W"] + 2 * p
    return out


def output_dims(spec):
    dims = []
    for c in spec["convs"]:
        ho, wo = out_size(c["H"], c["W"], c["f"], c["s"], c.get("pad", 0))
        dims.append(ho * wo * c["R"])
    return dims + [spec["head"]["R"]]


def make_noise(spec, N, seed=7):
    rng = np.random.default_rng(20_000 + seed)
    return [rng.standard_normal((spec["S"], N, d)) for d in output_dims(spec)]


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


# ---- torch ------------------------------------------------------------------------------------------------------------------------------
def torch_forward(spec, Xt, zs):
    """Xt: torch [N, H W C] (may require grad).  -> (head mean [S N, R], head var [S N, R], KL, [per-layer {name: leaf}]): the forward of
    tests/test_oracle_autograd.py::_torch_elbo (RBF base kernels, Conv2dMean, ConvKernel / AdditivePatchKernel head) with F.pad in front of
    every patch extraction."""
    import torch
    from test_oracle_autograd import JITTER, T, _conditional, _gauss_kl, _patches, _rbf
    S, N = spec["S"], Xt.shape[0]
    F = Xt.repeat(S, 1)
    kl = torch.zeros((), dtype=T)
    leaves = []

    def leaf(a):
        return torch.tensor(np.array(a, np.float64), dtype=T, requires_grad=True)

    def window(F, e):     # [S N, H W C] -> patches [S N, P, L] of the zero-padded image
        p = e.get("pad", 0)
        x = F.reshape(S * N, e["H"], e["W"], e["C"])
        return _patches(torch.nn.functional.pad(x, (0, 0, p, p, p, p)), e["f"], e["s"])
    for li, c in enumerate(spec["convs"]):
        assert c.get("base", "rbf") == "rbf"
        p = dict(Z=leaf(c["Z"]), q_mu=leaf(c["q_mu"]), q_sqrt=leaf(c["q_sqrt"]), variance=leaf(c["variance"]), lengthscales=leaf(c["ls"]))
        leaves.append(p)
        M, R = c["M"], c["R"]
        pt = window(F, c)
        P = pt.shape[1]
        cols = pt.reshape(S * N * P, -1)
        Kuu = _rbf(p["Z"], p["Z"], p["variance"], p["lengthscales"]) + JITTER * torch.eye(M, dtype=T)
        Kuf = _rbf(p["Z"], cols, p["variance"], p["lengthscales"])
        kff = p["variance"] * torch.ones(cols.shape[0], dtype=T)
        mean, var = _conditional(Kuu, Kuf, kff, p["q_mu"], p["q_sqrt"], c["white"])
        mean, var = mean.reshape(S * N, P * R), var.reshape(S * N, P * R)
        if c.get("mean_function") == "conv2d":      # the centre pixel of the PADDED image's patch
            centre = pt.reshape(S * N, P, c["f"], c["f"], c["C"])[:, :, c["f"] // 2, c["f"] // 2, 0]
            mean = mean + torch.cat([centre[:, :, None], torch.zeros(S * N, P, R - 1, dtype=T)], 2).reshape(S * N, P * R)
        z = torch.tensor(np.asarray(zs[li]).reshape(S * N, P * R), dtype=T)
        F = mean + z * torch.sqrt(var + JITTER)
        Z0 = torch.tensor(np.array(c["Z0"], np.float64), dtype=T)
        Kp = None if c["white"] else _rbf(Z0, Z0, p["variance"], p["lengthscales"]) + JITTER * torch.eye(M, dtype=T)
        kl = kl + _gauss_kl(p["q_mu"], p["q_sqrt"], Kp)
    h = spec["head"]
    M = h["M"]
    p = dict(Z=leaf(h["Z"]), q_mu=leaf(h["q_mu"]), q_sqrt=leaf(h["q_sqrt"]), variance=leaf(h["variance"]), lengthscales=leaf(h["ls"]),
             patch_weights=leaf(h["w"]))
    leaves.append(p)
    pt = window(F, h)
    P = pt.shape[1]
    w = p["patch_weights"]
    Kall = _rbf(p["Z"], pt.reshape(S * N * P, -1), p["variance"], p["lengthscales"]).reshape(M, S * N, P)
    Kzx = (Kall * w[None, None, :]).sum(2) / P
    if h.get("kernel", "conv") == "add":
        kdiag = p["variance"] * w.mean() * torch.ones(S * N, dtype=T)
    else:
        q = pt / p["lengthscales"]
        Kpp = p["variance"] * torch.exp(-0.5 * torch.cdist(q, q, compute_mode="donot_use_mm_for_euclid_dist") ** 2)
        kdiag = torch.einsum("npq,p,q->n", Kpp, w, w) / P ** 2
    Kuu = _rbf(p["Z"], p["Z"], p["variance"], p["lengthscales"]) + JITTER * torch.eye(M, dtype=T)
    mean, var = _conditional(Kuu, Kzx, kdiag, p["q_mu"], p["q_sqrt"], h["white"])
    kl = kl + _gauss_kl(p["q_mu"], p["q_sqrt"], None if h["white"] else Kuu)
    return mean, var, kl, leaves


def torch_elbo(spec, X, Y, zs):
    """(ELBO, data term, KL) as torch scalars and the leaves."""
    import torch
    from test_oracle_autograd import T, _robustmax_ve
    S, N = spec["S"], np.shape(X)[0]
    mean, var, kl, leaves = torch_forward(spec, torch.tensor(np.asarray(X, np.float64), dtype=T), zs)
    y = torch.tensor(np.tile(np.asarray(Y).reshape(1, N), [S, 1]).reshape(S * N), dtype=torch.long)
    data = _robustmax_ve(mean, var, y).reshape(S, N).mean(0).sum()
    return data * (spec["num_data"] / N) - kl, data, kl, leaves


def torch_reference(spec, X, Y, zs):
    """((ELBO, data term, KL), [per-layer {group: gradient}]) -- live_specs.torch_reference for a padded spec."""
    import torch
    e, data, kl, leaves = torch_elbo(spec, X, Y, zs)
    flat = [(li, k, t) for li, p in enumerate(leaves) for k, t in p.items()]
    tg = torch.autograd.grad(e, [t for _, _, t in flat])
    want = [{} for _ in leaves]
    for (li, k, _), g in zip(flat, tg):
        want[li][k] = np.tril(g.numpy()) if k == "q_sqrt" else g.numpy().copy()
    return (e.item(), data.item(), kl.item()), want


def torch_input_gradient(spec, X, Y, zs, objective="density", eps=1e-3):
    """(J [N], dX [N, H W C]) of DGP_Base.input_gradient's two objectives (RobustMax), dX in the caller's unpadded geometry: autograd through
    the pad.  The per-row quantity is tests/input_grad_ref.py's."""
    import math
    import torch
    from input_grad_ref import _p_label_largest
    from test_oracle_autograd import T
    S, N = spec["S"], np.shape(X)[0]
    Xt = torch.tensor(np.asarray(X, np.float64), dtype=T).requires_grad_()
    mean, var, _, _ = torch_forward(spec, Xt, zs)
    K = mean.shape[1]
    y = torch.as_tensor(np.asarray(Y).reshape(-1), dtype=torch.long).repeat(S)
    P = _p_label_largest(mean, var, y).reshape(S, N)
    if objective == "density":
        J = torch.log((P * (1.0 - eps) + (1.0 - P) * eps / (K - 1.0)).mean(0))
    else:
        J = (P * math.log(1.0 - eps) + (1.0 - P) * math.log(eps / (K - 1.0))).mean(0)
    (g,) = torch.autograd.grad(J.sum(), Xt)
    return J.detach().numpy(), g.numpy()


# ---- the stacks of the issue ------------------------------------------------------------------------------------------------------------
# name -> padded_spec arguments and N.  "res3": 10 x 10 x 1 -> conv f3 s1 p1 R2 with Conv2dMean (a residual block: same resolution) -> conv f3 s2
# p1 R2 ((10 + 2 - 3) % 2 != 0) -> ConvKernel head f3 p1, P = 25.  "wide_pad": 9 x 7 x 3 -> conv f3 s1 p2 R2 (a border wider than f // 2, a
# non-square image, C > 1) -> additive head without padding.  "ch_264_72": the smallest shape of tests/live_specs.py above M = 256 (CASES_MIXED),
# the conv layer (M = 264, the sweep + GEMM route) padded by 2: 28 -> 32, (32 - 5) % 2 != 0.
STACKS = {
    "res3": dict(hwc=(10, 10, 1), convs=[(3, 1, 2, 1), (3, 2, 2, 1)], head=(3, 1, 1), Ms=12, N=3, conv2d_mean=(0,)),
    "res3_white": dict(hwc=(10, 10, 1), convs=[(3, 1, 2, 1), (3, 2, 2, 1)], head=(3, 1, 1), Ms=12, N=3, conv2d_mean=(0,), whites=(True, True, True)),
    "wide_pad": dict(hwc=(9, 7, 3), convs=[(3, 1, 2, 2)], head=(3, 1, 0), Ms=12, N=3, additive=True),
    "ch_264_72": dict(hwc=(28, 28, 1), convs=[(5, 2, 10, 2)], head=(5, 1, 0), Ms=(264, 72), N=3),
}


def make_stack(name, **overrides):
    """(spec, X, Y, zs) of STACKS[name]; S = 2, seed 7."""
    k = dict(STACKS[name])
    k.update(overrides)
    N = k.pop("N")
    spec = padded_spec(**k)
    X, Y = syn.make_batch(k["hwc"], N, seed=7)
    return spec, X, Y, make_noise(spec, N, seed=7)

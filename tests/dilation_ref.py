"""Test helper for dilated conv layers (tests/test_host_dilation.py, tests/test_gpu_dilation.py): dilated model specs, a torch forward, and
NumPy space-to-batch.

A conv spec entry carries ``dil`` next to ``pad`` and its unpadded ``H``, ``W`` -- the form ``ModelBuilder.spec()`` writes and
``build_layers_from_spec`` reads.  Two references are built from it:

* ``torch_forward`` / ``torch_reference`` / ``torch_input_gradient``: the textbook forward of tests/test_oracle_autograd.py (its ``_rbf``,
  ``_conditional``, ``_gauss_kl`` and ``_robustmax_ve``, imported) whose patch extraction is ``torch.nn.functional.unfold(..., dilation=d)``
  behind ``F.pad``.  It knows nothing of phase sub-images.  Per-element lengthscales (``ls`` a vector), the Matern Gram matrices of
  tests/matern_ref.py, a mixing matrix (``@ W``) and a mean filter (patches ``@`` filter) are the few extra lines the compositions need.
* ``s2b`` / ``b2s`` in NumPy, for the device-against-device identity.

``dilated_spec`` draws live parameters by tests/live_specs.py's recipe, per layer on the geometry the window sees: a dilated layer's inducing
patches are cut from images of its PHASE size, whose ordinary patches are dilated windows of the image.  Test infrastructure only."""
import numpy as np

from deepcgp_amd import synthetic as syn
import live_specs as ls


def out_size(H, W, f, s, p, d=1):
    span = d * (f - 1) + 1
    return (H + 2 * p - span) // s + 1, (W + 2 * p - span) // s + 1


def phase_size(H, W, p, d):
    return -(-(H + 2 * p) // d), -(-(W + 2 * p) // d)


def chain(hwc, convs, head):
    """convs [(f, R, pad, dil)] (stride 1), head (f, s, pad) -> ([(H, W, C) entering each layer, unpadded, the head last], head patch count)."""
    H, W, C = hwc
    sizes = []
    for f, R, p, d in convs:
        sizes.append((H, W, C))
        H, W = out_size(H, W, f, 1, p, d)
        C = R
    sizes.append((H, W, C))
    ho, wo = out_size(H, W, head[0], head[1], head[2])
    return sizes, ho * wo


def dilated_spec(hwc, convs, head, Ms, S=2, seed=7, whites=None, c=1.0, a=0.1, num_data=60000, additive=False, conv2d_mean=()):
    """convs [(f, R, pad, dil)], head (f, s, pad); Ms one count per layer (or one int); conv2d_mean: indices of the conv layers with Conv2dMean."""
    nl = len(convs) + 1
    Ms = [Ms] * nl if np.ndim(Ms) == 0 else list(Ms)
    whites = [False] * nl if whites is None else list(whites)
    sizes, _ = chain(hwc, convs, head)
    spec = {"S": int(S), "num_data": int(num_data), "convs": []}
    for li, (f, R, p, d) in enumerate(convs):
        H, W, C = sizes[li]
        Hs, Ws = phase_size(H, W, p, d)
        one = ls.live_spec((Hs, Ws, C), [(f, 1, R)], (1, 1), Ms[li], c, a, S=S, seed=seed + li, white=whites[li], num_data=num_data)
        layer = one["convs"][0]
        layer.update(H=H, W=W, pad=p, dil=d)
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


def output_dims(spec):
    dims = []
    for c in spec["convs"]:
        ho, wo = out_size(c["H"], c["W"], c["f"], c["s"], c.get("pad", 0), c.get("dil", 1))
        Rout = c["R"] if c.get("mix_W") is None else np.shape(c["mix_W"])[1]
        dims.append((ho * wo * c["R"], ho * wo * Rout))
    return dims + [(spec["head"]["R"], spec["head"]["R"])]


def make_noise(spec, N, seed=7):
    """Per layer [S, N, P * (the layer's GPs)] in image order."""
    rng = np.random.default_rng(20_000 + seed)
    return [rng.standard_normal((spec["S"], N, d)) for d, _ in output_dims(spec)]


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


def torch_forward(spec, X, Y, zs, x_leaf=False):
    """dict(elbo, data [N], kl, leaves [{name: tensor}] per layer, means / vars [per layer [S, N, D]], X the input tensor).  RBF (scalar or
    per-element lengthscales) and Matern base kernels, Conv2dMean's centre tap, a mean filter and a mixing matrix as leaves, a ConvKernel or
    AdditivePatchKernel head, RobustMax on the labels Y."""
    import torch
    import test_oracle_autograd as toa
    from matern_ref import NU2, torch_gram
    T, JITTER = toa.T, toa.JITTER
    S, N = spec["S"], np.shape(X)[0]
    Xt = torch.tensor(np.asarray(X, np.float64).reshape(N, -1), dtype=T, requires_grad=bool(x_leaf))
    F = Xt.repeat(S, 1)
    kl = torch.zeros((), dtype=T)
    leaves, means, vars_ = [], [], []

    def leaf(a):
        return torch.tensor(np.array(a, np.float64), dtype=T, requires_grad=True)

    def window(F, e):
        p = e.get("pad", 0)
        x = F.reshape(S * N, e["H"], e["W"], e["C"])
        return torch_patches(torch.nn.functional.pad(x, (0, 0, p, p, p, p)), e["f"], e["s"], e.get("dil", 1))
    for li, c in enumerate(spec["convs"]):
        p = dict(Z=leaf(c["Z"]), q_mu=leaf(c["q_mu"]), q_sqrt=leaf(c["q_sqrt"]), variance=leaf(c["variance"]), lengthscales=leaf(c["ls"]))
        leaves.append(p)
        M, R = c["M"], c["R"]
        pt = window(F, c)
        P = pt.shape[1]
        cols = pt.reshape(S * N * P, -1)
        base = c.get("base", "rbf")
        if base in NU2:
            kern = lambda A, B, p=p, nu2=NU2[base]: torch_gram(A, B, p["variance"], p["lengthscales"], nu2)   # noqa: E731
        else:
            assert base == "rbf", base
            kern = lambda A, B, p=p: toa._rbf(A, B, p["variance"], p["lengthscales"])                         # noqa: E731  (ls [L]: / ls per element)
        Kuu = kern(p["Z"], p["Z"]) + JITTER * torch.eye(M, dtype=T)
        Kuf = kern(p["Z"], cols)
        kff = p["variance"] * torch.ones(cols.shape[0], dtype=T)
        gm, gv = toa._conditional(Kuu, Kuf, kff, p["q_mu"], p["q_sqrt"], c["white"])      # [S N P, R]
        z = torch.tensor(np.asarray(zs[li]).reshape(S * N * P, R), dtype=T)
        Rout = R
        if c.get("mix_W") is not None:      # sample the latent GPs, then mix
            p["mixing"] = leaf(np.reshape(c["mix_W"], (R, -1)))
            Wm = p["mixing"]
            Rout = Wm.shape[1]
            smp = (gm + z * torch.sqrt(gv + JITTER)) @ Wm
            mean, var = gm @ Wm, gv @ (Wm * Wm)
        else:
            mean, var = gm, gv
            smp = None
        extra = torch.zeros(S * N * P, Rout, dtype=T)
        if c.get("mean_function") == "conv2d":      # the centre tap of the dilated window, channel 0 into map 0
            centre = pt.reshape(S * N * P, c["f"], c["f"], c["C"])[:, c["f"] // 2, c["f"] // 2, 0]
            extra = torch.cat([centre[:, None], torch.zeros(S * N * P, Rout - 1, dtype=T)], 1)
        if c.get("mean_filter") is not None:
            p["mean_filter"] = leaf(np.reshape(c["mean_filter"], (c["f"], c["f"], c["C"], Rout)))
            extra = extra + cols @ p["mean_filter"].reshape(-1, Rout)
        mean = mean + extra
        smp = mean + z * torch.sqrt(var + JITTER) if smp is None else smp + extra
        means.append(mean.reshape(S, N, P * Rout)), vars_.append(var.reshape(S, N, P * Rout))
        F = smp.reshape(S * N, P * Rout)
        Z0 = torch.tensor(np.array(c["Z0"], np.float64), dtype=T)
        Kp = None if c["white"] else kern(Z0, Z0) + JITTER * torch.eye(M, dtype=T)
        kl = kl + toa._gauss_kl(p["q_mu"], p["q_sqrt"], Kp)
    h = spec["head"]
    M = h["M"]
    p = dict(Z=leaf(h["Z"]), q_mu=leaf(h["q_mu"]), q_sqrt=leaf(h["q_sqrt"]), variance=leaf(h["variance"]), lengthscales=leaf(h["ls"]),
             patch_weights=leaf(h["w"]))
    leaves.append(p)
    pt = window(F, h)
    P = pt.shape[1]
    w = p["patch_weights"]
    Kall = toa._rbf(p["Z"], pt.reshape(S * N * P, -1), p["variance"], p["lengthscales"]).reshape(M, S * N, P)
    Kzx = (Kall * w[None, None, :]).sum(2) / P
    if h.get("kernel", "conv") == "add":
        kdiag = p["variance"] * w.mean() * torch.ones(S * N, dtype=T)
    else:
        q = pt / p["lengthscales"]
        Kpp = p["variance"] * torch.exp(-0.5 * torch.cdist(q, q, compute_mode="donot_use_mm_for_euclid_dist") ** 2)
        kdiag = torch.einsum("npq,p,q->n", Kpp, w, w) / P ** 2
    Kuu = toa._rbf(p["Z"], p["Z"], p["variance"], p["lengthscales"]) + JITTER * torch.eye(M, dtype=T)
    mean, var = toa._conditional(Kuu, Kzx, kdiag, p["q_mu"], p["q_sqrt"], h["white"])
    kl = kl + toa._gauss_kl(p["q_mu"], p["q_sqrt"], None if h["white"] else Kuu)
    means.append(mean.reshape(S, N, -1)), vars_.append(var.reshape(S, N, -1))
    y = torch.tensor(np.tile(np.asarray(Y).reshape(1, N), [S, 1]).reshape(S * N), dtype=torch.long)
    data = toa._robustmax_ve(mean, var, y).reshape(S, N).mean(0)
    elbo = data.sum() * (spec["num_data"] / N) - kl
    return dict(elbo=elbo, data=data, kl=kl, leaves=leaves, means=means, vars=vars_, X=Xt, head=(mean, var))


def torch_reference(spec, X, Y, zs):
    """dict(parts (ELBO, data term, KL), want [per-layer {group: gradient}] -- q_sqrt's cut to the lower triangle --, means, vars [per layer
    [S, N, D]] as NumPy)."""
    import torch
    out = torch_forward(spec, X, Y, zs)
    flat = [(li, k, t) for li, p in enumerate(out["leaves"]) for k, t in p.items()]
    tg = torch.autograd.grad(out["elbo"], [t for _, _, t in flat])
    want = [{} for _ in out["leaves"]]
    for (li, k, _), g in zip(flat, tg):
        want[li][k] = np.tril(g.numpy()) if k == "q_sqrt" else g.numpy().copy()
    return dict(parts=(out["elbo"].item(), out["data"].sum().item(), out["kl"].item()), want=want,
                means=[m.detach().numpy() for m in out["means"]], vars=[v.detach().numpy() for v in out["vars"]])


def torch_input_gradient(spec, X, Y, zs, objective="density", eps=1e-3):
    """(J [N], dX [N, H W C]) of DGP_Base.input_gradient's two objectives (RobustMax), dX in the caller's unpadded, undilated geometry:
    autograd through the pad and the unfold.  The per-row quantity is tests/input_grad_ref.py's (as tests/padding_ref.py uses it)."""
    import math
    import torch
    from input_grad_ref import _p_label_largest
    S, N = spec["S"], np.shape(X)[0]
    out = torch_forward(spec, X, Y, zs, x_leaf=True)
    mean, var = out["head"]
    K = mean.shape[1]
    y = torch.as_tensor(np.asarray(Y).reshape(-1), dtype=torch.long).repeat(S)
    P = _p_label_largest(mean, var, y).reshape(S, N)
    if objective == "density":
        J = torch.log((P * (1.0 - eps) + (1.0 - P) * eps / (K - 1.0)).mean(0))
    else:
        J = (P * math.log(1.0 - eps) + (1.0 - P) * math.log(eps / (K - 1.0))).mean(0)
    (g,) = torch.autograd.grad(J.sum(), out["X"])
    return J.detach().numpy(), g.numpy()


# ---- the stacks of the issue ---------------------------------------------------------------------------------------------------------
# convs [(f, R, pad, dil)], head (f, s, pad).
#   dil2          10 x 10 x 1 -> conv f3 d2 R2 with Conv2dMean (6 x 6) -> conv f3 d1 R2 (4 x 4) -> ConvKernel head f3 (P = 4): d divides both sides
#   dil2_odd      9 x 7 x 3 -> conv f3 d2 R2 (5 x 3) -> additive head f3 (P = 3): non-square, C > 1, phantoms in both axes (d^2 P' / P = 1.6)
#   dil3_pad      11 x 11 x 1, pad 3 (17 x 17) -> conv f3 d3 R2 with Conv2dMean (11 x 11: resolution kept) -> head f5 s2 (P = 16): 17 % 3 != 0
#   two_dilated   12 x 12 x 2 -> conv f3 d2 R2 (8 x 8) -> conv f3 d2 R2 (4 x 4) -> head f3 (P = 4): a dilated layer above layer 0, one feeding the head
#   ch_264_72_d2  28 x 28 x 1 -> conv f5 d2 R4, M 264 (20 x 20) -> head f5, M 72 (P = 256), N = 2: the sweep + GEMM route above M = 256
STACKS = {
    "dil2": dict(hwc=(10, 10, 1), convs=[(3, 2, 0, 2), (3, 2, 0, 1)], head=(3, 1, 0), Ms=12, N=3, conv2d_mean=(0,)),
    "dil2_odd": dict(hwc=(9, 7, 3), convs=[(3, 2, 0, 2)], head=(3, 1, 0), Ms=12, N=3, additive=True),
    "dil3_pad": dict(hwc=(11, 11, 1), convs=[(3, 2, 3, 3)], head=(5, 2, 0), Ms=12, N=3, conv2d_mean=(0,)),
    "two_dilated": dict(hwc=(12, 12, 2), convs=[(3, 2, 0, 2), (3, 2, 0, 2)], head=(3, 1, 0), Ms=12, N=3),
    "two_dilated_white": dict(hwc=(12, 12, 2), convs=[(3, 2, 0, 2), (3, 2, 0, 2)], head=(3, 1, 0), Ms=12, N=3, whites=(True, True, True)),
    "ch_264_72_d2": dict(hwc=(28, 28, 1), convs=[(5, 4, 0, 2)], head=(5, 1, 0), Ms=(264, 72), N=2),
}


def make_stack(name, **overrides):
    """(spec, X, Y, zs) of STACKS[name]; S = 2, seed 7."""
    k = dict(STACKS[name])
    k.update(overrides)
    N = k.pop("N")
    spec = dilated_spec(**k)
    X, Y = syn.make_batch(k["hwc"], N, seed=7)
    return spec, X, Y, make_noise(spec, N, seed=7)

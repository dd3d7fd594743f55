"""Test helper for the linear convolutional mean function (``deepcgp_amd.mean_functions.LinearConv2dMean``, csrc/conv_mean.hip;
tests/test_host_conv_mean.py, tests/test_gpu_conv_mean.py).

* ``RefConvMean``: the mean function in NumPy, a callable the UNMODIFIED oracle takes -- ``oracle.layers.ConvLayer.conditional_ND`` adds
  ``mean_function(view.mean_view(NHWC_X, PNL))`` and ``oracle.grad.conv_layer_backward`` adds ``mean_function.backward(NHWC, gmean)`` to dX.
  ``backward`` also records (X, g); ``filter_grad()`` is the filter's gradient summed over the recorded calls (``reset()`` forgets them), so
  ``elbo_and_grad`` plus ``filter_grad()`` is the whole gradient of a model with such means.
* ``oracle_model``: tests/padding_ref.py's padded oracle with a ``RefConvMean`` put on every conv layer whose spec entry has ``mean_filter``
  (a padded layer is the oracle layer on the padded geometry behind np.pad: the mean sees the padded image, as the device's does).
* ``torch_forward`` / ``torch_reference`` / ``torch_input_gradient``: the textbook forward of tests/test_oracle_autograd.py (its helper
  functions, imported) with F.pad in front of every patch extraction, RBF / Matern / ArcCosine base kernels (the Gram matrices of
  tests/matern_ref.py and tests/acos_ref.py) and the mean as ``patches @ W`` with W a leaf: autograd gives every group including ``mean_filter``, and dX.  ``oracle.grad.elbo_and_grad`` knows
  no padded layer (it scatters patch gradients into the layer's own geometry), so the padded stacks take their gradients from here; the
  two references agree on an unpadded stack (tests/test_host_conv_mean.py).
* ``CASES`` / ``make_case``: the stacks of the GPU tests.  Test infrastructure only."""
import copy

import numpy as np

from deepcgp_amd import synthetic as syn
import padding_ref as pr


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


# ---- torch --------------------------------------------------------------------------------------------------------------------------
def torch_forward(spec, X, Y, zs, x_leaf=False, ve=None):
    """dict(elbo, kl, leaves [{name: tensor}] per layer -- ``mean_filter`` [f, f, C, R] among a conv layer's where it has one --, mean, var
    [S, N, R] of the head, data [N] = 1/S sum_s E_q[log p(y_n | f_sn)], X the input tensor (a leaf when x_leaf), F [per conv layer samples]).
    ``ve``: another likelihood's rule (tests/compose_ref.py), a callable (mean, var [S, N, R]) -> E_q[log p(y | f)] as [S, N] or [S, N, R]
    (summed over R, averaged over S) or the per-image average [N] itself; None: RobustMax on the labels Y.  A conv entry with
    ``mean_function`` "conv2d" adds Conv2dMean's centre pixel."""
    import torch
    import test_oracle_autograd as toa
    from matern_ref import NU2, torch_gram
    T, JITTER = toa.T, toa.JITTER
    S, N = spec["S"], np.shape(X)[0]
    Xt = torch.tensor(np.asarray(X, np.float64).reshape(N, -1), dtype=T, requires_grad=bool(x_leaf))
    F = Xt.repeat(S, 1)
    kl = torch.zeros((), dtype=T)
    leaves, samples = [], []

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
        elif base == "acos":      # tests/acos_ref.py's Gram matrix (K(Z, Z)'s diagonal in closed form); leaves as the device names them
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
        mean, var = toa._conditional(Kuu, Kuf, kff, p["q_mu"], p["q_sqrt"], c["white"])
        mean, var = mean.reshape(S * N, P * R), var.reshape(S * N, P * R)
        assert c.get("mean_function") in (None, "conv2d") and not (c.get("mean_function") and c.get("mean_filter") is not None)
        if c.get("mean_function") == "conv2d":      # Conv2dMean: the centre pixel of the (padded) patch's channel 0 into map 0
            centre = pt.reshape(S * N, P, c["f"], c["f"], c["C"])[:, :, c["f"] // 2, c["f"] // 2, 0]
            mean = mean + torch.cat([centre[:, :, None], torch.zeros(S * N, P, R - 1, dtype=T)], 2).reshape(S * N, P * R)
        if c.get("mean_filter") is not None:
            p["mean_filter"] = leaf(np.reshape(c["mean_filter"], (c["f"], c["f"], c["C"], R)))
            mean = mean + (cols @ p["mean_filter"].reshape(-1, R)).reshape(S * N, P * R)
        z = torch.tensor(np.asarray(zs[li]).reshape(S * N, P * R), dtype=T)
        F = mean + z * torch.sqrt(var + JITTER)
        samples.append(F)
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
    return dict(elbo=elbo, kl=kl, leaves=leaves, mean=mean.reshape(S, N, -1), var=var.reshape(S, N, -1), data=data, X=Xt, F=samples)


def torch_reference(spec, X, Y, zs):
    """((ELBO, data term, KL), [per-layer {group: gradient}]); q_sqrt's gradient cut to the lower triangle (the parameter)."""
    import torch
    out = torch_forward(spec, X, Y, zs)
    flat = [(li, k, t) for li, p in enumerate(out["leaves"]) for k, t in p.items()]
    tg = torch.autograd.grad(out["elbo"], [t for _, _, t in flat])
    want = [{} for _ in out["leaves"]]
    for (li, k, _), g in zip(flat, tg):
        want[li][k] = np.tril(g.numpy()) if k == "q_sqrt" else g.numpy().copy()
    return (out["elbo"].item(), out["data"].sum().item(), out["kl"].item()), want


def torch_input_gradient(spec, X, Y, zs):
    """(J [N], dX [N, H W C]) of DGP_Base.input_gradient(objective="elbo"): J_n = 1/S sum_s E_q[log p(y_n | f_sn)], the per-row quantity of
    tests/input_grad_ref.py's RobustMax objective, through a forward that has the mean's term; dX in the caller's unpadded geometry."""
    import torch
    out = torch_forward(spec, X, Y, zs, x_leaf=True)
    (g,) = torch.autograd.grad(out["data"].sum(), out["X"])
    return out["data"].detach().numpy(), g.numpy()


# ---- the stacks of the GPU tests ----------------------------------------------------------------------------------------------------
# name -> padding_ref.padded_spec arguments, N, and the mean filter of every conv layer ("channels" | "centre0" | "random").  S = 2, seed 7.
#   ch_res   10 x 10 x 1 -> conv f3 s1 p1 R2 -> conv f3 s1 p1 R2 (C = R = 2: both maps skip, a residual block) -> head f3 p1; M = 12
#   even_s2  9 x 7 x 3, f4 s2 R3, M = 5: an even filter, H != W, stride 2, L = 48
#   wide_R   8 x 8 x 1, f3 s1 R17, M = 4: L = 9 is no multiple of 4, R crosses a 16-column fragment
#   m264     padding_ref.STACKS["ch_264_72"]'s geometry: the conv layer on the sweep + GEMM route (M = 264) with finalize
#   valid2   12 x 12 x 1 -> conv f3 s1 R2 -> conv f3 s2 R2 -> head f3 (P = 4), no padding: the stack oracle.grad.elbo_and_grad can differentiate
#            (on 10 x 10 the head has one patch and d / d patch_weights is dead, 4e-11)
CASES = {
    "ch_res": dict(hwc=(10, 10, 1), convs=[(3, 1, 2, 1), (3, 1, 2, 1)], head=(3, 1, 1), Ms=12, N=3, filters="channels"),
    "ch_res_white": dict(hwc=(10, 10, 1), convs=[(3, 1, 2, 1), (3, 1, 2, 1)], head=(3, 1, 1), Ms=12, N=3, filters="channels", whites=(True, True, True)),
    "even_s2": dict(hwc=(9, 7, 3), convs=[(4, 2, 3, 0)], head=(2, 1, 0), Ms=5, N=3, filters="random"),
    "wide_R": dict(hwc=(8, 8, 1), convs=[(3, 1, 17, 0)], head=(3, 1, 0), Ms=4, N=3, filters="random"),
    "m264": dict(pr.STACKS["ch_264_72"], filters="random"),
    "valid2": dict(hwc=(12, 12, 1), convs=[(3, 1, 2, 0), (3, 2, 2, 0)], head=(3, 1, 0), Ms=12, N=3, filters="random"),
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
    spec = add_filters(pr.padded_spec(**k), kind, trainable=trainable)
    if base is not None:
        for c in spec["convs"]:
            c["base"] = base
            if base == "acos":      # (variance, weight_variances, bias_variance): none of them gpflow's default 1
                c["acos"] = (1.7, 0.8, 0.5)
                c["variance"] = 1.7
    X, Y = syn.make_batch(k["hwc"], N, seed=7)
    return spec, X, Y, pr.make_noise(spec, N, seed=7)


def without_filters(spec, mean_function=None):
    """The spec with its mean filters taken off (and ``mean_function`` put on every conv entry, e.g. "conv2d")."""
    out = copy.deepcopy(spec)
    for c in out["convs"]:
        c.pop("mean_filter", None)
        c.pop("mean_trainable", None)
        if mean_function is not None:
            c["mean_function"] = mean_function
    return out

"""Test helper: THE torch forward (float64, CPU) that the device features are judged against -- padding, dilation, the RBF / Matern /
ArcCosine base kernels, Conv2dMean and a linear conv mean, mixing, a ConvKernel or additive head, and any likelihood rule.

It is the textbook forward of tests/test_oracle_autograd.py built from that file's pieces, imported (``_rbf``, ``_conditional``,
``_gauss_kl``, ``_robustmax_ve``), the Gram matrices of tests/matern_ref.py and tests/acos_ref.py and ``dilation_ref.torch_patches`` behind
``F.pad``; autograd differentiates through all of it.  The per-feature helper files keep their Gram functions, NumPy mirrors, oracle builders
and case tables and call in here.  ``test_oracle_autograd._torch_elbo`` (the third-party pin of the oracle, with the dense ARD head) and
``input_grad_ref.head_marginals`` (written to share no code) stay apart on purpose.

The order of operations is fixed: the reference numbers of every feature's GPU tests are this file's, to the bit; tests/test_host_torch_ref.py
pins them to tests/golden/torch_ref_parent.npz.  Test infrastructure only: nothing under deepcgp_amd/ imports this file."""
import math

import numpy as np


def forward(spec, X, Y, zs, x_leaf=False, ve=None):
    """dict(elbo, kl, data [N] = 1/S sum_s E_q[log p(y_n | f_sn)], leaves [{name: tensor}] per layer, mean, var [S, N, R] of the head, X the
    input tensor (a leaf when x_leaf), F, Fmeans, Fvars [per conv layer, S N x P Rout]: the layers' samples and marginals).
    ELBO = num_data / N * sum(data) - KL.

    A conv entry may carry ``pad``, ``dil``, ``base`` ("rbf" with scalar or per-element lengthscales | "matern32" | "matern52" | "acos" with
    the optional triple ``acos``), ``mean_function`` "conv2d", ``mean_filter`` (leaf ``mean_filter`` [f, f, C, Rout]; with Conv2dMean the two
    add) and ``mix_W`` (leaf ``mixing`` [R, Rout]: the sample is drawn in the latent space and mixed).  The head is a ConvKernel or, with
    ``kernel`` "add", an AdditivePatchKernel on an RBF.
    ``ve``: a likelihood's rule, a callable (mean, var [S, N, R]) -> E_q[log p(y | f)] as [S, N] or [S, N, R] (summed over R, averaged over
    S) or the per-image average [N] itself; None: RobustMax on the labels Y."""
    import torch
    import acos_ref
    import test_oracle_autograd as toa
    from dilation_ref import torch_patches
    from matern_ref import NU2, torch_gram
    T, JITTER = toa.T, toa.JITTER
    S, N = spec["S"], np.shape(X)[0]
    Xt = torch.tensor(np.asarray(X, np.float64).reshape(N, -1), dtype=T, requires_grad=bool(x_leaf))
    F = Xt.repeat(S, 1)                                                                      # row s * N + n
    kl = torch.zeros((), dtype=T)
    leaves, samples, Fmeans, Fvars = [], [], [], []

    def leaf(a):
        return torch.tensor(np.array(a, np.float64), dtype=T, requires_grad=True)

    def window(F, e):     # [S N, H W C] -> the (dilated) patches [S N, P, L] of the zero-padded image
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
            kern = lambda A, B, same=False, p=p, nu2=NU2[base]: torch_gram(A, B, p["variance"], p["lengthscales"], nu2)   # noqa: E731
        elif base == "acos":      # K(Z, Z)'s diagonal in closed form (same=True); leaves as the device names them
            av, aw, ab = c.get("acos", (1.0, 1.0, 1.0))
            del p["lengthscales"]
            p.update(variance=leaf(av), weight_variances=leaf(aw), bias_variance=leaf(ab))
            kern = lambda A, B, same=False, p=p: acos_ref.torch_gram(A, B, p["variance"], p["weight_variances"], p["bias_variance"], same=same)   # noqa: E731
        else:
            assert base == "rbf", base
            kern = lambda A, B, same=False, p=p: toa._rbf(A, B, p["variance"], p["lengthscales"])               # noqa: E731  (ls [L]: / ls per element)
        Kuu = kern(p["Z"], p["Z"], True) + JITTER * torch.eye(M, dtype=T)
        Kuf = kern(p["Z"], cols)
        kff = p["variance"] * torch.ones(cols.shape[0], dtype=T)                               # Kdiag of all three bases
        gm, gv = toa._conditional(Kuu, Kuf, kff, p["q_mu"], p["q_sqrt"], c["white"])           # [S N P, R]
        z = torch.tensor(np.asarray(zs[li]).reshape(S * N * P, R), dtype=T)                    # one value per (patch, GP)
        u, Rout = None, R
        if c.get("mix_W") is not None:      # sample the latent GPs, then mix
            p["mixing"] = leaf(np.reshape(c["mix_W"], (R, -1)))
            Wm = p["mixing"]
            Rout = Wm.shape[1]
            u = (gm + z * torch.sqrt(gv + JITTER)) @ Wm
            gm, gv = gm @ Wm, gv @ (Wm * Wm)
        m = torch.zeros(S * N * P, Rout, dtype=T)
        assert c.get("mean_function") in (None, "conv2d"), c.get("mean_function")
        if c.get("mean_function") == "conv2d":      # Conv2dMean: the centre tap of the (padded, dilated) window's channel 0 into map 0
            centre = pt.reshape(S * N * P, c["f"], c["f"], c["C"])[:, c["f"] // 2, c["f"] // 2, 0]
            m = torch.cat([centre[:, None], torch.zeros(S * N * P, Rout - 1, dtype=T)], 1)
        if c.get("mean_filter") is not None:
            p["mean_filter"] = leaf(np.reshape(c["mean_filter"], (c["f"], c["f"], c["C"], Rout)))
            m = m + cols @ p["mean_filter"].reshape(-1, Rout)
        mean = gm + m
        smp = mean + z * torch.sqrt(gv + JITTER) if u is None else u + m      # unmixed: no `@ eye(R)`, the oracle's order of operations
        F = smp.reshape(S * N, P * Rout)
        samples.append(F)
        Fmeans.append(mean.reshape(S * N, P * Rout))
        Fvars.append(gv.reshape(S * N, P * Rout))
        Z0 = torch.tensor(np.array(c["Z0"], np.float64), dtype=T)
        Kp = None if c["white"] else kern(Z0, Z0, True) + JITTER * torch.eye(M, dtype=T)      # the frozen prior
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
    if ve is None:
        y = torch.tensor(np.tile(np.asarray(Y).reshape(1, N), [S, 1]).reshape(S * N), dtype=torch.long)
        data = toa._robustmax_ve(mean, var, y).reshape(S, N).mean(0)
    else:
        data = ve(mean.reshape(S, N, -1), var.reshape(S, N, -1))
        data = data if data.dim() == 1 else data.reshape(S, N, -1).sum(2).mean(0)
    elbo = data.sum() * (spec["num_data"] / N) - kl
    return dict(elbo=elbo, kl=kl, data=data, leaves=leaves, mean=mean.reshape(S, N, -1), var=var.reshape(S, N, -1), X=Xt, F=samples,
                Fmeans=Fmeans, Fvars=Fvars)


def gradients(out, extra=()):
    """([per-layer {group: d ELBO / d leaf}] -- q_sqrt's cut to the lower triangle, the parameter --, [d ELBO / d each tensor of ``extra``])."""
    import torch
    flat = [(li, k, t) for li, p in enumerate(out["leaves"]) for k, t in p.items()]
    tg = torch.autograd.grad(out["elbo"], [t for _, _, t in flat] + list(extra), retain_graph=True)
    want = [{} for _ in out["leaves"]]
    for (li, k, _), g in zip(flat, tg):
        want[li][k] = np.tril(g.numpy()) if k == "q_sqrt" else g.numpy().copy()
    return want, [g.numpy().copy() for g in tg[len(flat):]]


def reference(spec, X, Y, zs, ve=None):
    """dict(parts (ELBO, data term, KL), want [per-layer {group: gradient}], means, vars [per layer, the head last, [S, N, D]] as NumPy, out
    the forward's dict)."""
    out = forward(spec, X, Y, zs, ve=ve)
    S, N = out["mean"].shape[:2]
    want, _ = gradients(out)
    return dict(parts=(out["elbo"].item(), out["data"].sum().item(), out["kl"].item()), want=want, out=out,
                means=[m.detach().numpy().reshape(S, N, -1) for m in out["Fmeans"] + [out["mean"]]],
                vars=[v.detach().numpy().reshape(S, N, -1) for v in out["Fvars"] + [out["var"]]])


def input_gradient(spec, X, Y, zs, J, ve=None):
    """(J [N], dX [N, H W C]) of a per-image objective ``J(out)`` -- a callable on the forward's dict that returns [N] --, dX in the caller's
    unpadded, undilated geometry: autograd through the pad and the unfold."""
    import torch
    out = forward(spec, X, Y, zs, x_leaf=True, ve=ve)
    Jn = J(out)
    (g,) = torch.autograd.grad(Jn.sum(), out["X"])
    return Jn.detach().numpy(), g.numpy()


def data_term(out):
    """DGP_Base.input_gradient(objective="elbo"): J_n = 1/S sum_s E_q[log p(y_n | f_sn)] of the forward's own likelihood rule."""
    return out["data"]


def robustmax_objective(Y, objective="density", eps=1e-3):
    """J of DGP_Base.input_gradient's two RobustMax objectives from tests/input_grad_ref.py's per-row quantity P(f_y is the largest)."""
    import torch
    from input_grad_ref import _p_label_largest

    def J(out):
        S, N, K = out["mean"].shape
        y = torch.as_tensor(np.asarray(Y).reshape(-1), dtype=torch.long).repeat(S)
        P = _p_label_largest(out["mean"].reshape(S * N, K), out["var"].reshape(S * N, K), y).reshape(S, N)
        if objective == "density":
            return torch.log((P * (1.0 - eps) + (1.0 - P) * eps / (K - 1.0)).mean(0))
        return (P * math.log(1.0 - eps) + (1.0 - P) * math.log(eps / (K - 1.0))).mean(0)
    return J


def robustmax_density(Y):
    """J_n = log 1/S sum_s p(y_n | f_sn) from test_oracle_autograd._robustmax_predict's class probabilities."""
    import torch
    import test_oracle_autograd as toa

    def J(out):
        S, N, K = out["mean"].shape
        yy = torch.tensor(np.asarray(Y).reshape(N), dtype=torch.long)
        p = toa._robustmax_predict(out["mean"].reshape(S * N, -1), out["var"].reshape(S * N, -1)).reshape(S, N, -1)
        return torch.log(p[:, torch.arange(N), yy].mean(0))
    return J


def gaussian_rule(Y, s2):
    """The Gaussian likelihood's rule as a ``ve``: Y [N, R], variance s2 (a number)."""
    import torch

    def ve(m3, v3):
        Yt = torch.tensor(np.asarray(Y, np.float64).reshape(1, m3.shape[1], -1), dtype=m3.dtype)
        return (-0.5 * math.log(2.0 * math.pi * s2) - 0.5 * ((Yt - m3) ** 2 + v3) / s2).sum(2).mean(0)
    return ve

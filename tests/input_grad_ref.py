"""Reference for the input-gradient tests (tests/test_host_input_grad.py, tests/test_gpu_input_grad.py): PyTorch autograd (CPU, float64)
with ``X.requires_grad_()`` through a forward pass written for this file, and the float64 oracle's per-image objectives.

The forward is the textbook model from a neutral spec (deepcgp_amd.synthetic): patches by an index gather, RBF / ArcCosine(order 0) Gram
matrices from expanded squared distances / weighted inner products, the sparse conditional through two triangular solves, the head's
ConvKernel / AdditivePatchKernel / dense RBF(ARD) statistics, and the three likelihoods' per-row quantities -- RobustMax by 20-point
Gauss-Hermite quadrature, the Gaussian closed form, the jittered probit.  It shares no code with deepcgp_amd/ or with the oracle's
hand-written reverse pass.  One term is shared with the oracle rather than independent of it: the ArcCosine K_uu is evaluated in NumPy in
the oracle's expression order (see head_marginals); it depends on parameters only and nothing differentiates through it.  Test
infrastructure only."""
import math

import numpy as np
import torch

from deepcgp_amd import synthetic as syn
from oracle_build import oracle_model

JITTER = 1e-3
T = torch.float64
_GX, _GW = np.polynomial.hermite.hermgauss(20)


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64), dtype=T)


def _gather_patches(x, H, W, C, f, s):
    """x [R, H*W*C] -> [R, P, L]: p = oh * Wo + ow, l = (kh * f + kw) * C + c (tf.extract_image_patches order)."""
    Ho, Wo = (H - f) // s + 1, (W - f) // s + 1
    oh, ow, kh, kw, c = np.meshgrid(np.arange(Ho), np.arange(Wo), np.arange(f), np.arange(f), np.arange(C), indexing="ij")
    idx = ((oh * s + kh) * W + (ow * s + kw)) * C + c
    return x[:, torch.as_tensor(idx.reshape(Ho * Wo, f * f * C))]


def _rbf(A, B, variance, ls):
    A, B = A / ls, B / ls
    d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * A @ B.T
    return variance * torch.exp(-0.5 * torch.clamp(d2, min=0.0))


def _acos0(A, B, variance=1.0, wv=1.0, bv=1.0):
    inner = wv * (A @ B.T) + bv
    na, nb = torch.sqrt(wv * (A * A).sum(1) + bv), torch.sqrt(wv * (B * B).sum(1) + bv)
    return variance * (1.0 - torch.acos(1e-15 + (1.0 - 2e-15) * inner / na[:, None] / nb[None, :]) / math.pi)


def _sparse_conditional(Kuu, Kuf, kff, q_mu, q_sqrt, white):
    """q(f) at the columns of Kuf [M, n]: mean [n, R], var [n, R]."""
    M = Kuu.shape[0]
    Lu = torch.linalg.cholesky(Kuu)
    A = torch.linalg.solve_triangular(Lu, Kuf, upper=False)
    if not white:
        A = torch.linalg.solve_triangular(Lu.T, A, upper=True)
    Lq = torch.tril(q_sqrt)
    SK = Lq @ Lq.transpose(1, 2) - (torch.eye(M, dtype=T) if white else Kuu)[None]
    var = kff[:, None] + (A[None] * (SK @ A[None])).sum(1).T
    return A.T @ q_mu, var


def head_marginals(spec, X, zs):
    """X: torch [N, D_in] (may require grad) -> the head's (mean, var), each [S, N, R], with the noise zs (per layer [S, N, D])."""
    S, N = spec["S"], X.shape[0]
    F = X.repeat(S, 1)                                                         # row s * N + n
    for li, c in enumerate(spec["convs"]):
        pt = _gather_patches(F, c["H"], c["W"], c["C"], c["f"], c["s"])
        P, R, M = pt.shape[1], c["R"], c["M"]
        cols = pt.reshape(S * N * P, -1)
        Z = _t(c["Z"])
        if c.get("base", "rbf") == "acos":
            # (K_uu's diagonal is acos at 1 - 1e-15, where one ulp of the cosine moves K by 1e-9: it is the constant 1 - acos(1 - 1e-15) / pi,
            # written out as the oracle and the device write it; parameter-only, nothing differentiates through it)
            Zn = np.asarray(c["Z"], np.float64)
            den = np.sqrt(np.sum(1.0 * np.square(Zn), axis=1) + 1.0)
            theta = np.arccos(1e-15 + (1.0 - 2e-15) * (((1.0 * Zn) @ Zn.T + 1.0) / den[:, None] / den[None, :]))
            theta[np.diag_indices_from(theta)] = np.arccos(1.0 - 1e-15)
            Kuu = _t(1.0 * (1.0 / np.pi) * (np.pi - theta))
            Kuf, kff = _acos0(Z, cols), torch.ones(cols.shape[0], dtype=T)
        else:
            Kuu, Kuf = _rbf(Z, Z, c["variance"], c["ls"]), _rbf(Z, cols, c["variance"], c["ls"])
            kff = c["variance"] * torch.ones(cols.shape[0], dtype=T)
        mean, var = _sparse_conditional(Kuu + JITTER * torch.eye(M, dtype=T), Kuf, kff, _t(c["q_mu"]), _t(c["q_sqrt"]), c["white"])
        mean, var = mean.reshape(S * N, P, R), var.reshape(S * N, P * R)
        if c.get("mean_function") == "conv2d":                                   # output map 0 += centre pixel of input channel 0
            centre = (c["f"] // 2 * c["f"] + c["f"] // 2) * c["C"]
            mean = torch.cat([mean[:, :, :1] + pt[:, :, centre:centre + 1], mean[:, :, 1:]], 2)
        F = mean.reshape(S * N, P * R) + _t(zs[li]).reshape(S * N, P * R) * torch.sqrt(var + JITTER)
    h = spec["head"]
    M, Z = h["M"], _t(h["Z"])
    if h.get("kernel", "conv") == "rbf":
        ls = _t(h["ls_ard"])[None, :]
        Kuu, Kzx = _rbf(Z, Z, h["variance"], ls), _rbf(Z, F, h["variance"], ls)
        kdiag = h["variance"] * torch.ones(S * N, dtype=T)
    else:
        pt = _gather_patches(F, h["H"], h["W"], h["C"], h["f"], h["s"])
        P, w = pt.shape[1], _t(h["w"])
        Kall = _rbf(Z, pt.reshape(S * N * P, -1), h["variance"], h["ls"]).reshape(M, S * N, P)
        Kzx = (Kall * w).sum(2) / P
        Kuu = _rbf(Z, Z, h["variance"], h["ls"])
        if h.get("kernel", "conv") == "add":
            kdiag = h["variance"] * w.mean() * torch.ones(S * N, dtype=T)
        else:
            q = pt / h["ls"]
            n2 = (q * q).sum(2)
            d2 = torch.clamp(n2[:, :, None] + n2[:, None, :] - 2.0 * q @ q.transpose(1, 2), min=0.0)
            kdiag = h["variance"] * torch.einsum("npq,p,q->n", torch.exp(-0.5 * d2), w, w) / P ** 2
    mean, var = _sparse_conditional(Kuu + JITTER * torch.eye(M, dtype=T), Kzx, kdiag, _t(h["q_mu"]), _t(h["q_sqrt"]), h["white"])
    return mean.reshape(S, N, -1), var.reshape(S, N, -1)


def _p_label_largest(mu, var, y):
    """P(f_y is the largest) by 20-point Gauss-Hermite over f_y, gpflow RobustMax's clips; mu, var [n, K], y [n] long."""
    gx, gw = _t(_GX), _t(_GW / math.sqrt(math.pi))
    K = mu.shape[1]
    on = torch.nn.functional.one_hot(y, K).to(T)
    my, vy = (on * mu).sum(1), (on * var).sum(1)
    x = my[:, None] + gx[None, :] * torch.sqrt(torch.clamp(2.0 * vy, min=1e-10))[:, None]              # [n, 20]
    d = (x[:, None, :] - mu[:, :, None]) / torch.sqrt(torch.clamp(var, min=1e-10))[:, :, None]          # [n, K, 20]
    cdf = 0.5 * (1.0 + torch.erf(d / math.sqrt(2.0))) * (1.0 - 2e-4) + 1e-4
    cdf = torch.where(on[:, :, None] > 0, torch.ones_like(cdf), cdf)
    return cdf.prod(1) @ gw


def objective(spec, X, Y, zs, objective="density", likelihood="multiclass", eps=1e-3, s2=None):
    """J [N] (torch) of the batch: see DGP_Base.input_gradient.  likelihood: 'multiclass' (Y int labels), 'gaussian' (Y [N, D], variance
    s2), 'bernoulli' (Y [N, D] in {0, 1})."""
    mean, var = head_marginals(spec, X, zs)
    S, N, K = mean.shape
    if likelihood == "multiclass":
        y = torch.as_tensor(np.asarray(Y).reshape(-1), dtype=torch.long).repeat(S)
        P = _p_label_largest(mean.reshape(S * N, K), var.reshape(S * N, K), y).reshape(S, N)
        if objective == "density":
            return torch.log((P * (1.0 - eps) + (1.0 - P) * eps / (K - 1.0)).mean(0))
        return (P * math.log(1.0 - eps) + (1.0 - P) * math.log(eps / (K - 1.0))).mean(0)
    if objective != "elbo":
        raise NotImplementedError(objective)
    Yt = _t(Y).reshape(1, N, K)
    if likelihood == "gaussian":
        return (-0.5 * math.log(2.0 * math.pi * s2) - 0.5 * ((Yt - mean) ** 2 + var) / s2).sum(2).mean(0)
    gx, gw = _t(_GX), _t(_GW / math.sqrt(math.pi))
    f = mean[..., None] + torch.sqrt(torch.clamp(2.0 * var, min=1e-10))[..., None] * gx                 # [S, N, K, 20]
    p = 0.5 * (1.0 + torch.erf(f / math.sqrt(2.0))) * (1.0 - 2e-3) + 1e-3
    lp = torch.where(Yt[..., None] == 1.0, torch.log(p), torch.log(1.0 - p))
    return (lp @ gw).sum(2).mean(0)


def autograd_input_gradient(spec, X, Y, zs, **kw):
    """(J [N], dX [N, D_in]) as numpy: row n of dX is dJ_n / dX_n (the images are independent, so it is d(sum J) / dX)."""
    Xt = _t(X).clone().requires_grad_()
    J = objective(spec, Xt, Y, zs, **kw)
    (g,) = torch.autograd.grad(J.sum(), Xt)
    return J.detach().numpy(), g.numpy()


# ---- the oracle's objectives (values, central differences) --------------------------------------------------------------------------
def oracle_for(spec, X, Ylab):
    ref = oracle_model(spec, X, Ylab)
    if spec["head"].get("kernel", "conv") == "add":
        from oracle.kernels import AdditivePatchKernel
        k = ref.layers[-1].kern
        ref.layers[-1].kern = AdditivePatchKernel(k.base_kernel, k.view, k.patch_weights)
    return ref


def oracle_objective(ref, spec, X, Y, zs, objective="density", likelihood="multiclass", s2=None):
    """J [N] from the float64 oracle: predict_y / E_log_p_Y (RobustMax), propagate + a NumPy tail (Gaussian, Bernoulli)."""
    S = spec["S"]
    if likelihood == "multiclass":
        Y = np.asarray(Y).reshape(-1)
        if objective == "density":
            p, _ = ref.predict_y(X, S, zs=zs)                                    # [S, N, K]
            return np.log(p[:, np.arange(len(Y)), Y].mean(0))
        return ref.E_log_p_Y(X, Y, zs=zs)
    _, Fm, Fv = ref.propagate(X, S=S, zs=zs)
    m, v, Y = Fm[-1], Fv[-1], np.asarray(Y, np.float64)[None]
    if likelihood == "gaussian":
        return (-0.5 * np.log(2.0 * np.pi * s2) - 0.5 * (np.square(Y - m) + v) / s2).sum(2).mean(0)
    from scipy.special import erf
    f = m[..., None] + np.sqrt(np.maximum(2.0 * v, 1e-10))[..., None] * _GX
    p = 0.5 * (1.0 + erf(f / np.sqrt(2.0))) * (1.0 - 2e-3) + 1e-3
    lp = np.where(Y[..., None] == 1.0, np.log(p), np.log(1.0 - p))
    return (lp @ (_GW / np.sqrt(np.pi))).sum(2).mean(0)


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def make_case(name, white=False, M=17, S=3, N=5, seed=7, head_outputs=10):
    """(spec, X, Ylab, zs) of a named model family at small sizes."""
    kw = dict(S=S, num_data=300, seed=seed, white=white, conv_q_sqrt_scale=0.3, head_q_sqrt_scale=0.7, variance=2.0, ls=1.5, head_outputs=head_outputs)
    hwc, convs, head = (10, 10, 1), [(3, 1, 2)], (3, 1)
    if name == "head_mnist":                  # head-only, MNIST geometry
        hwc, convs, head = (28, 28, 1), [], (5, 1)
    elif name == "conv_head_cfg2":            # conv + head, cfg2 geometry
        hwc, convs, head = (28, 28, 1), [(5, 2, 10)], (5, 1)
    elif name == "three_ragged":              # three layers, stride 2, H != W, odd sizes
        hwc, convs, head = (15, 13, 1), [(4, 2, 2), (3, 1, 2)], (3, 1)
    elif name == "cifar3":                    # 3-channel first layer
        hwc, convs, head = (12, 12, 3), [(4, 2, 2)], (3, 1)
    elif name == "acos":
        kw["base_kernel"] = "acos"
    elif name == "dense_ard":
        kw["head_kernel"] = "rbf"
    elif name not in ("conv_small", "identity_mean", "additive", "head_small"):
        raise KeyError(name)
    if name == "head_small":
        convs = []
    if name in ("head_mnist", "conv_head_cfg2"):
        kw.update(variance=5.0, ls=5.0)
    if name in ("three_ragged", "cifar3"):    # (lengthscales at which the deeper features are not all far from every inducing patch)
        kw.update(ls=4.0)
    if name == "dense_ard":
        kw.update(ls=10.0)
    spec = syn.make_spec(hwc, convs, head, M, **kw)
    rng = np.random.default_rng(seed)
    if name == "conv_head_cfg2":              # (the head sees ten maps of a layer with random q_mu: a lengthscale at which it responds to them)
        spec["head"]["ls"] = 20.0
    if name != "dense_ard":
        spec["head"]["w"] = 0.5 + rng.random(spec["head"]["w"].shape)
    if name == "additive":
        spec["head"]["kernel"] = "add"
    if name == "identity_mean":
        spec["convs"][0]["mean_function"] = "conv2d"
    X, Ylab = syn.make_batch(hwc, N, seed=seed)
    zs = syn.make_noise(spec, N, seed=seed)
    return spec, X, Ylab, zs

"""Reference for the ArcCosine(order 0) base kernel of the conv layers at NON-UNIT parameters (tests/test_host_acos.py,
tests/test_gpu_acos.py).

gpflow 1.x ``ArcCosine(order=0)``:

    k(a, b) = variance (pi - acos(1e-15 + (1 - 2e-15) c)) / pi,   c = (w a.b + b) / sqrt((w |a|^2 + b)(w |b|^2 + b))
    Kdiag = variance

with w = weight_variances and b = bias_variance.  On the diagonal of a Gram matrix of one set of points c == 1 identically in the points, in w
and in b, so k(z, z) = variance DIAG with the constant DIAG = 1 - acos(1 - 1e-15) / pi: it depends on the ``variance`` leaf alone.
``torch_gram(..., same=True)`` writes that diagonal by a mask and evaluates acos on an argument whose diagonal was replaced by 0 BEFORE the
call (the double-where form): autograd never multiplies acos' slope at 1 - 1e-15 (2e7) into anything, no inf * 0 reaches a leaf, and the
hand-written diagonal skip of oracle/grad.py and csrc/grad.hip has no counterpart here.

* ``torch_forward``: the textbook torch float64 forward of tests/test_oracle_autograd.py (its ``_patches``, ``_conditional``, ``_gauss_kl``,
  ``_robustmax_ve`` and head by import) for specs whose conv layers carry ``base = "acos"``; leaves per conv layer Z, q_mu, q_sqrt, variance,
  weight_variances, bias_variance.  The head stays RBF.
* ``acos_case``: tests/live_specs.py's cases with ArcCosine conv layers whose three parameters all differ from 1, from each other and between
  layers; carried in the spec as the optional per-layer key ``acos = (variance, weight_variances, bias_variance)``, which
  ``build_layers_from_spec`` and tests/oracle_build.py honour (absent: gpflow's (1, 1, 1)).  ``c["variance"]`` mirrors the first of the three.

Test infrastructure only: nothing under deepcgp_amd/ imports this file."""
import math

import numpy as np

DIAG = 1.0 - math.acos(1.0 - 1e-15) / math.pi      # k(z, z) / variance

# per conv layer: variance, weight_variances, and bias_variance as a multiple of  w * mean_i |Z_i|^2  of the layer's own inducing patches
# (deep layers see patches 10 x and 30 x larger: at b = 1 the bias would be invisible there and d/db dead)
TRIPLES = ((1.7, 0.8, 0.5), (0.6, 1.3, 0.8), (1.4, 0.7, 0.6))
NAMES = ("variance", "weight_variances", "bias_variance")


def numpy_gram(A, B, variance, w, b):
    """The formula in NumPy, no mask (argument clamped to <= 1 as the device and oracle/grad.py do)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    da, db = np.sqrt(w * np.sum(A * A, 1) + b), np.sqrt(w * np.sum(B * B, 1) + b)
    c = (w * (A @ B.T) + b) / da[:, None] / db[None, :]
    return variance * (1.0 - np.arccos(np.minimum(1e-15 + (1.0 - 2e-15) * c, 1.0)) / np.pi)


def numpy_kuu(Z, variance, w, b):
    """K(Z, Z) with the diagonal in closed form."""
    K = numpy_gram(Z, Z, variance, w, b)
    K[np.diag_indices_from(K)] = variance * DIAG
    return K


def torch_gram(A, B, variance, w, b, same=False):
    """variance, w, b: tensors.  same=True: A is B (K_uu, the prior's K(Z0, Z0)); the diagonal is variance * DIAG."""
    import torch
    da = torch.sqrt(w * (A * A).sum(1) + b)
    db = torch.sqrt(w * (B * B).sum(1) + b)
    c = (w * (A @ B.T) + b) / da[:, None] / db[None, :]
    if same:
        eye = torch.eye(A.shape[0], dtype=torch.bool)
        c = torch.where(eye, torch.zeros_like(c), c)            # acos never sees the diagonal's 1
    k = variance * (math.pi - torch.acos(1e-15 + (1.0 - 2e-15) * c)) / math.pi
    if same:
        k = torch.where(eye, (variance * DIAG).expand_as(k), k)
    return k


def torch_forward(spec, X, Y, zs, x_leaf=False, likelihood="multiclass", s2=None):
    """dict(elbo, leaves [{name: tensor}] per layer, mean, var [S, N, R] of the head, data [N] the per-image data term
    1/S sum_s E_q[log p(y_n | f_sn)], X the input tensor (a leaf when x_leaf), layer_mean / layer_var: per conv layer [S * N, P * R]).
    ELBO = num_data / N * sum(data) - KL.  Conv layers: spec base 'acos' with the key ``acos``; the head: ConvKernel on an RBF, as
    tests/test_oracle_autograd.py's _torch_elbo builds it."""
    import torch
    import test_oracle_autograd as toa
    T, JITTER = toa.T, toa.JITTER
    S, N = spec["S"], X.shape[0]
    Xt = torch.tensor(np.asarray(X, np.float64).reshape(N, -1), dtype=T, requires_grad=bool(x_leaf))
    F = Xt.repeat(S, 1)                                                                      # row s * N + n
    kl = torch.zeros((), dtype=T)
    leaves, lmean, lvar = [], [], []

    def leaf(a):
        return torch.tensor(np.array(a, np.float64), dtype=T, requires_grad=True)
    for li, c in enumerate(spec["convs"]):
        assert c.get("base") == "acos", c.get("base")
        v, w, b = c["acos"]
        p = dict(Z=leaf(c["Z"]), q_mu=leaf(c["q_mu"]), q_sqrt=leaf(c["q_sqrt"]), variance=leaf(v), weight_variances=leaf(w), bias_variance=leaf(b))
        leaves.append(p)
        M, R = c["M"], c["R"]
        pt = toa._patches(F.reshape(S * N, c["H"], c["W"], c["C"]), c["f"], c["s"])           # [SN, P, L]
        P = pt.shape[1]
        cols = pt.reshape(S * N * P, -1)
        kern = lambda A, B, same=False, p=p: torch_gram(A, B, p["variance"], p["weight_variances"], p["bias_variance"], same)   # noqa: E731
        Kuu = kern(p["Z"], p["Z"], True) + JITTER * torch.eye(M, dtype=T)
        Kuf = kern(p["Z"], cols)
        kff = p["variance"] * torch.ones(cols.shape[0], dtype=T)                               # ArcCosine.Kdiag
        mean, var = toa._conditional(Kuu, Kuf, kff, p["q_mu"], p["q_sqrt"], c["white"])
        mean, var = mean.reshape(S * N, P * R), var.reshape(S * N, P * R)
        assert c.get("mean_function") is None
        lmean.append(mean)
        lvar.append(var)
        z = torch.tensor(np.asarray(zs[li]).reshape(S * N, P * R), dtype=T)
        F = mean + z * torch.sqrt(var + JITTER)
        Z0 = torch.tensor(np.array(c["Z0"], np.float64), dtype=T)
        Kp = None if c["white"] else kern(Z0, Z0, True) + JITTER * torch.eye(M, dtype=T)
        kl = kl + toa._gauss_kl(p["q_mu"], p["q_sqrt"], Kp)
    h = spec["head"]
    assert h.get("kernel", "conv") == "conv"
    M = h["M"]
    p = dict(Z=leaf(h["Z"]), q_mu=leaf(h["q_mu"]), q_sqrt=leaf(h["q_sqrt"]), variance=leaf(h["variance"]), lengthscales=leaf(h["ls"]),
             patch_weights=leaf(h["w"]))
    leaves.append(p)
    pt = toa._patches(F.reshape(S * N, h["H"], h["W"], h["C"]), h["f"], h["s"])
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
    if likelihood == "multiclass":
        y = torch.tensor(np.tile(np.asarray(Y).reshape(1, N), [S, 1]).reshape(S * N), dtype=torch.long)
        data = toa._robustmax_ve(mean, var, y).reshape(S, N).mean(0)
    else:
        assert likelihood == "gaussian" and s2 is not None
        Yt = torch.tensor(np.asarray(Y, np.float64).reshape(1, N, -1), dtype=T)
        m3, v3 = mean.reshape(S, N, -1), var.reshape(S, N, -1)
        data = (-0.5 * math.log(2.0 * math.pi * s2) - 0.5 * ((Yt - m3) ** 2 + v3) / s2).sum(2).mean(0)
    elbo = data.sum() * (spec["num_data"] / N) - kl
    return dict(elbo=elbo, leaves=leaves, mean=mean.reshape(S, N, -1), var=var.reshape(S, N, -1), data=data, X=Xt, layer_mean=lmean,
                layer_var=lvar)


def torch_reference(spec, X, Y, zs, **kw):
    """(ELBO, [per-layer {group: gradient}]) like live_specs.torch_reference, from ``torch_forward``."""
    import torch
    out = torch_forward(spec, X, Y, zs, **kw)
    flat = [(li, k, t) for li, p in enumerate(out["leaves"]) for k, t in p.items()]
    tg = torch.autograd.grad(out["elbo"], [t for _, _, t in flat])
    want = [{} for _ in out["leaves"]]
    for (li, k, _), g in zip(flat, tg):
        want[li][k] = np.tril(g.numpy()) if k == "q_sqrt" else g.numpy().copy()
    return out["elbo"].item(), want


def set_acos(c, variance, w, b):
    """Write the three parameters of a conv layer's spec entry (and the mirror in c['variance'])."""
    c["acos"] = (float(variance), float(w), float(b))
    c["variance"] = float(variance)


def acos_spec(spec, triples=TRIPLES, conv_q_sqrt_scale=0.3):
    """`spec` (a live_specs spec) with every conv layer turned into an ArcCosine layer at non-unit parameters, in place: layer i takes
    (variance, w, beta * w * mean |Z_i|^2) from triples[i]; an unwhitened layer's q_sqrt is rebuilt as 0.3 chol(K_uu^acos + jitter) at those
    parameters (live_spec built it from an RBF Gram)."""
    from deepcgp_amd import synthetic as syn
    for li, c in enumerate(spec["convs"]):
        v, w, beta = triples[li]
        Z = np.asarray(c["Z"], np.float64)
        b = beta * w * float(np.mean(np.sum(Z * Z, 1)))
        c["base"] = "acos"
        set_acos(c, v, w, b)
        if not c["white"]:
            Lu = np.linalg.cholesky(numpy_kuu(Z, v, w, b) + syn.JITTER * np.eye(c["M"]))
            c["q_sqrt"] = np.tile(Lu[None], [c["R"], 1, 1]) * conv_q_sqrt_scale
    return spec


def acos_case(name):
    """(spec, X, Y, zs): live_specs.make_case(name) through ``acos_spec``."""
    import live_specs as ls
    spec, X, Y, zs = ls.make_case(name)
    return acos_spec(spec), X, Y, zs


def spec_value(l, name):
    """The value of gradient group `name` in a spec layer (conv layers: the three kernel parameters live in l['acos'])."""
    import live_specs as ls
    if name in NAMES and "acos" in l:
        return l["acos"][NAMES.index(name)]
    return l[ls.SPEC_KEY[name]]


def adam_numpy_step(spec, grads, state, lr, t):
    """live_specs.adam_numpy_step on a spec with ArcCosine conv layers: the three kernel parameters move through softplus + 1e-6."""
    import live_specs as ls
    for c in spec["convs"]:
        c["variance"], c["weight_variances"], c["bias_variance"] = c["acos"]
    ls.adam_numpy_step(spec, grads, state, lr, t)
    for c in spec["convs"]:
        set_acos(c, c["variance"], c.pop("weight_variances"), c.pop("bias_variance"))

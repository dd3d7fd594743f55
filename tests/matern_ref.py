"""Reference for the Matern base kernels of the conv layers (tests/test_host_matern.py, tests/test_gpu_matern.py).

gpflow 1.x ``Matern32`` / ``Matern52`` with ``ARD=False``:

    r = sqrt(|x - z|^2 / l^2 + 1e-12)                     (gpflow's scaled_euclid_dist)
    Matern32: k = variance (1 + a) exp(-a),            a = sqrt(3) r
    Matern52: k = variance (1 + a + a^2 / 3) exp(-a),  a = sqrt(5) r
    Kdiag = variance

* ``Matern32`` / ``Matern52``: NumPy classes with ``K(A, B=None)``, ``Kdiag`` and ``variance`` -- for the operator tests and for handing
  to the oracle's layer classes, as ``oracle.gpflow_ref.ArcCosine`` is handed in tests/test_gpu_ops.py::test_acos_conv_layer.  Squared
  distances from explicit differences (no |x|^2 + |z|^2 - 2 x.z cancellation).
* ``torch_forward``: the textbook torch float64 forward of tests/test_oracle_autograd.py (its ``_patches``, ``_conditional``, ``_gauss_kl``,
  ``_robustmax_ve`` and head by import) for specs whose conv layers carry ``base in {"matern32", "matern52"}``; only the conv layers' Gram
  function differs.  Test infrastructure only: nothing under deepcgp_amd/ imports this file."""
import math

import numpy as np

NU2 = {"matern32": 3, "matern52": 5}


def _sqdist(A, B):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.zeros((A.shape[0], B.shape[0]))
    for l0 in range(0, A.shape[1], 16):          # in slabs of 16 coordinates: [a, b, 16] temporaries
        d = A[:, None, l0:l0 + 16] - B[None, :, l0:l0 + 16]
        out += np.einsum("abl,abl->ab", d, d)
    return out


class _Matern:
    nu2 = None

    def __init__(self, input_dim, variance=1.0, lengthscales=1.0):
        self.input_dim, self.variance, self.lengthscales = int(input_dim), float(variance), float(lengthscales)

    def K(self, A, B=None):
        r = np.sqrt(_sqdist(A, A if B is None else B) / self.lengthscales ** 2 + 1e-12)
        a = math.sqrt(self.nu2) * r
        return self.variance * ((1.0 + a) if self.nu2 == 3 else (1.0 + a + a * a / 3.0)) * np.exp(-a)

    def Kdiag(self, A):
        return np.full(np.shape(A)[0], self.variance)


class Matern32(_Matern):
    nu2 = 3


class Matern52(_Matern):
    nu2 = 5


def dk_drho(rho, variance, nu2):
    """dk / drho at rho = r^2 (with the 1e-12 inside): -(3/2) variance exp(-a) | -(5/6) variance (1 + a) exp(-a)."""
    a = np.sqrt(nu2 * np.asarray(rho, np.float64))
    return -1.5 * variance * np.exp(-a) if nu2 == 3 else -(5.0 / 6.0) * variance * (1.0 + a) * np.exp(-a)


def torch_gram(A, B, variance, ls, nu2):
    import torch
    rho = torch.cdist(A / ls, B / ls, compute_mode="donot_use_mm_for_euclid_dist") ** 2 + 1e-12
    a = math.sqrt(nu2) * torch.sqrt(rho)
    return variance * ((1.0 + a) if nu2 == 3 else (1.0 + a + a * a / 3.0)) * torch.exp(-a)


def torch_forward(spec, X, Y, zs, x_leaf=False, likelihood="multiclass", s2=None):
    """dict(elbo, leaves [{name: tensor}] per layer, mean, var [S, N, R] of the head, data [N] the per-image data term
    1/S sum_s E_q[log p(y_n | f_sn)], X the input tensor (a leaf when x_leaf)).  ELBO = num_data / N * sum(data) - KL.
    likelihood: 'multiclass' (Y labels; RobustMax) or 'gaussian' (Y [N, R], variance s2).  Conv layers: spec base 'rbf', 'matern32' or
    'matern52'; the head: ConvKernel on an RBF, as tests/test_oracle_autograd.py's _torch_elbo builds it."""
    import torch
    import test_oracle_autograd as toa
    T, JITTER = toa.T, toa.JITTER
    S, N = spec["S"], X.shape[0]
    Xt = torch.tensor(np.asarray(X, np.float64).reshape(N, -1), dtype=T, requires_grad=bool(x_leaf))
    F = Xt.repeat(S, 1)                                                                      # row s * N + n
    kl = torch.zeros((), dtype=T)
    leaves = []

    def leaf(a):
        return torch.tensor(np.array(a, np.float64), dtype=T, requires_grad=True)
    for li, c in enumerate(spec["convs"]):
        p = dict(Z=leaf(c["Z"]), q_mu=leaf(c["q_mu"]), q_sqrt=leaf(c["q_sqrt"]), variance=leaf(c["variance"]), lengthscales=leaf(c["ls"]))
        leaves.append(p)
        M, R = c["M"], c["R"]
        pt = toa._patches(F.reshape(S * N, c["H"], c["W"], c["C"]), c["f"], c["s"])           # [SN, P, L]
        P = pt.shape[1]
        cols = pt.reshape(S * N * P, -1)
        base = c.get("base", "rbf")
        if base in NU2:
            kern = lambda A, B, p=p, nu2=NU2[base]: torch_gram(A, B, p["variance"], p["lengthscales"], nu2)   # noqa: E731
        else:
            assert base == "rbf", base
            kern = lambda A, B, p=p: toa._rbf(A, B, p["variance"], p["lengthscales"])           # noqa: E731
        Kuu = kern(p["Z"], p["Z"]) + JITTER * torch.eye(M, dtype=T)
        Kuf = kern(p["Z"], cols)
        kff = p["variance"] * torch.ones(cols.shape[0], dtype=T)                               # Stationary.Kdiag
        mean, var = toa._conditional(Kuu, Kuf, kff, p["q_mu"], p["q_sqrt"], c["white"])
        mean, var = mean.reshape(S * N, P * R), var.reshape(S * N, P * R)
        assert c.get("mean_function") is None
        z = torch.tensor(np.asarray(zs[li]).reshape(S * N, P * R), dtype=T)
        F = mean + z * torch.sqrt(var + JITTER)
        Z0 = torch.tensor(np.array(c["Z0"], np.float64), dtype=T)
        Kp = None if c["white"] else kern(Z0, Z0) + JITTER * torch.eye(M, dtype=T)
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
    return dict(elbo=elbo, leaves=leaves, mean=mean.reshape(S, N, -1), var=var.reshape(S, N, -1), data=data, X=Xt)


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


def matern_case(name, base):
    """live_specs.make_case(name) with every conv layer's base kernel set to `base` ('matern32' | 'matern52')."""
    import live_specs as ls
    spec, X, Y, zs = ls.make_case(name)
    for c in spec["convs"]:
        c["base"] = base
    return spec, X, Y, zs

"""Reference for the Matern base kernels of the conv layers (tests/test_host_matern.py, tests/test_gpu_matern.py).

gpflow 1.x ``Matern32`` / ``Matern52`` with ``ARD=False``:

    r = sqrt(|x - z|^2 / l^2 + 1e-12)                     (gpflow's scaled_euclid_dist)
    Matern32: k = variance (1 + a) exp(-a),            a = sqrt(3) r
    Matern52: k = variance (1 + a + a^2 / 3) exp(-a),  a = sqrt(5) r
    Kdiag = variance

* ``Matern32`` / ``Matern52``: NumPy classes with ``K(A, B=None)``, ``Kdiag`` and ``variance`` -- for the operator tests and for handing
  to the oracle's layer classes, as ``oracle.gpflow_ref.ArcCosine`` is handed in tests/test_gpu_ops.py::test_acos_conv_layer.  Squared
  distances from explicit differences (no |x|^2 + |z|^2 - 2 x.z cancellation).
* ``torch_gram``: the Gram function tests/torch_ref.py's forward uses for conv layers whose spec carries ``base in {"matern32", "matern52"}``.
  Test infrastructure only: nothing under deepcgp_amd/ imports this file."""
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


def matern_case(name, base):
    """live_specs.make_case(name) with every conv layer's base kernel set to `base` ('matern32' | 'matern52')."""
    import live_specs as ls
    spec, X, Y, zs = ls.make_case(name)
    for c in spec["convs"]:
        c["base"] = base
    return spec, X, Y, zs

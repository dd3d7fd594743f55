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

* ``torch_gram``: the Gram function tests/torch_ref.py's forward uses for conv layers whose spec carries ``base = "acos"``; its leaves per conv
  layer are Z, q_mu, q_sqrt, variance, weight_variances, bias_variance.  The head stays RBF.
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

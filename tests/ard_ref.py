"""Test helper: model cases whose conv layers carry per-dimension (ARD) lengthscales on their RBF base kernel (--ard), and the measures
the ARD tests share.

``ard_case(name)`` is ``live_specs.make_case(name)`` with every conv layer's ``ls`` replaced by the vector
``ls * (0.8 + 0.4 * default_rng(seed).random(L))``, L = f * f * C: the spread of live_specs' dense-head lengthscales.  The torch references of
tests/ (matern_ref, compose_ref, mixing_ref) divide the patches by ``ls`` as it stands, so a vector goes through them unchanged and its
gradient comes back under the key ``lengthscales`` with shape [L].

Used by tests/test_host_ard.py (liveness of the references, flags, builders, checkpoints; no GPU) and tests/test_gpu_ard.py."""
import numpy as np

import live_specs as ls

# the conv layers' lengthscale vectors join the groups live_specs asks a median and a floor share of (the head's scalar cannot)
MEDIAN_GROUPS = ls.MEDIAN_GROUPS + ("lengthscales",)
CAPPED_GROUPS = ls.CAPPED_GROUPS + ("lengthscales",)

CASES = ("small3_M12", "small3_M20", "small3_white_M20", "odd_M33", "mnist3_M72", "ch_M200", "ch_M384", "ch_264_72")
COMPOSE_CASES = ("ch_264_72-softmax3-rbf-conv2d-all", "even_s2-multiclass3-rbf-filter-none", "ch_res-gaussian1-rbf-none-none",
                 "valid2-poisson1-rbf-none-all", "small3_20_40_24-studentt3-rbf-none-alternate")
MIXING_CASES = ("pad_lin", "deep")


def ardify(spec, seed=11):
    """Every conv layer's scalar ``ls`` of ``spec`` becomes the vector ls * (0.8 + 0.4 U(0, 1)), in place; one generator for the whole spec."""
    rng = np.random.default_rng(seed)
    for c in spec["convs"]:
        assert c.get("base", "rbf") == "rbf", c.get("base")
        L = c["f"] * c["f"] * c["C"]
        c["ls"] = float(c["ls"]) * (0.8 + 0.4 * rng.random(L))
    return spec


def ard_case(name, seed=11):
    """(spec, X, Y, zs) of live_specs.make_case(name) with ARD conv layers."""
    spec, X, Y, zs = ls.make_case(name)
    return ardify(spec, seed), X, Y, zs


def assert_live(case, want):
    """live_specs.assert_live with the conv layers' lengthscale vectors among the median and capped groups (the head's is a scalar)."""
    for li, name, top, med, left_out in ls.liveness(want):
        vector = name != "lengthscales" or np.ndim(want[li][name]) > 0
        assert top >= ls.LIVE_MAX, (case, li, name, "max", top)
        if name in MEDIAN_GROUPS and vector:
            assert med >= ls.LIVE_MEDIAN, (case, li, name, "median / max", med)
        if name in CAPPED_GROUPS and vector:
            assert left_out <= ls.LEFT_OUT_CAP, (case, li, name, "share below the entry floor", left_out)


def model_values(model):
    """live_specs.model_values for a model whose conv layers may be ARD: ``lengthscales`` is then the [L] vector."""
    out = []
    for li, l in enumerate(model.layers):
        head = li == len(model.layers) - 1
        kern = l.kern.base_kernel if head else l.base_kernel
        d = dict(Z=np.array(l.feature.Z), q_mu=np.array(l.q_mu), q_sqrt=np.array(l.q_sqrt), variance=float(kern.variance))
        d["lengthscales"] = np.array(kern.lengthscales, np.float64) if getattr(kern, "ARD", False) else float(kern.lengthscales)
        if head:
            d["patch_weights"] = np.array(l.kern.patch_weights)
        out.append(d)
    return out


def rbf_ard_numpy(A, B, variance, lengthscales):
    """k(a, b) = variance exp(-1/2 sum_l (a_l - b_l)^2 / l_l^2) by explicit differences (no |a|^2 + |b|^2 - 2 a.b cancellation)."""
    A, B = np.asarray(A, np.float64) / lengthscales, np.asarray(B, np.float64) / lengthscales
    out = np.empty((A.shape[0], B.shape[0]))
    for i in range(A.shape[0]):
        d = B - A[i]
        out[i] = variance * np.exp(-0.5 * np.einsum("nl,nl->n", d, d))
    return out

"""ArcCosine conv layers at non-unit parameters, the part that needs no GPU: the masked torch reference of tests/acos_ref.py (its diagonal
is the closed form, its gradient is the derivative of its value), the liveness of that reference on the cases tests/test_gpu_acos.py runs on
the device, the spec key ``acos`` in both builders, and the rounding floor of the comparison -- oracle/grad.py against torch autograd."""
import copy
import functools
import math

import numpy as np
import pytest

import acos_ref as ar
import live_specs as ls
import torch_ref as tr

GPU_CASES = ("small3_M20", "small3_white_M20", "odd_M33", "mnist3_M72", "ch_M200", "ch_M384")

# central differences of the masked ELBO: step h = FD_REL_STEP * max|theta| of the group, error relative to the group's largest gradient entry
# (derived in the docstring of test_autograd_is_the_derivative_of_the_masked_forward)
FD_REL_STEP = 1e-4
FD_BOUND = 5e-6


@functools.lru_cache(maxsize=None)
def _case(name):
    pytest.importorskip("torch")
    spec, X, Y, zs = ar.acos_case(name)
    ref = tr.reference(spec, X, Y, zs)
    e_t, want = ref["parts"][0], ref["want"]
    return spec, X, Y, zs, e_t, want


def test_closed_form_diagonal_and_mask():
    """c == 1 on the diagonal, numerically: the unmasked Gram's diagonal is the closed form to 1e-8 variance at several (z, w, b) -- one ulp
    of the cosine is worth ~1e-9 variance there --; the masked Gram carries the closed form exactly, equals the unmasked one off the diagonal,
    and its gradient is finite, zero from the diagonal to Z, w and b, and DIAG per diagonal entry to the variance."""
    torch = pytest.importorskip("torch")
    assert ar.DIAG == 1.0 - math.acos(1e-15 + (1.0 - 2e-15) * 1.0) / math.pi          # the formula's own argument at c = 1
    assert abs(ar.DIAG - (1.0 - math.sqrt(2e-15) / math.pi)) < 1e-10                  # (1 - 1e-15 rounds to 1 - 9 ulp: 5.7e-12 of this)
    rng = np.random.default_rng(0)
    for v, w, b, scale, L in [(1.7, 0.8, 0.3, 1.0, 9), (0.6, 1.3, 26.8, 5.0, 18), (1.4, 0.7, 200.0, 30.0, 250), (2.0, 1e-3, 1e-3, 1.0, 25),
                              (0.5, 40.0, 1e-2, 0.1, 16)]:
        Z = scale * rng.standard_normal((40, L))
        t = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (Z, v, w, b)]
        raw = ar.torch_gram(t[0], t[0], t[1], t[2], t[3], same=False).detach().numpy()
        assert np.all(np.isfinite(raw)), (v, w, b)
        assert np.abs(np.diag(raw) - v * ar.DIAG).max() <= 1e-8 * v, (v, w, b, np.abs(np.diag(raw) - v * ar.DIAG).max())
        K = ar.torch_gram(t[0], t[0], t[1], t[2], t[3], same=True)
        Kn = K.detach().numpy()
        off = ~np.eye(40, dtype=bool)
        assert np.array_equal(np.diag(Kn), np.full(40, v * ar.DIAG)) and np.array_equal(Kn[off], raw[off])
        assert np.abs(Kn - ar.numpy_kuu(Z, v, w, b)).max() <= 1e-13 * v
        g = torch.autograd.grad(torch.diagonal(K).sum(), t, allow_unused=True, retain_graph=True)
        assert g[0] is None or not g[0].numpy().any()
        assert g[1].item() == 40 * ar.DIAG and not g[2].item() and not g[3].item()
        gs = torch.autograd.grad(K.sum(), t)
        assert all(np.all(np.isfinite(x.numpy())) for x in gs)
        # c is homogeneous of degree 0 in (w, b): w dK/dw + b dK/db = 0
        assert abs(w * gs[2].item() + b * gs[3].item()) <= 1e-12 * abs(w * gs[2].item())


def test_spec_key_reaches_both_builders_and_defaults_stay():
    """``acos = (variance, w, b)`` in a conv layer's spec entry: both builders construct the kernel with it; absent, gpflow's (1, 1, 1)."""
    from deepcgp_amd import synthetic as syn
    from deepcgp_amd.layers import ConvLayer
    from oracle_build import oracle_layers
    import deepcgp_amd.models as M
    spec = syn.make_spec((12, 12, 1), [(3, 1, 2)], (3, 1), M=6, S=2, seed=4, base_kernel="acos")

    class Stub(ConvLayer):    # (no device: skip the prior factorisation)
        def _build_prior_cholesky(self):
            pass
    real, M.ConvLayer = M.ConvLayer, Stub
    try:
        k0 = M.build_layers_from_spec(spec)[0].base_kernel
        keyed = copy.deepcopy(spec)
        ar.set_acos(keyed["convs"][0], 1.7, 0.8, 0.3)
        k1 = M.build_layers_from_spec(keyed)[0].base_kernel
    finally:
        M.ConvLayer = real
    assert (k0.variance, k0.weight_variances, k0.bias_variance) == (1.0, 1.0, 1.0)
    assert (k1.variance, k1.weight_variances, k1.bias_variance) == (1.7, 0.8, 0.3) and k1._describe() == [1.0, 1.7, 0.8, 0.3]
    o0, o1 = oracle_layers(spec)[0].base_kernel, oracle_layers(keyed)[0].base_kernel
    assert (o0.variance, o0.weight_variances, o0.bias_variance) == (1.0, 1.0, 1.0)
    assert (o1.variance, o1.weight_variances, o1.bias_variance) == (1.7, 0.8, 0.3)


def test_case_parameters_differ_from_one_from_each_other_and_between_layers():
    for name in GPU_CASES:
        spec = ar.acos_case(name)[0]
        seen = []
        for c in spec["convs"]:
            v, w, b = c["acos"]
            Z = np.asarray(c["Z"])
            assert c["base"] == "acos" and c["variance"] == v
            assert len({v, w, b, 1.0}) == 4, (name, v, w, b)
            assert 0.3 <= b / (w * np.mean(np.sum(Z * Z, 1))) <= 1.0, (name, b)       # the size of w * mean |z|^2
            seen.append((v, w, b))
            if not c["white"]:
                Lu = np.linalg.cholesky(ar.numpy_kuu(Z, v, w, b) + 1e-3 * np.eye(c["M"]))
                assert np.array_equal(c["q_sqrt"][0], 0.3 * Lu)
        assert all(len({t[i] for t in seen}) == len(seen) for i in range(3)), (name, seen)


@pytest.mark.parametrize("case", GPU_CASES)
def test_reference_gradients_are_live(case):
    """live_specs.assert_live on the reference alone, and weight_variances and bias_variance at or above LIVE_MAX in every conv layer."""
    spec, X, Y, zs, e_t, want = _case(case)
    rows = ls.liveness(want)
    for r in rows:
        print("%s L%d %-17s max %.3e  median / max %.3e  below the entry floor %.3f" % ((case,) + r))
    lo = min(rows, key=lambda r: r[2])
    med = min((r for r in rows if r[1] in ls.MEDIAN_GROUPS), key=lambda r: r[3])
    left = max((r for r in rows if r[1] == "q_sqrt"), key=lambda r: r[4])
    print("TABLE %-17s %-4d %-3d %.1e (L%d %s)  %.1e (L%d %s)  %.3f (L%d)" % (case, spec["head"]["M"], X.shape[0], lo[2], lo[0], lo[1], med[3], med[0],
                                                                            med[1], left[4], left[0]))
    ls.assert_live(case, want)
    for li in range(len(spec["convs"])):
        for name in ("weight_variances", "bias_variance"):
            assert abs(want[li][name]) >= ls.LIVE_MAX, (case, li, name, want[li][name])
        # c depends on (w, b) through b / w alone
        w, b = spec["convs"][li]["acos"][1:]
        assert abs(w * want[li]["weight_variances"] + b * want[li]["bias_variance"]) <= 1e-9 * abs(w * want[li]["weight_variances"]), (case, li)


def _get(l, name):
    return np.array(ar.spec_value(l, name), np.float64)


def _set(l, name, value):
    if name in ar.NAMES and "acos" in l:
        t = list(l["acos"])
        t[ar.NAMES.index(name)] = float(value)
        ar.set_acos(l, *t)
    else:
        l[ls.SPEC_KEY[name]] = float(value) if np.ndim(value) == 0 else value


def _fd(spec, X, Y, zs, li, name, idx, h):
    """Central difference of the masked torch ELBO in entry `idx` of group `name` of layer `li`, step h."""
    import torch
    out = []
    for sgn in (1.0, -1.0):
        s = copy.deepcopy(spec)
        l = (s["convs"] + [s["head"]])[li]
        x = _get(l, name)
        x[idx] += sgn * h
        _set(l, name, x)
        with torch.no_grad():
            out.append(tr.forward(s, X, Y, zs)["elbo"].item())
    return (out[0] - out[1]) / (2.0 * h)


def _fd_entries(name, g, rng, n=3):
    """The largest entry of a group and n - 1 more, drawn from the parameters (q_sqrt: the lower triangle)."""
    g = np.asarray(g, np.float64)
    if g.ndim == 0:
        return [()]
    ok = np.ones(g.shape, bool) if name != "q_sqrt" else np.broadcast_to(np.tril(np.ones(g.shape[1:], bool)), g.shape)
    cand = np.argwhere(ok)
    picks = [np.unravel_index(np.argmax(np.abs(g) * ok), g.shape)]
    picks += [tuple(cand[i]) for i in rng.choice(len(cand), size=n - 1, replace=False)]
    return picks


def test_autograd_is_the_derivative_of_the_masked_forward():
    """Central differences (float64) of the masked torch ELBO against its autograd gradient on three entries of every group of small3_M20,
    the three kernel parameters of both conv layers included.  With the K_uu diagonal a constant the differences are no longer swamped by
    acos(1 - 1e-15).

    Step and bound.  h = r max|theta| of the group; error relative to the group's largest gradient entry, worst over the 18 groups (the
    largest entry of each), measured once:

        r       1e-3     1e-4     1e-5     3e-6     1e-6     1e-7     1e-8
        error   1.3e-5   1.7e-7   2.8e-6   5.4e-6   3.2e-5   2.5e-4   2.7e-3

    Truncation falls as r^2 (13 r^2 of the gradient: 1.3e-5 at 1e-3, so 1.3e-7 at 1e-4), rounding rises as 2.7e-11 / r (|ELBO| = 4.9e5
    carries ~1e-10 of absolute noise per evaluation, divided by 2 h): they cross between r = 1e-4 and 2e-4.  r = 1e-4 is the step; there
    truncation plus rounding is 1.3e-7 + 2.7e-7 = 4e-7, and the bound is about ten times that, 5e-6 -- a twentieth of the 1e-4 the project
    quotes for its finite-difference reach (oracle/__init__.py).  A factor of w, b or variance missing from one group is an error of order
    one on this scale."""
    spec, X, Y, zs, e_t, want = _case("small3_M20")
    rng = np.random.default_rng(5)
    worst = 0.0
    for li, groups in enumerate(want):
        l = (spec["convs"] + [spec["head"]])[li]
        for name, g in groups.items():
            top = np.abs(g).max()
            h = FD_REL_STEP * max(np.abs(_get(l, name)).max(), 1e-3)
            for idx in _fd_entries(name, g, rng):
                fd = _fd(spec, X, Y, zs, li, name, idx, h)
                err = abs(fd - np.asarray(g)[idx]) / top
                worst = max(worst, err)
                print("fd L%d %-17s %-12s autograd % .6e  difference % .6e  err / max %.2e" % (li, name, idx, np.asarray(g)[idx], fd, err))
                assert err <= FD_BOUND, (li, name, idx, fd, np.asarray(g)[idx])
    print("fd WORST %.3e" % worst)


@pytest.mark.parametrize("case", GPU_CASES)
def test_oracle_gradient_against_torch_autograd(case):
    """The comparison floor: oracle/grad.py (hand-written reverse pass, NumPy) against autograd of the masked forward, two independent
    float64 programs, group-wise and entry-wise (live_specs.errors).  The bars are those of tests/test_gpu_acos.py -- a tenth of them here,
    since that module's bounds are ten times this floor and may not pass 1e-7 / 1e-5."""
    from oracle.grad import elbo_and_grad
    from oracle_build import oracle_model
    spec, X, Y, zs, e_t, want = _case(case)
    e_o, g_o = elbo_and_grad(oracle_model(spec, X, Y), X, Y, zs)
    wg = we = 0.0
    for li, groups in enumerate(want):
        assert set(groups) == set(g_o[li]), (case, li)
        for name, w in groups.items():
            eg, ee = ls.errors(name, np.asarray(g_o[li][name], np.float64), w)
            print("%s L%d %-17s group %.3e  entry %.3e" % (case, li, name, eg, ee))
            wg, we = max(wg, eg), max(we, ee)
    print("FLOOR %-17s elbo %.1e  group %.1e  entry %.1e" % (case, abs(e_o - e_t) / abs(e_t), wg, we))
    assert abs(e_o - e_t) <= 1e-10 * abs(e_t), (case, e_o, e_t)
    assert wg <= 1e-8 and we <= 1e-6, (case, wg, we)

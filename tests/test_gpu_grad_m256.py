"""The reverse pass (csrc/grad.hip) and the device optimiser steps at M <= 256 against torch autograd, entry by entry, on specs whose every
gradient group is live.

At M <= 256 a training step takes the route every quoted number runs on: the one-launch strip kernel of the conditional's adjoint
(csrc/conv_bwd_fused.hip, from 4096 columns on for Mp <= 256, R <= 16, unwhitened layers), syrk_kscale_kernel for W_r (128 < M <= 256 and
K >= 8192 columns), the gemm_tn / stacked-k branches of cond_backward_main, head_cond.hip and layer-0 de-duplication.  The gradient tests of
tests/test_gpu_model.py compare that route group-wise, with an absolute fallback, on specs whose reference gradient is dead in most groups
(tests/test_host_grad_m256.py records two of them); this module is tests/test_gpu_grad_large_m.py's scheme on the M <= 256 route.  The
reference is torch.autograd.grad of tests/test_oracle_autograd.py's textbook forward (float64, CPU); the specs are tests/live_specs.py's
CASES_M256.

Liveness (asserted on the reference alone, here and without a GPU in tests/test_host_grad_m256.py): every group |want|max >= 1e-3; Z, q_mu,
patch_weights median >= 1e-6 |want|max; at most half of Z, q_mu, patch_weights, tril(q_sqrt) below the entry floor 1e-6 |want|max.  The
reference's figures, smallest over the layers of a case (group maximum | median / max of Z, q_mu, patch_weights | largest share of tril(q_sqrt)
below the entry floor).  S = 2 except the two ch cases, S = 4 (15 x 4 x 144 = 8640 columns in the conv layer):

    case              M    N   c    a     min group max             min median / max     q_sqrt below floor
    ch_M256           256  15  1.0  0.1   2.4e+01 (L1 lengthscales)  2.0e-03 (L1 Z)       0.004 (L1)
    ch_M200           200  15  1.0  0.1   2.0e+01 (L1 lengthscales)  1.3e-03 (L1 Z)       0.003 (L1)
    ch_white_M256     256  15  1.0  0.1   9.2e-01 (L1 variance)      3.0e-03 (L0 q_mu)    0.033 (L1)
    h_M256            256  8   0.5  0.3   1.6e+01 (L0 variance)      2.8e-03 (L0 Z)       0.000 (L0)
    mnist3_M256       256  3   1.0  0.1   1.6e+00 (L2 variance)      7.1e-04 (L2 Z)       0.052 (L1)
    mnist3_M72        72   3   1.0  0.1   9.3e-01 (L0 Z)             4.6e-04 (L2 Z)       0.025 (L1)
    small3_M20        20   3   1.0  0.1   1.9e+00 (L2 variance)      1.9e-02 (L1 Z)       0.000 (L0)
    small3_white_M20  20   3   1.0  0.1   2.0e-03 (L0 lengthscales)  4.3e-02 (L2 q_mu)    0.001 (L2)
    small3_M12        12   4   1.0  0.1   6.3e+00 (L2 variance)      1.3e-03 (L2 Z)       0.001 (L2)
    odd_M33           33   5   1.0  0.1   7.6e+01 (L0 variance)      1.0e-02 (L1 Z)       0.002 (L1)
    additive_M24      24   3   1.0  0.1   1.2e+01 (L0 variance)      1.4e-02 (L1 q_mu)    0.002 (L1)
    dense_ard_M24     24   3   1.0  0.1   1.2e+01 (L0 variance)      5.9e-03 (L1 Z)       0.001 (L1)
    conv2d_mean_M24   24   3   1.0  0.1   1.2e+01 (L1 variance)      2.2e-02 (L1 q_mu)    0.002 (L1)

small3_M12 (12 x 12 x 1 images, small3's layers) is the case at M <= 16: the K_uf adjoint (csrc/grad.hip, kuf_adjoint) then runs on one row chunk
and writes its column sums without the second launch.  The last three are the model variants the textbook forward supports (12 x 12 x 1 images, conv (3, 1, 3), head (3, 1)): the additive head,
the dense RBF(ARD) head, Conv2dMean.  The arc-cosine base kernel has this module's scheme in tests/test_gpu_acos.py, at non-unit variance,
weight_variances and bias_variance: its reference (tests/acos_ref.py) has leaves for all three and writes K_uu's diagonal as the closed
form of the variance alone, so autograd never differentiates acos at the coincident points (slope 2e7 at 1 - 1e-15).

Rounding floor of the comparison: oracle/grad.py against torch autograd, two independent float64 implementations, on every case on the CPU.
Largest error over the groups of a case, group-wise (|a - b|max / |want|max) / entry-wise (|a - b| / |want| over the entries with
|want| >= 1e-6 |want|max):

    ch_M256 2.6e-11 / 5.3e-7      ch_M200 2.0e-11 / 2.2e-8      ch_white_M256 2.4e-11 / 2.9e-8    h_M256 2.9e-11 / 1.8e-8
    mnist3_M256 5.9e-10 / 3.3e-7  mnist3_M72 7.7e-11 / 6.2e-9   small3_M20 3.5e-13 / 3.4e-10      small3_white_M20 1.0e-11 / 3.8e-11
    odd_M33 2.6e-12 / 7.4e-9      additive_M24 4.0e-12 / 3.5e-9 dense_ard_M24 1.1e-12 / 6.2e-10   conv2d_mean_M24 4.9e-12 / 4.2e-10
    small3_M12 4.8e-12 / 5.4e-9

TOL_E = ten times the largest entry-wise floor = 5.3e-6, inside the 1e-5 it may not exceed (no case needed its c moved).

Largest device-vs-autograd error seen per case on an MI355X, over all the routes the case runs (group-wise / entry-wise):

    ch_M256 3.1e-11 / 3.3e-7      ch_M200 8.6e-12 / 4.1e-8      ch_white_M256 1.3e-12 / 1.8e-8    h_M256 2.7e-11 / 7.3e-9
    mnist3_M256 3.1e-9 / 1.8e-7   mnist3_M72 2.0e-11 / 5.4e-9   small3_M20 5.1e-13 / 2.9e-11      small3_white_M20 3.3e-11 / 3.3e-11
    odd_M33 6.2e-12 / 6.4e-9      additive_M24 1.1e-11 / 2.9e-9 dense_ard_M24 1.4e-12 / 3.0e-10   conv2d_mean_M24 5.3e-12 / 2.6e-10
    small3_M12 4.3e-12 / 4.0e-9
"""
import copy
import functools

import numpy as np
import pytest

from deepcgp_amd import synthetic as syn
from deepcgp_amd.models import build_from_spec
import live_specs as ls

pytestmark = pytest.mark.gpu

TOL_GROUP = 1e-7         # |got - want|max <= TOL_GROUP * |want|max, every group of every layer, no absolute fallback
TOL_E = 5.3e-6           # entry-wise: 10 x the largest oracle-vs-autograd floor of the module docstring


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(spec, X, Y, zs, e_t, want): the case and its torch reference, computed once per process; liveness asserted before anything else."""
    pytest.importorskip("torch")
    spec, X, Y, zs = ls.make_case(name)
    assert spec["head"]["M"] <= 256
    e_t, want = ls.torch_reference(spec, X, Y, zs)
    ls.assert_live(name, want)
    return spec, X, Y, zs, e_t, want


CH = ("ch_M256", "ch_M200")
UNDER_4096 = ("mnist3_M256", "mnist3_M72", "small3_M20", "odd_M33")       # every layer under the strip kernel's 4096 columns
# (case, ctx options, dedup_layer0): every route is compared with autograd, not only with another route
PARITY = ([(c, {}, False) for c in ls.CASES_M256]
          + [(c, dict(no_fused_bwd=1), False) for c in CH]                 # the launch-per-product adjoint where the default is the strip kernel
          + [(c, dict(fused_bwd_min_cols=0), False) for c in UNDER_4096]   # the strip kernel forced (conv layers and head)
          + [(c, dict(no_syrk=1), False) for c in CH]                      # W_r through the general GEMM
          + [(c, {}, True) for c in ("ch_M256", "h_M256", "mnist3_M72")]   # layer-0 de-duplication against the tiled reference
          + [("ch_M200", dict(grad_nofork=1), False)])                     # the reverse pass on one stream


def _route_id(case, opts, dedup):
    return "-".join([case] + ["%s=%d" % kv for kv in opts.items()] + (["dedup"] if dedup else []))


@pytest.mark.parametrize("case,opts,dedup", PARITY, ids=[_route_id(*p) for p in PARITY])
def test_gradient_matches_torch_autograd_up_to_M256(ctx, case, opts, dedup):
    """ELBO to 1e-9, every group of every layer group-wise to 1e-7 of the group's maximum and entry-wise to TOL_E over the entries at or
    above the floor, the device's q_sqrt gradient exactly zero above the diagonal, and the same bits when the step is repeated."""
    spec, X, Y, zs, e_t, want = _case(case)
    tag = _route_id(case, opts, dedup)
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    with ctx.options(**opts):
        e, grads = model.compute_gradients(X, Y, zs=zs)
        e2, grads2 = model.compute_gradients(X, Y, zs=zs)
    rows = []
    for li, groups in enumerate(want):
        assert set(groups) == set(grads[li]), (tag, li)
        for name, w in groups.items():
            got = np.asarray(grads[li][name], np.float64)
            rows.append((li, name) + ls.errors(name, got, w))
            print("%s L%d %-14s group %.3e  entry %.3e  |want|max %.3e" % ((tag,) + rows[-1] + (np.abs(w).max(),)))
    print("%s elbo rel %.3e  WORST group %.3e entry %.3e" % (tag, abs(e - e_t) / abs(e), max(r[2] for r in rows), max(r[3] for r in rows)))
    assert abs(e - e_t) <= 1e-9 * abs(e), (tag, e, e_t)
    for li, name, err_g, err_e in rows:
        assert err_g <= TOL_GROUP, (tag, li, name, "group-wise", err_g)
        assert err_e <= TOL_E, (tag, li, name, "entry-wise", err_e)
    for li, g in enumerate(grads):
        assert not np.triu(g["q_sqrt"], 1).any(), (tag, li, "q_sqrt above the diagonal")
    assert e == e2
    for li, (a, b) in enumerate(zip(grads, grads2)):
        for name in a:
            assert np.array_equal(a[name], b[name]), (tag, li, name, "repeat")
    model.close()


# (case, ctx options, whether the strip kernel must launch)
ROUTES = ([(c, {}, True) for c in CH] + [(c, dict(no_fused_bwd=1), False) for c in CH]
          + [(c, dict(fused_bwd_min_cols=0), True) for c in UNDER_4096] + [(c, {}, False) for c in UNDER_4096])


@pytest.mark.parametrize("case,opts,strip", ROUTES, ids=[_route_id(c, o, False) for c, o, _ in ROUTES])
def test_the_route_is_the_one_taken(ctx, case, opts, strip):
    """The launch counts of one reverse pass (ctx.timing): on the two ch cases the default options launch the strip kernel (family
    conv_bwd_fused) and the conv layer's W_r contraction (grad_wr), no_fused_bwd = 1 launches no strip kernel; on the cases under 4096 columns
    the strip kernel runs only when fused_bwd_min_cols = 0 forces it.  No timer family tells syrk_kscale_kernel from the general GEMM inside
    grad_wr, so that W_r took the kernel is not asserted from the counts: the ch cases have the shape its condition asks for (128 < M <= 256,
    K = 8640 >= 8192 columns; tests/test_host_grad_m256.py), and the no_syrk = 1 route above is compared with autograd on its own.  What stays
    unseen: the other conditions of syrk_applies (even leading dimension and batch stride, a 16-byte aligned operand, batch <= 64) are not
    checked, so a quiet fall-back of W_r to the general GEMM would pass every test of this module."""
    spec, X, Y, zs = ls.make_case(case)
    model = build_from_spec(spec, X, Y)
    with ctx.options(**opts):
        model.compute_gradients(X, Y, zs=zs)          # first call: allocations
        ctx.timing_enable(1)
        ctx.timing_reset()
        try:
            model.compute_gradients(X, Y, zs=zs)
            tim = ctx.timing()
        finally:
            ctx.timing_enable(0)
    n_strip, n_wr = tim.get("conv_bwd_fused", (0, 0.0))[0], tim.get("grad_wr", (0, 0.0))[0]
    print("%s launches: conv_bwd_fused %d  grad_wr %d  grad_wr_head %d" % (_route_id(case, opts, False), n_strip, n_wr,
                                                                       tim.get("grad_wr_head", (0, 0.0))[0]))
    assert (n_strip > 0) if strip else (n_strip == 0), (case, opts, n_strip)
    assert n_wr > 0, (case, opts, n_wr)
    model.close()


def test_sgd_step_follows_the_torch_gradient_at_M200(ctx):
    """One sgd_step(lr) on ch_M200: Z, q_mu, q_sqrt = theta + lr * (torch gradient), variance and lengthscale by the softplus update of
    test_sgd_natgrad_and_trainable_flags (1), all to 1e-9 relative."""
    spec, X, Y, zs, _, want = _case("ch_M200")
    # lr * |want|max is 1.4e-4 (head lengthscale) to 0.2 (head q_mu) of the group's largest parameter.  Asserted below at 1e-5: with the
    # 1e-9 bar on the result the gradient itself is then pinned to 1e-4 of its maximum or better -- a step that moves nothing checks nothing.
    lr = 1e-4
    model = build_from_spec(spec, X, Y)
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.sgd_step(lr)
    model.pull_parameters()
    for li, (l, now) in enumerate(zip(spec["convs"] + [spec["head"]], ls.model_values(model))):
        for name, w in want[li].items():
            x = np.asarray(l[ls.SPEC_KEY[name]], np.float64)
            if name in ls.POSITIVE:
                u = ls.softplus_inv(x) + lr * w * (1.0 - np.exp(-(x - 1e-6)))
                expect = np.log1p(np.exp(u)) + 1e-6
            else:
                expect = x + lr * w
            err = rel(now[name], expect)
            print("sgd L%d %-14s rel %.3e  (moved %.3e)" % (li, name, err, rel(expect, x)))
            assert rel(expect, x) >= 1e-5, (li, name, "the step moves the group too little to check its gradient", rel(expect, x))
            assert err < 1e-9, (li, name, err)
    model.close()


def _prior(l):
    Zp = np.asarray(l.get("Z0", l["Z"]), np.float64)          # conv layers: the frozen prior patches; the head: its live Z
    return syn._rbf(Zp, Zp, l["variance"], l["ls"]) + syn.JITTER * np.eye(l["M"])


def test_natgrad_step_matches_numpy_on_torch_gradients_at_M200(ctx):
    """(a) One natgrad_step on the real objective of ch_M200 against tests/natgrad_ref.py fed with the TORCH gradients, rel < 1e-8.
    gamma = 1e-5: the data term is scaled by num_data / N = 4000, and on the CPU the NumPy restatement itself leaves the positive-definite
    cone in the head at 1e-4 (it holds at 3e-5; 1e-5 keeps a factor of three from that edge and still moves the head's q_mu by 0.99 and its
    q_sqrt by 0.08 of their maxima, the conv layer's by 1.8e-2 and 2.8e-4).
    (b) Conjugacy: with scale = 0 the objective is -KL[q || prior], so one step with gamma = 1 lands on the prior.  The bound is ten times
    the residual natgrad_ref.py itself reaches from the torch gradient of the same objective in float64 (the larger of the two layers;
    measured on the CPU: |q_mu|max 5.6e-12 .. 8.4e-12, rel(q_sqrt q_sqrt^T, K) 8.6e-12 .. 1.2e-11 with the BLAS thread count; the device
    reached 8.7e-12 and 2.3e-11)."""
    from natgrad_ref import natgrad_reference
    spec, X, Y, zs, _, want = _case("ch_M200")
    layers = spec["convs"] + [spec["head"]]
    model = build_from_spec(spec, X, Y)
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.natgrad_step(1e-5)
    model.pull_parameters()
    for li, (l, m) in enumerate(zip(layers, model.layers)):
        mu1, L1 = natgrad_reference(np.asarray(l["q_mu"]), np.asarray(l["q_sqrt"]), want[li]["q_mu"], want[li]["q_sqrt"], 1e-5)
        print("natgrad L%d rel q_mu %.3e q_sqrt %.3e (moved %.3e / %.3e)" % (li, rel(m.q_mu, mu1), rel(m.q_sqrt, L1), rel(mu1, l["q_mu"]),
                                                                           rel(L1, l["q_sqrt"])))
        assert rel(m.q_mu, mu1) < 1e-8 and rel(m.q_sqrt, L1) < 1e-8, (li, rel(m.q_mu, mu1), rel(m.q_sqrt, L1))
    model.close()
    # (b)
    kl_only = copy.deepcopy(spec)
    kl_only["num_data"] = 0                                   # the torch forward's scale is num_data / N
    _, g0 = ls.torch_reference(kl_only, X, Y, zs)
    res_mu = res_S = 0.0
    for li, l in enumerate(layers):
        mu1, L1 = natgrad_reference(np.asarray(l["q_mu"]), np.asarray(l["q_sqrt"]), g0[li]["q_mu"], g0[li]["q_sqrt"], 1.0)
        K = _prior(l)
        res_mu = max(res_mu, np.abs(mu1).max())
        res_S = max(res_S, max(rel(L1[r] @ L1[r].T, K) for r in range(L1.shape[0])))
    print("natgrad conjugacy, NumPy restatement: |q_mu|max %.3e  rel(S, K) %.3e" % (res_mu, res_S))
    model = build_from_spec(spec, X, Y)
    model.compute_gradients(X, Y, zs=zs, scale=0.0, fetch=False)
    model.natgrad_step(1.0)
    model.pull_parameters()
    dev = [(np.abs(m.q_mu).max(), max(rel(m.q_sqrt[r] @ m.q_sqrt[r].T, _prior(l)) for r in range(m.q_sqrt.shape[0])))
           for l, m in zip(layers, model.layers)]
    for li, (dmu, dS) in enumerate(dev):
        print("natgrad conjugacy, device L%d: |q_mu|max %.3e  rel(S, K) %.3e" % (li, dmu, dS))
    for li, (dmu, dS) in enumerate(dev):
        assert dmu <= 10.0 * res_mu and dS <= 10.0 * res_S, (li, dmu, dS, res_mu, res_S)
    model.close()


def test_adam_one_call_steps_match_numpy_on_torch_gradients_at_M200(ctx):
    """Three steps of dcgp_model_train_step_adam on ch_M200 against NumPy Adam on torch gradients recomputed after every step: the scheme
    and the tolerances of test_adam_steps_match_numpy_on_oracle_gradients."""
    spec, X, Y, zs, _, _ = _case("ch_M200")
    spec = copy.deepcopy(spec)
    N, lr, state = X.shape[0], 0.05, {}
    model = build_from_spec(spec, X, Y)
    for t in range(1, 4):
        z = syn.make_noise(spec, N, seed=100 + t)
        e = model.train_step(X, Y, lr, zs=z, t=t)
        e_t, g = ls.torch_reference(spec, X, Y, z)
        print("adam t%d elbo rel %.3e" % (t, abs(e - e_t) / abs(e_t)))
        assert abs(e - e_t) <= 1e-8 * abs(e_t), (t, e, e_t)
        ls.adam_numpy_step(spec, g, state, lr, t)
    model.pull_parameters()
    rows = []
    for li, (l, now) in enumerate(zip(spec["convs"] + [spec["head"]], ls.model_values(model))):
        for name in now:
            rows.append((li, name, rel(now[name], l[ls.SPEC_KEY[name]])))
            print("adam L%d %-14s rel %.3e" % rows[-1])
    for li, name, err in rows:
        assert err < (1e-8 if name in ls.POSITIVE else 1e-7), (li, name, err)
    model.close()

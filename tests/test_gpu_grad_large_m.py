"""The reverse pass (csrc/grad.hip) and the device optimiser steps at M > 256 against torch autograd, on specs whose every gradient group is live.

Above M = 256 a training step takes other code than every gradient test of tests/test_gpu_model.py: K_uf through the sweep + GEMM route, the
head conditional off head_cond.hip above 512, the conditional's adjoint launch per product (conv_bwd_fused.hip refuses Mp > 256), W_r through
the general GEMM (syrk_kscale_kernel refuses), and kuu_backward / kl_products / kl_apply / NatGrad on the 12- / 32-panel factorisation chain,
with padded rows and a ragged last panel at M = 1000 (Mp = 1008).  The reference is torch.autograd.grad of tests/test_oracle_autograd.py's
textbook forward (float64, CPU); the specs come from tests/live_specs.py, whose docstring says why they are not make_config's.

Liveness (asserted on the reference alone, here and without a GPU in tests/test_host_grad_large_m.py): every group |want|max >= 1e-3; Z, q_mu,
patch_weights median >= 1e-6 |want|max; at most half of Z, q_mu, patch_weights, tril(q_sqrt) below the entry floor 1e-6 |want|max.  The
reference's figures, smallest over the layers of a case (group maximum | median / max of Z, q_mu, patch_weights | largest share of tril(q_sqrt)
below the entry floor):

    case            c    a     min group max           min median / max       q_sqrt below floor
    ch_M1024        0.7  0.1   1.9e+02 (L0 q_sqrt)        9.3e-04 (L1 Z)         0.034 (L1)
    ch_M1000        0.7  0.1   6.7e+01 (L1 lengthscales)  9.9e-04 (L1 Z)         0.060 (L1)
    h_M1024         0.5  0.3   1.8e+02 (L0 patch_weights) 3.3e-03 (L0 Z)         0.006 (L0)
    cifar3_M384     1.0  0.1   2.1e-01 (L0 Z)             7.6e-04 (L1 Z)         0.301 (L1)
    mnist3_M320     1.0  0.1   1.8e+00 (L2 lengthscales)  1.1e-03 (L2 Z)         0.061 (L1)
    ch_white_M384   1.0  0.1   4.8e+00 (L0 lengthscales)  2.3e-03 (L1 q_mu)      0.113 (L1)
    ch_M384         1.0  0.1   9.3e+01 (L1 lengthscales)  1.1e-03 (L1 Z)         0.027 (L1)

cifar3_M384 is the cfg4 geometry itself (32 x 32 x 3, convs (4, 2, 10), (5, 1, 10), head (5, 1)): with the lengthscale tied to the norm of
each layer's own inducing patches it is inside the bounds, no substitute geometry was needed.

Rounding floor of the comparison: oracle/grad.py against torch autograd, two independent float64 implementations, on the same cases on the
CPU (the oracle takes 1 - 10 s per case, so all seven were measured).  Largest error over the groups of a case, group-wise
(|a - b|max / |want|max) and entry-wise (|a - b| / |want| over the entries with |want| >= 1e-6 |want|max):

    ch_M1024 2.5e-11 / 4.0e-7    ch_M1000 3.2e-11 / 7.6e-7    h_M1024 2.5e-11 / 1.9e-7    cifar3_M384 2.4e-10 / 4.0e-7
    mnist3_M320 8.8e-11 / 2.8e-7    ch_M384 1.1e-11 / 1.0e-7    ch_white_M384 2.9e-12 / 3.3e-8

The entry-wise floor grows with the conditioning of K_uu (at c = 1.0 the M = 1000 / 1024 cases gave 4.7e-6 / 3.3e-6 and the head-only case
2.9e-5: the constants above were chosen on the CPU for a floor below 1e-6, before the device was consulted).  TOL_E = ten times the largest
= 7.6e-6, inside the 1e-5 it may not exceed.

Largest device-vs-autograd error seen per case on an MI355X, with and without dedup_layer0 (group-wise / entry-wise; every figure is printed
before it is asserted, run with -s):

    ch_M1024 7.1e-11 / 7.3e-7    ch_M1000 9.9e-11 / 5.1e-7    h_M1024 1.6e-11 / 7.9e-8    cifar3_M384 3.5e-10 / 5.6e-7
    mnist3_M320 9.8e-11 / 2.7e-7    ch_M384 2.0e-11 / 2.3e-7    ch_white_M384 6.0e-12 / 2.3e-8
"""
import copy
import functools

import numpy as np
import pytest

from deepcgp_amd import synthetic as syn
from deepcgp_amd.models import build_from_spec
import live_specs as ls

pytestmark = pytest.mark.gpu

TOL_GROUP = 1e-7         # |got - want|max <= TOL_GROUP * |want|max, every group of every layer
TOL_E = 7.6e-6           # entry-wise: 10 x the largest oracle-vs-autograd floor of the module docstring


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(spec, X, Y, zs, e_t, want): the case and its torch reference, computed once per process; liveness asserted before anything else."""
    pytest.importorskip("torch")
    spec, X, Y, zs = ls.make_case(name)
    e_t, want = ls.torch_reference(spec, X, Y, zs)
    ls.assert_live(name, want)
    return spec, X, Y, zs, e_t, want


PARITY = [("ch_M1024", False), ("ch_M1000", False), ("h_M1024", False), ("h_M1024", True), ("cifar3_M384", False), ("mnist3_M320", False),
          ("ch_white_M384", False), ("ch_M384", False), ("ch_M384", True)]


@pytest.mark.parametrize("case,dedup", PARITY, ids=["%s%s" % (c, "-dedup" if d else "") for c, d in PARITY])
def test_gradient_matches_torch_autograd_above_M256(ctx, case, dedup):
    """ELBO to 1e-9, every group of every layer group-wise to 1e-7 of the group's maximum and entry-wise to TOL_E over the entries at or
    above the floor, the device's q_sqrt gradient exactly zero above the diagonal, and the same bits when the step is repeated.
    ``dedup``: dedup_layer0 (the first layer on the distinct images only, as the training loop runs it) against the tiled reference."""
    spec, X, Y, zs, e_t, want = _case(case)
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    e, grads = model.compute_gradients(X, Y, zs=zs)
    e2, grads2 = model.compute_gradients(X, Y, zs=zs)
    rows = []
    for li, groups in enumerate(want):
        assert set(groups) == set(grads[li]), (case, li)
        for name, w in groups.items():
            got = np.asarray(grads[li][name], np.float64)
            rows.append((li, name) + ls.errors(name, got, w))
            print("%s%s L%d %-14s group %.3e  entry %.3e  |want|max %.3e" % ((case, "-dedup" if dedup else "") + rows[-1] + (np.abs(w).max(),)))
    print("%s%s elbo rel %.3e  WORST group %.3e entry %.3e" % (case, "-dedup" if dedup else "", abs(e - e_t) / abs(e),
                                                           max(r[2] for r in rows), max(r[3] for r in rows)))
    assert abs(e - e_t) <= 1e-9 * abs(e), (case, e, e_t)
    for li, name, err_g, err_e in rows:
        assert err_g <= TOL_GROUP, (case, li, name, "group-wise", err_g)
        assert err_e <= TOL_E, (case, li, name, "entry-wise", err_e)
    for li, g in enumerate(grads):
        assert not np.triu(g["q_sqrt"], 1).any(), (case, li, "q_sqrt above the diagonal")
    assert e == e2
    for li, (a, b) in enumerate(zip(grads, grads2)):
        for name in a:
            assert np.array_equal(a[name], b[name]), (case, li, name, "repeat")
    model.close()


def test_sgd_step_follows_the_torch_gradient_at_M384(ctx):
    """One sgd_step(lr) at M = 384: Z, q_mu, q_sqrt = theta + lr * (torch gradient), variance and lengthscale by the softplus update of
    test_sgd_natgrad_and_trainable_flags (1), all to 1e-9 relative."""
    spec, X, Y, zs, _, want = _case("ch_M384")
    lr = 1e-4           # lr * |want|max is 0.06 - 0.6 of a parameter here: far above 1e-9 of it, so the gradient is what is checked
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
            print("sgd L%d %-14s rel %.3e" % (li, name, err))
            assert err < 1e-9, (li, name, err)
    model.close()


def _prior(l):
    Zp = np.asarray(l.get("Z0", l["Z"]), np.float64)          # conv layers: the frozen prior patches; the head: its live Z
    return syn._rbf(Zp, Zp, l["variance"], l["ls"]) + syn.JITTER * np.eye(l["M"])


def test_natgrad_step_matches_numpy_on_torch_gradients_at_M384(ctx):
    """(a) One natgrad_step on the real objective against tests/natgrad_ref.py fed with the TORCH gradients, rel < 1e-8.  gamma = 1e-5: the
    data term is scaled by num_data / N = 15 000, and from 1e-4 on the NumPy restatement itself leaves the positive-definite cone in the head.
    (b) Conjugacy: with scale = 0 the objective is -KL[q || prior], so one step with gamma = 1 lands on the prior.  The bound is ten times
    the residual natgrad_ref.py itself reaches from the torch gradient of the same objective in float64 (the larger of the two layers;
    measured on the CPU: |q_mu|max 3.4e-11, rel(q_sqrt q_sqrt^T, K) 4.4e-11)."""
    from natgrad_ref import natgrad_reference
    spec, X, Y, zs, _, want = _case("ch_M384")
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


def test_adam_one_call_steps_match_numpy_on_torch_gradients_at_M384(ctx):
    """Three steps of dcgp_model_train_step_adam at M = 384 against NumPy Adam on torch gradients recomputed after every step: the scheme
    and the tolerances of test_adam_steps_match_numpy_on_oracle_gradients.  (The same three steps on oracle/grad.py's gradients instead of
    torch's end within 2.8e-8 of these on the CPU, q_sqrt the largest: Adam's m / (sqrt(v) + 1e-8) magnifies rounding in the few
    q_sqrt entries whose gradient is below 1e-6.)"""
    spec, X, Y, zs, _, _ = _case("ch_M384")
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

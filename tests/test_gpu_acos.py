"""ArcCosine(order 0) conv layers (--base-kernel acos) on the device at NON-UNIT variance, weight_variances and bias_variance: the reverse pass
(acos_e_form_kernel, acos_divide_kernel, acos_kuu_backward_kernel, the rs2 / acos_w arguments of patch_backward, the P2_SLOT sums), the two
extra optimiser slots, the data path and the forward's acos epilogues against torch autograd of tests/acos_ref.py's textbook forward
(float64, CPU), entry by entry.  tests/test_gpu_grad_m256.py's scheme; every other model-level ArcCosine test runs at (1, 1, 1), where a
missing or doubled factor of w, b or variance is invisible.

The reference writes K_uu's diagonal as the closed form variance (1 - acos(1 - 1e-15) / pi) of the variance leaf alone (c == 1 there
identically in z, w, b), so it needs no hand-written diagonal skip.  The device and the oracle write the same constant (BaseKernel::eval_diag,
oracle/gpflow_ref.py): evaluated from the rounded cosine the entry moves by ~1e-9 variance per ulp, which inv(K_uu) amplified into a floor
of 1.4e-7 group-wise / 6.3e-4 entry-wise between the oracle and autograd on these very cases -- above any bar this module may hold.

Cases: tests/live_specs.py's, through acos_ref.acos_case: layer i has (variance, w) = (1.7, 0.8), (0.6, 1.3) and b = (0.5, 0.8) x w x mean|z|^2
of its own inducing patches.  Liveness of the reference (tests/test_host_acos.py; smallest group maximum | smallest median / max of Z, q_mu,
patch_weights | largest share of tril(q_sqrt) below the entry floor); c = 1.0, a = 0.1, S = 2 (ch_M200: S = 4) everywhere:

    case              M    N   min group max             min median / max   q_sqrt below floor
    small3_M20        20   3   4.6e-01 (L1 bias_variance)  5.8e-02 (L1 Z)     0.000 (L0)
    small3_white_M20  20   3   1.0e-02 (L0 bias_variance)  3.8e-02 (L0 q_mu)  0.000 (L2)
    odd_M33           33   5   7.2e+00 (L0 bias_variance)  1.2e-02 (L1 Z)     0.001 (L1)
    mnist3_M72        72   3   1.7e-02 (L0 Z)              4.8e-04 (L2 Z)     0.033 (L0)
    ch_M200           200  15  5.4e+00 (L0 Z)              1.6e-03 (L1 Z)     0.002 (L1)
    ch_M384           384  4   3.3e+01 (L0 q_sqrt)         1.2e-03 (L1 Z)     0.022 (L1)

Routes.  The kernel-specific code sits behind the conditional's adjoint: every option of tests/test_gpu_grad_m256.py's PARITY changes how
dK_uf, S = d ELBO / d K_uu or the layer's rows reach it, so each is a row here.  The strip kernel (conv_bwd_fused.hip) is kernel-agnostic
(unwhitened, Mp <= 256, R <= 16, from 4096 columns on): ch_M200 takes it by default, no_fused_bwd = 1 takes it away, fused_bwd_min_cols = 0
forces it on the unwhitened cases under 4096 columns (never on a whitened layer: no row for small3_white_M20).  syrk_kscale_kernel forms W_r at
128 < M <= 256 and 8192 columns: ch_M200 only.  dedup_layer0 feeds the first layer N rows instead of S N.  ch_M384 is the M > 256 route.
The one route an ArcCosine layer never takes is the input gradient's fused patch adjoint (input_grad.hip: RBF only).

Rounding floor: oracle/grad.py against autograd, two independent float64 programs, on the CPU (tests/test_host_acos.py; ELBO relative /
group-wise / entry-wise), the bound, and the largest device-vs-autograd error seen on an MI355X over all the routes of the case:

    case              floor                          bound                  device
    small3_M20        1.2e-16 / 2.6e-13 / 1.2e-11    1e-9 / 1e-7 / 1.5e-6   1.2e-16 / 1.4e-12 / 2.8e-11
    small3_white_M20  0.0e+00 / 2.5e-11 / 2.5e-11    1e-9 / 1e-7 / 1.5e-6   0.0e+00 / 4.9e-12 / 1.0e-11
    odd_M33           4.7e-16 / 2.7e-12 / 3.6e-09    1e-9 / 1e-7 / 1.5e-6   1.5e-15 / 1.7e-11 / 2.5e-09
    mnist3_M72        1.2e-15 / 1.9e-10 / 1.7e-08    1e-9 / 1e-7 / 1.5e-6   9.7e-15 / 7.9e-11 / 1.1e-08
    ch_M200           7.1e-16 / 5.5e-11 / 5.4e-08    1e-9 / 1e-7 / 1.5e-6   1.7e-15 / 9.2e-11 / 3.0e-08
    ch_M384           5.7e-15 / 1.1e-11 / 1.5e-07    1e-9 / 1e-7 / 1.5e-6   5.7e-15 / 1.5e-11 / 1.7e-07

TOL_E = ten times the largest entry-wise floor = 1.5e-6, inside the 1e-5 it may not exceed; ten times the largest group-wise floor is 1.9e-9 and
the bar is the 1e-7 of the other three kernels; the ELBO bar is 1e-9.  No bar is lifted and no case needed its constants moved.

Also seen there: three Adam steps within 7.2e-14 (the six kernel parameters bit for bit), the SGD step 2.5e-14, the NatGrad step 1.8e-14; the
input gradient within 7.6e-16 absolute (|dX|max 3.5e-5 .. 1.4e-3), J 3.6e-14; head marginals 8.3e-13; forward ELBO 5.7e-15.  Sensitivity
(scratch builds): d/dw multiplied by acos_w once more fails small3_M20 at L0 weight_variances, 1.4e-2 group-wise; patch_backward without its
acos_w argument fails it at L0 Z, 0.26 group-wise, and every input-gradient case (1.4e-6 .. 3.6e-4 absolute against the 1e-7 bar).
"""
import copy
import functools

import numpy as np
import pytest

from deepcgp_amd import synthetic as syn
from deepcgp_amd.models import build_from_spec
import acos_ref as ar
import live_specs as ls
import torch_ref as tr

pytestmark = pytest.mark.gpu

TOL_ELBO = 1e-9
TOL_GROUP = 1e-7         # |got - want|max <= TOL_GROUP * |want|max, every group of every layer, no absolute fallback
TOL_E = 1.5e-6           # entry-wise: 10 x the largest oracle-vs-autograd floor of the module docstring
CASES = ("small3_M20", "small3_white_M20", "odd_M33", "mnist3_M72", "ch_M200", "ch_M384")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(spec, X, Y, zs, e_t, want): the case and its torch reference, computed once per process; liveness asserted before anything else."""
    pytest.importorskip("torch")
    spec, X, Y, zs = ar.acos_case(name)
    ref = tr.reference(spec, X, Y, zs)
    e_t, want = ref["parts"][0], ref["want"]
    ls.assert_live(name, want)
    return spec, X, Y, zs, e_t, want


UNDER_4096 = ("small3_M20", "odd_M33", "mnist3_M72")                      # unwhitened, every layer under the strip kernel's 4096 columns
# (case, ctx options, dedup_layer0): every route is compared with autograd, not only with another route
PARITY = ([(c, {}, False) for c in CASES]
          + [("ch_M200", dict(no_fused_bwd=1), False)]                     # the launch-per-product adjoint where the default is the strip kernel
          + [(c, dict(fused_bwd_min_cols=0), False) for c in UNDER_4096]   # the strip kernel forced
          + [("ch_M200", dict(no_syrk=1), False)]                          # W_r through the general GEMM
          + [(c, {}, True) for c in ("ch_M200", "mnist3_M72")]             # layer-0 de-duplication against the tiled reference
          + [("ch_M200", dict(grad_nofork=1), False)])                     # the reverse pass on one stream


def _route_id(case, opts, dedup):
    return "-".join([case] + ["%s=%d" % kv for kv in opts.items()] + (["dedup"] if dedup else []))


@pytest.mark.parametrize("case,opts,dedup", PARITY, ids=[_route_id(*p) for p in PARITY])
def test_gradient_matches_torch_autograd(ctx, case, opts, dedup):
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
        assert set(groups) == set(grads[li]), (tag, li, sorted(groups), sorted(grads[li]))
        for name, w in groups.items():
            got = np.asarray(grads[li][name], np.float64)
            rows.append((li, name) + ls.errors(name, got, w))
            print("%s L%d %-17s group %.3e  entry %.3e  |want|max %.3e" % ((tag,) + rows[-1] + (np.abs(w).max(),)))
    print("%s elbo rel %.3e  WORST group %.3e entry %.3e" % (tag, abs(e - e_t) / abs(e_t), max(r[2] for r in rows), max(r[3] for r in rows)))
    assert abs(e - e_t) <= TOL_ELBO * abs(e_t), (tag, e, e_t)
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


# ---- the forward at non-unit parameters -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["odd_M33", "ch_M384"])
def test_forward_value_and_layer_moments(ctx, case):
    """One conv layer + head through the fused layer kernel (odd_M33: M = 33, R = 13) and through the M > 256 route (ch_M384): the
    forward-only ELBO and every layer's mean and variance against the torch forward, 1e-9 -- conv_fused.hip's and the sweep's acos epilogues at
    w, b, variance != 1."""
    torch = pytest.importorskip("torch")
    spec, X, Y, zs, e_t, _ = _case(case)
    with torch.no_grad():
        out = tr.forward(spec, X, Y, zs)
    S, N = spec["S"], X.shape[0]
    model = build_from_spec(spec, X, Y)
    e = model.compute_log_likelihood(X, Y, zs=zs)
    _, Fm, Fv = model.propagate(X, S=S, zs=zs)
    want_m = [m.numpy().reshape(S, N, -1) for m in out["Fmeans"]] + [out["mean"].numpy()]
    want_v = [v.numpy().reshape(S, N, -1) for v in out["Fvars"]] + [out["var"].numpy()]
    print("%s forward elbo rel %.3e" % (case, abs(e - e_t) / abs(e_t)))
    assert abs(e - e_t) <= TOL_ELBO * abs(e_t), (case, e, e_t)
    for li in range(len(want_m)):
        print("%s L%d mean %.3e var %.3e" % (case, li, rel(Fm[li], want_m[li]), rel(Fv[li], want_v[li])))
        assert rel(Fm[li], want_m[li]) <= 1e-9 and rel(Fv[li], want_v[li]) <= 1e-9, (case, li)
    model.close()


# ---- optimisers -----------------------------------------------------------------------------------------------------------------------
def _layers(spec):
    return spec["convs"] + [spec["head"]]


def test_adam_steps_match_numpy_on_torch_gradients(ctx):
    """Three steps of the one-call Adam step on small3_M20 against NumPy Adam on torch gradients recomputed after every step, 1e-9; the two
    extra positive parameters move through softplus + 1e-6, and the Python kernel objects carry them after pull_parameters."""
    spec, X, Y, zs, _, _ = _case("small3_M20")
    start = copy.deepcopy(spec)
    spec = copy.deepcopy(spec)
    N, lr, state = X.shape[0], 0.05, {}
    model = build_from_spec(spec, X, Y)
    for t in range(1, 4):
        z = syn.make_noise(spec, N, seed=100 + t)
        e = model.train_step(X, Y, lr, zs=z, t=t)
        ref = tr.reference(spec, X, Y, z)
        e_t, g = ref["parts"][0], ref["want"]
        print("adam t%d elbo rel %.3e" % (t, abs(e - e_t) / abs(e_t)))
        assert abs(e - e_t) <= 1e-9 * abs(e_t), (t, e, e_t)
        ar.adam_numpy_step(spec, g, state, lr, t)
    model.pull_parameters()
    rows = []
    for li, (l, l0, now) in enumerate(zip(_layers(spec), _layers(start), ls.model_values(model))):
        assert set(now) == set(g[li]), (li, sorted(now))
        for name in now:
            rows.append((li, name, rel(now[name], ar.spec_value(l, name)), rel(ar.spec_value(l, name), ar.spec_value(l0, name))))
            print("adam L%d %-17s rel %.3e  (moved %.3e)" % rows[-1])
    for li, name, err, moved in rows:
        assert moved >= 1e-3, (li, name, "has not moved", moved)
        assert err < 1e-9, (li, name, err)
    k = model.layers[1].base_kernel
    assert type(k).__name__ == "ArcCosine" and (k.variance, k.weight_variances, k.bias_variance) == tuple(
        ls.model_values(model)[1][n] for n in ar.NAMES)
    model.close()


def _sgd_expect(x, w, lr, positive):
    if not positive:
        return x + lr * w
    u = ls.softplus_inv(x) + lr * w * (1.0 - np.exp(-(x - 1e-6)))
    return np.log1p(np.exp(u)) + 1e-6


def test_sgd_step_follows_the_torch_gradient(ctx):
    """One sgd_step(lr) on small3_M20: every group = theta + lr * (torch gradient), the positive ones -- weight_variances and bias_variance
    among them -- through the softplus, 1e-9 relative."""
    spec, X, Y, zs, _, want = _case("small3_M20")
    # lr * |want|max is 1.7e-5 (layer 1's bias_variance, 27 with a gradient of 0.46) of the group's largest parameter or more.  Asserted below
    # at 1e-5: with the 1e-9 bar on the result the gradient itself is then pinned to 1e-4 of its maximum or better
    lr = 1e-3
    model = build_from_spec(spec, X, Y)
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.sgd_step(lr)
    model.pull_parameters()
    for li, (l, now) in enumerate(zip(_layers(spec), ls.model_values(model))):
        for name, w in want[li].items():
            x = np.asarray(ar.spec_value(l, name), np.float64)
            expect = _sgd_expect(x, w, lr, name in ls.POSITIVE)
            err = rel(now[name], expect)
            print("sgd L%d %-17s rel %.3e  (moved %.3e)" % (li, name, err, rel(expect, x)))
            assert rel(expect, x) >= 1e-5, (li, name, "the step moves the group too little to check its gradient", rel(expect, x))
            assert err < 1e-9, (li, name, err)
    model.close()


def test_one_arccosine_parameter_can_be_held(ctx):
    """set_trainable(layer, "weight_variances", False): that parameter keeps its bits through an SGD and an Adam step while bias_variance
    and the variance of the same layer, and everything in the other layers, move as they would have; switched back on, it moves again."""
    spec, X, Y, zs, _, want = _case("small3_M20")
    lr = 1e-3
    model = build_from_spec(spec, X, Y)
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.set_trainable(0, "weight_variances", False)
    model.set_trainable(1, "bias_variance", False)
    model.sgd_step(lr)
    model.pull_parameters()
    now = ls.model_values(model)
    for li, held in ((0, "weight_variances"), (1, "bias_variance")):
        for name in ar.NAMES:
            x = ar.spec_value(spec["convs"][li], name)
            if name == held:
                assert now[li][name] == x, (li, name, now[li][name], x)
            else:
                assert now[li][name] != x and rel(now[li][name], _sgd_expect(x, want[li][name], lr, True)) < 1e-9, (li, name)
    assert rel(now[2]["lengthscales"], _sgd_expect(spec["head"]["ls"], want[2]["lengthscales"], lr, True)) < 1e-9
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.adam_step(0.01, t=1)
    model.pull_parameters()
    after = ls.model_values(model)
    assert after[0]["weight_variances"] == now[0]["weight_variances"] and after[1]["bias_variance"] == now[1]["bias_variance"]
    for li, name in ((0, "bias_variance"), (0, "variance"), (1, "weight_variances"), (1, "variance")):
        assert abs(np.log(after[li][name] / now[li][name])) > 1e-3, (li, name)       # a first Adam step moves by ~lr in the unconstrained space
    model.set_trainable(0, "weight_variances", True)
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.sgd_step(lr)
    model.pull_parameters()
    assert ls.model_values(model)[0]["weight_variances"] != after[0]["weight_variances"]
    with pytest.raises(Exception):
        model.set_trainable(2, "weight_variances", False)                            # the head's kernel is an RBF
    model.close()


def test_natgrad_step_matches_numpy_on_torch_gradients(ctx):
    """One natgrad_step on small3_M20 against tests/natgrad_ref.py fed the torch gradients, rel < 1e-8."""
    from natgrad_ref import natgrad_reference
    spec, X, Y, zs, _, want = _case("small3_M20")
    gamma = 1e-5
    model = build_from_spec(spec, X, Y)
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.natgrad_step(gamma)
    model.pull_parameters()
    for li, (l, m) in enumerate(zip(_layers(spec), model.layers)):
        mu1, L1 = natgrad_reference(np.asarray(l["q_mu"]), np.asarray(l["q_sqrt"]), want[li]["q_mu"], want[li]["q_sqrt"], gamma)
        print("natgrad L%d rel q_mu %.3e q_sqrt %.3e (moved %.3e / %.3e)" % (li, rel(m.q_mu, mu1), rel(m.q_sqrt, L1), rel(mu1, l["q_mu"]),
                                                                           rel(L1, l["q_sqrt"])))
        assert rel(m.q_mu, mu1) < 1e-8 and rel(m.q_sqrt, L1) < 1e-8, (li, rel(m.q_mu, mu1), rel(m.q_sqrt, L1))
    model.close()


# ---- the data path --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small3_M20", "odd_M33"])
@pytest.mark.parametrize("objective", ["elbo", "density"])
def test_input_gradient_matches_torch_autograd(ctx, case, objective):
    """input_gradient against autograd with respect to X (the acos_w factor of patch_backward's dX): tests/test_gpu_input_grad.py's bounds --
    J 1e-9 relative (2e-8 for the density of an unwhitened ArcCosine model), dX 1e-7 of max(1, |dX|max).  Head marginals of predict_f
    against the forward's, 1e-9."""
    torch = pytest.importorskip("torch")
    import test_oracle_autograd as toa
    spec, X, Y, zs, _, _ = _case(case)
    S, N = spec["S"], X.shape[0]
    out = tr.forward(spec, X, Y, zs, x_leaf=True)
    if objective == "elbo":
        Jt = out["data"]
    else:
        p = toa._robustmax_predict(out["mean"].reshape(S * N, -1), out["var"].reshape(S * N, -1)).reshape(S, N, -1)
        Jt = torch.log(p[:, torch.arange(N), torch.tensor(np.asarray(Y).reshape(-1), dtype=torch.long)].mean(0))
    (gX,) = torch.autograd.grad(Jt.sum(), out["X"])
    Jw, want = Jt.detach().numpy(), gX.numpy()
    model = build_from_spec(spec, X, Y)
    J, got = model.input_gradient(X, Y, objective=objective, zs=zs)
    err = np.abs(got.reshape(want.shape) - want).max()
    print("%s %s: |dX - autograd| = %.3e, |want|max = %.3e, J vs torch %.3e" % (case, objective, err, np.abs(want).max(), rel(J, Jw)))
    assert rel(J, Jw) <= (2e-8 if objective == "density" else 1e-9), (J, Jw)
    assert err <= 1e-7 * max(1.0, np.abs(want).max()), (err, np.abs(want).max())
    Fm, Fv = model.predict_f(X, S, zs=zs)
    print("%s predict_f mean %.3e var %.3e" % (case, rel(Fm, out["mean"].detach().numpy()), rel(Fv, out["var"].detach().numpy())))
    assert rel(Fm, out["mean"].detach().numpy()) <= 1e-9 and rel(Fv, out["var"].detach().numpy()) <= 1e-9
    model.close()

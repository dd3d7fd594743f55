"""Per-dimension (ARD) lengthscales on the conv layers' RBF base kernel on the device (--ard): the operator entry dcgp_kuf_patches_rbf_ard
and K_uu of scaled rows against explicit-difference NumPy, a ConvLayer against the oracle's layer, and the model path -- ELBO, every
gradient group, the three optimisers, composition with the other features, the data path, the flag and its checkpoints -- against torch
autograd of the references of tests/ (which divide the patches by ``ls`` as it stands: a vector goes through them unchanged).

The cases are tests/ard_ref.py's: live_specs' with every conv layer's ``ls`` replaced by a vector spread 0.8 - 1.2 around it; their reference
gradients are live, the lengthscale vectors included (asserted without a GPU in tests/test_host_ard.py).  Bars: operators 1e-12 of the
variance, the layer 1e-9, ELBO 1e-9 relative, every group 1e-7 of the group's maximum, entry-wise 1e-5 over live_specs.errors' kept entries
-- tests/test_gpu_matern.py's, on the same sweep + GEMM route.  Every figure is printed before it is asserted (run with -s)."""
import copy
import functools
import os

import numpy as np
import pytest

from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.models import build_from_spec
import ard_ref as ar
import live_specs as ls
import torch_ref as tr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]   # a hung launch ends the run instead of holding the device

TOL_ELBO, TOL_GROUP, TOL_E = 1e-9, 1e-7, 1e-5
INPUT_GRAD_TOL = 1e-7                   # tests/test_gpu_input_grad.py: |dX - autograd|max <= 1e-7 * max(1, |autograd|max)
# (H, W, C, f, s, M): L = 9, 32, 250, 25, 25, 275 -- L not a multiple of 4, L > 256 (the norm and tile loops chunk there); M not a multiple
# of 16; Mp > 256; patch counts that do not fill a 64-column tile; stride > 1
GEOMS = [(12, 12, 1, 3, 1, 6), (13, 13, 2, 4, 3, 33), (14, 14, 10, 5, 1, 72), (28, 28, 1, 5, 2, 200), (28, 28, 1, 5, 2, 264), (9, 9, 11, 5, 2, 20)]
DEDUP = pytest.mark.parametrize("dedup", [False, True], ids=["tiled", "dedup"])


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


# ---- 1. operators -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,C,f,s,M", GEOMS)
def test_kuf_patches_ard_and_kuu_of_scaled_rows(ctx, H, W, C, f, s, M):
    """Both output layouts and K_uu against explicit differences, 1e-12 of the variance; Z[0] IS a patch of image 1."""
    from oracle.views import FullView as OFullView
    from deepcgp_amd.kernels import RBF
    from deepcgp_amd.layers import MultiOutputConvKernel
    from deepcgp_amd.views import FullView
    rng = np.random.default_rng(H + M)
    N, var = 3, 1.7
    X = rng.standard_normal((N, H, W, C))
    v, ov = FullView((H, W), f, C, s), OFullView((H, W), f, C, s)
    L, P = v.patch_length, v.patch_count
    PNL = ov.extract_patches_PNL(X)                                # [P, N, L]
    Z = rng.standard_normal((M, L))
    Z[0] = PNL[P // 2, 1]
    lsc = 0.9 * np.sqrt(L) * (0.8 + 0.4 * rng.random(L))
    k = RBF(L, var, lsc, ARD=True)
    got, want = k.K(Z), ar.rbf_ard_numpy(Z, Z, var, lsc)
    assert np.all(np.isfinite(got)) and np.abs(got - want).max() <= 1e-12 * var, np.abs(got - want).max()
    assert np.abs(k._gram(Z, 1e-3) - (want + 1e-3 * np.eye(M))).max() <= 1e-12 * var
    mok = MultiOutputConvKernel(k, H * W * C, P)
    pmn = mok.Kuf(Z, (X, v))                                       # layout 0: [P, M, N]
    want_pmn = np.stack([ar.rbf_ard_numpy(Z, PNL[p], var, lsc) for p in range(P)])
    assert pmn.shape == (P, M, N) and np.all(np.isfinite(pmn))
    err = np.abs(pmn - want_pmn).max()
    print("ARD %s L %d Kuu err %.2e Kuf err %.2e  coincident entry: got %.17g want %.17g" % ((H, W, C, f, s, M), L, np.abs(got - want).max(), err,
                                                                                           pmn[P // 2, 0, 1], want_pmn[P // 2, 0, 1]))
    assert err <= 1e-12 * var, err
    dX, dZ, out = ctx.to_device(X), ctx.to_device(Z), ctx.empty((M, N * P))
    k._kuf(ctx, dX, N, H, W, C, f, s, dZ, M, out, 1)               # layout 1: [M, N * P], column n * P + p
    assert np.array_equal(out.numpy().reshape(M, N, P), np.transpose(pmn, (1, 2, 0)))
    # equal lengthscales: the scalar entry's values to rounding
    one = RBF(L, var, 3.0)
    same = MultiOutputConvKernel(RBF(L, var, np.full(L, 3.0), ARD=True), H * W * C, P).Kuf(Z, (X, v))
    assert np.abs(same - MultiOutputConvKernel(one, H * W * C, P).Kuf(Z, (X, v))).max() <= 1e-12 * var


def test_argument_checks(ctx):
    from deepcgp_amd.kernels import RBF
    Lb = dev.lib()
    X, Z, out = ctx.to_device(np.zeros((1, 4, 4, 1))), ctx.to_device(np.zeros((4, 9))), ctx.empty((4, 4))
    good, bad = ctx.to_device(np.ones(9)), ctx.to_device(np.array([1.0] * 8 + [0.0]))
    assert Lb.dcgp_kuf_patches_rbf_ard(ctx.handle, X.ptr, 1, 4, 4, 1, 3, 1, Z.ptr, 4, 1.0, good.ptr, out.ptr, 1) == 0
    assert Lb.dcgp_kuf_patches_rbf_ard(ctx.handle, X.ptr, 1, 4, 4, 1, 3, 1, Z.ptr, 4, 1.0, bad.ptr, out.ptr, 1) == dev.ERR_ARG
    assert b"not positive" in Lb.dcgp_last_error(ctx.handle)
    assert Lb.dcgp_kuf_patches_rbf_ard(ctx.handle, X.ptr, 1, 4, 4, 1, 3, 1, Z.ptr, 4, 1.0, None, out.ptr, 1) == dev.ERR_ARG
    assert Lb.dcgp_kuf_patches_rbf_ard(ctx.handle, X.ptr, 1, 4, 4, 1, 5, 1, Z.ptr, 4, 1.0, good.ptr, out.ptr, 1) == dev.ERR_ARG      # f > H
    with pytest.raises(ValueError):                                # a kernel of another patch length
        RBF(8, 1.0, np.ones(8), ARD=True)._kuf(ctx, X, 1, 4, 4, 1, 3, 1, Z, 4, out, 1)
    # the model: a wrong count, a non-positive entry, a multi-patch head, a Matern layer
    spec, Xm, Y, zs = ar.ard_case("small3_M20")
    model = build_from_spec(spec, Xm, Y)
    model._build()
    L0 = spec["convs"][0]["f"] ** 2 * spec["convs"][0]["C"]
    vals = np.ones(L0 + 1)
    assert Lb.dcgp_model_set_param(model._model, 0, b"ard_lengthscales", vals.ctypes.data, L0 + 1) == dev.ERR_ARG
    assert b"expected" in Lb.dcgp_last_error(ctx.handle)
    vals[2] = -1.0
    assert Lb.dcgp_model_set_param(model._model, 0, b"ard_lengthscales", vals.ctypes.data, L0) == dev.ERR_ARG
    assert b"> 0" in Lb.dcgp_last_error(ctx.handle)
    hl = np.ones(spec["head"]["Z"].shape[1])
    assert Lb.dcgp_model_set_param(model._model, len(model.layers) - 1, b"ard_lengthscales", hl.ctypes.data, hl.size) == dev.ERR_ARG
    assert b"single-patch head" in Lb.dcgp_last_error(ctx.handle)
    model.close()
    plain = ls.make_case("small3_M20")[0]
    plain["convs"][0]["base"] = "matern32"
    model = build_from_spec(plain, Xm, Y)
    model._build()
    assert Lb.dcgp_model_set_param(model._model, 0, b"ard_lengthscales", np.ones(L0).ctypes.data, L0) == dev.ERR_ARG
    assert b"RBF base kernel" in Lb.dcgp_last_error(ctx.handle)
    model.close()


# ---- 2. layer ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [False, True])
def test_conv_layer_against_the_oracle_layer(ctx, white):
    from oracle.gpflow_ref import RBF as ORBF
    from oracle.layers import ConvLayer as OConvLayer
    from oracle.views import FullView as OFullView
    from deepcgp_amd.kernels import RBF, PatchInducingFeatures
    from deepcgp_amd.layers import ConvLayer
    from deepcgp_amd.views import FullView
    rng = np.random.default_rng(12)
    H, W, C, f, s, M, R, N = 12, 12, 3, 5, 1, 24, 4, 3
    X = rng.standard_normal((N, H * W * C))
    v, ov = FullView((H, W), f, C, s), OFullView((H, W), f, C, s)
    L = v.patch_length
    lsc = 7.0 * (0.8 + 0.4 * rng.random(L))
    Z, q_mu = rng.standard_normal((M, L)), rng.standard_normal((M, R))
    q_sqrt = np.tril(rng.standard_normal((R, M, M))) * 0.2 + np.eye(M)[None]
    layer = ConvLayer(RBF(L, 1.3, lsc, ARD=True), None, PatchInducingFeatures(Z), v, white=white, gp_count=R, q_mu=q_mu, q_sqrt=q_sqrt)
    olayer = OConvLayer(ORBF(L, 1.3, lsc, ARD=True), None, Z, ov, white=white, gp_count=R, q_mu=q_mu, q_sqrt=q_sqrt)
    m, var = layer.conditional_ND(X)
    om, ovar = olayer.conditional_ND(X)
    print("ARD layer white=%s mean %.2e var %.2e" % (white, rel(m, om), rel(var, ovar)))
    assert rel(m, om) <= 1e-9 and rel(var, ovar) <= 1e-9
    assert abs(layer.KL() - olayer.KL()) <= 1e-9 * abs(olayer.KL())
    z = rng.standard_normal((1, N, layer.num_outputs))
    smp, m2, v2 = layer.sample_from_conditional(X[None], z=z)                 # with z
    assert rel(smp[0], om + z[0] * np.sqrt(ovar + 1e-3)) <= 1e-9 and np.array_equal(m2[0], m)
    smp0, _, _ = layer.sample_from_conditional(X[None])                        # without: finite, the layer's shape
    assert smp0.shape == smp.shape and np.all(np.isfinite(smp0))
    # full_cov=True uses the vector too (a scalar in its place is the bug to exclude): against the oracle
    fm, fv = layer.conditional_ND(X, full_cov=True)
    ofm, ofv = olayer.conditional_ND(X, full_cov=True)
    print("ARD layer full_cov mean %.2e var %.2e" % (rel(fm, ofm), rel(fv, ofv)))
    assert rel(fm, ofm) <= 1e-9 and rel(fv, ofv) <= 1e-9


# ---- 3. model value and gradients ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    """(spec, X, Y, zs, e_t, want): the ARD case and its torch reference, computed once per process; never written to."""
    pytest.importorskip("torch")
    spec, X, Y, zs = ar.ard_case(name)
    ref = tr.reference(spec, X, Y, zs)
    e_t, want = ref["parts"][0], ref["want"]
    ar.assert_live(name, want)
    return spec, X, Y, zs, e_t, want


def _check_gradients(tag, grads, want):
    rows = []
    for li, groups in enumerate(want):
        assert set(groups) == set(grads[li]), (tag, li, sorted(groups), sorted(grads[li]))
        for name, w in groups.items():
            g = np.asarray(grads[li][name], np.float64)
            assert g.shape == np.shape(w), (tag, li, name, g.shape, np.shape(w))
            rows.append((li, name) + ls.errors(name, g, w))
            print("%s L%d %-14s group %.3e  entry %.3e  |want|max %.3e" % ((tag,) + rows[-1] + (np.abs(w).max(),)))
    print("%s WORST group %.3e entry %.3e" % (tag, max(r[2] for r in rows), max(r[3] for r in rows)))
    for li, name, err_g, err_e in rows:
        assert err_g <= TOL_GROUP, (tag, li, name, "group-wise", err_g)
        assert err_e <= TOL_E, (tag, li, name, "entry-wise", err_e)


@DEDUP
@pytest.mark.parametrize("case", ar.CASES)
def test_elbo_and_gradient_match_torch_autograd(ctx, case, dedup):
    spec, X, Y, zs, e_t, want = _case(case)
    tag = "ARD %s-%s" % (case, "dedup" if dedup else "tiled")
    model = build_from_spec(copy.deepcopy(spec), X, Y)
    model.dedup_layer0 = dedup
    e, grads = model.compute_gradients(X, Y, zs=zs)
    e_f = model.compute_log_likelihood(X, Y, zs=zs)
    print("%s elbo rel %.3e forward-only %.3e" % (tag, abs(e - e_t) / abs(e_t), abs(e_f - e_t) / abs(e_t)))
    assert abs(e - e_t) <= TOL_ELBO * abs(e_t), (tag, e, e_t)
    assert abs(e_f - e_t) <= TOL_ELBO * abs(e_t), (tag, "forward-only", e_f, e_t)
    _check_gradients(tag, grads, want)
    for li, c in enumerate(spec["convs"]):
        assert grads[li]["lengthscales"].shape == (c["f"] * c["f"] * c["C"],)
    model.close()


# ---- 4. equal lengthscales: the scalar model on the same route ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["small3_M20", "small3_white_M20"])
def test_equal_lengthscales_are_the_scalar_model(ctx, case):
    """No reference: every l_l = l against the scalar model forced onto the sweep + GEMM route (no_fused_layer).  ELBO 1e-9, every shared group
    1e-7, and sum_l gard_l = d / d l at 1e-7 of it -- which a missed prior term breaks on the unwhitened case."""
    spec, X, Y, zs = ls.make_case(case)
    vec = copy.deepcopy(spec)
    for c in vec["convs"]:
        c["ls"] = np.full(c["f"] * c["f"] * c["C"], c["ls"])
    a, b = build_from_spec(vec, X, Y), build_from_spec(copy.deepcopy(spec), X, Y)
    ea, ga = a.compute_gradients(X, Y, zs=zs)
    ctx._check(dev.lib().dcgp_ctx_set_option(ctx.handle, b"no_fused_layer", 1))
    try:
        eb, gb = b.compute_gradients(X, Y, zs=zs)
    finally:
        ctx._check(dev.lib().dcgp_ctx_set_option(ctx.handle, b"no_fused_layer", 0))
    print("ARD equal %s elbo rel %.3e" % (case, abs(ea - eb) / abs(eb)))
    assert abs(ea - eb) <= TOL_ELBO * abs(eb)
    for li, (x, y) in enumerate(zip(ga, gb)):
        for name in y:
            if name == "lengthscales" and li < len(spec["convs"]):
                err = abs(x[name].sum() - y[name]) / abs(y[name])
                print("ARD equal %s L%d sum gard %.15g scalar %.15g rel %.3e" % (case, li, x[name].sum(), float(y[name]), err))
                assert err <= TOL_GROUP, (case, li, err)
            else:
                err = ls.errors(name, x[name], y[name])[0]
                print("ARD equal %s L%d %-14s group %.3e" % (case, li, name, err))
                assert err <= TOL_GROUP, (case, li, name, err)
    a.close(), b.close()


# ---- 5. optimisers -----------------------------------------------------------------------------------------------------------------------
def test_adam_steps_match_numpy_on_torch_gradients(ctx):
    """Three one-call Adam steps on small3_M20 against NumPy Adam on torch gradients recomputed after every step (test_gpu_matern's scheme
    and tolerances): the step's ELBO at t >= 2 is that of the moved vector, so in_scale follows it; the vector stays positive."""
    spec, X, Y, zs, _, _ = _case("small3_M20")
    spec = copy.deepcopy(spec)
    N, lr, state = X.shape[0], 0.05, {}
    model = build_from_spec(copy.deepcopy(spec), X, Y)
    for t in range(1, 4):
        z = syn.make_noise(spec, N, seed=100 + t)
        e = model.train_step(X, Y, lr, zs=z, t=t)
        ref = tr.reference(spec, X, Y, z)
        e_t, g = ref["parts"][0], ref["want"]
        print("ARD adam t%d elbo rel %.3e" % (t, abs(e - e_t) / abs(e_t)))
        assert abs(e - e_t) <= 1e-8 * abs(e_t), (t, e, e_t)
        ls.adam_numpy_step(spec, g, state, lr, t)
    model.pull_parameters()
    for li, (l, now) in enumerate(zip(spec["convs"] + [spec["head"]], ar.model_values(model))):
        for name in now:
            err = rel(now[name], l[ls.SPEC_KEY[name]])
            print("ARD adam L%d %-14s rel %.3e" % (li, name, err))
            assert err < (1e-8 if name in ls.POSITIVE else 1e-7), (li, name, err)
    k0 = model.layers[0].base_kernel
    assert k0.ARD and k0.lengthscales.shape == (9,) and np.all(k0.lengthscales > 0) and not np.array_equal(k0.lengthscales, _case("small3_M20")[0]["convs"][0]["ls"])
    # a model rebuilt from the pulled values gives the device model's ELBO: the staging scale is 1 / the vector
    e_dev = model.compute_log_likelihood(X, Y, zs=zs)
    e_new = tr.forward(spec, X, Y, zs)["elbo"].item()
    assert abs(e_dev - e_new) <= 1e-8 * abs(e_new)
    model.close()


def test_sgd_step_follows_the_torch_gradient(ctx):
    spec, X, Y, zs, _, want = _case("small3_M20")
    lr = 1e-4
    model = build_from_spec(copy.deepcopy(spec), X, Y)
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.sgd_step(lr)
    model.pull_parameters()
    for li, (l, now) in enumerate(zip(spec["convs"] + [spec["head"]], ar.model_values(model))):
        for name, w in want[li].items():
            x = np.asarray(l[ls.SPEC_KEY[name]], np.float64)
            if name in ls.POSITIVE:
                u = ls.softplus_inv(x) + lr * w * (1.0 - np.exp(-(x - 1e-6)))
                expect = np.log1p(np.exp(u)) + 1e-6
            else:
                expect = x + lr * w
            err = rel(now[name], expect)
            print("ARD sgd L%d %-14s rel %.3e  (moved %.3e)" % (li, name, err, rel(expect, x)))
            assert rel(expect, x) >= 1e-5, (li, name, "the step moves the group too little to check its gradient", rel(expect, x))
            assert err < 1e-9, (li, name, err)
    model.close()


def test_natgrad_step_matches_numpy_on_torch_gradients(ctx):
    from natgrad_ref import natgrad_reference
    spec, X, Y, zs, _, want = _case("small3_M20")
    gamma = 1e-5
    model = build_from_spec(copy.deepcopy(spec), X, Y)
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.natgrad_step(gamma)
    model.pull_parameters()
    for li, (l, m) in enumerate(zip(spec["convs"] + [spec["head"]], model.layers)):
        mu1, L1 = natgrad_reference(np.asarray(l["q_mu"]), np.asarray(l["q_sqrt"]), want[li]["q_mu"], want[li]["q_sqrt"], gamma)
        assert rel(m.q_mu, mu1) < 1e-8 and rel(m.q_sqrt, L1) < 1e-8, (li, rel(m.q_mu, mu1), rel(m.q_sqrt, L1))
    assert np.array_equal(model.layers[0].base_kernel.lengthscales, spec["convs"][0]["ls"])      # NatGrad moves q_mu / q_sqrt only
    model.close()


def test_set_trainable_optimizer_state_and_clip(ctx):
    spec, X, Y, zs, _, want = _case("small3_M20")
    vec0 = [np.array(c["ls"]) for c in spec["convs"]]
    model = build_from_spec(copy.deepcopy(spec), X, Y)
    # frozen: the vector stays to the bit, the variance and everything else move
    model.set_trainable(0, "ard_lengthscales", False)
    model.train_step(X, Y, 0.05, zs=zs, t=1)
    model.pull_parameters()
    assert np.array_equal(model.layers[0].base_kernel.lengthscales, vec0[0])
    assert not np.array_equal(model.layers[1].base_kernel.lengthscales, vec0[1]) and model.layers[0].base_kernel.variance != spec["convs"][0]["variance"]
    model.set_trainable(0, "ard_lengthscales", True)
    model.train_step(X, Y, 0.05, zs=zs, t=2)
    model.pull_parameters()
    assert not np.array_equal(model.layers[0].base_kernel.lengthscales, vec0[0])
    # optimizer_state: the new group with m | v, a round trip into a second model gives the same next step
    st = model.optimizer_state()
    for li, v in enumerate(vec0):
        for mv in ("m", "v"):
            assert st["layers/%d/ard_lengthscales/%s" % (li, mv)].shape == v.shape
    assert np.abs(st["layers/1/ard_lengthscales/m"]).max() > 0 and "layers/2/ard_lengthscales/m" not in st
    other = build_from_spec(copy.deepcopy(spec), X, Y)
    other._build()
    for p, q in zip(other.parameters, model.parameters):
        p.assign(np.array(q.value))
    other.sync_parameters()
    other.set_optimizer_state(st)
    ea, eb = model.train_step(X, Y, 0.05, zs=zs, t=3), other.train_step(X, Y, 0.05, zs=zs, t=3)
    model.pull_parameters(), other.pull_parameters()
    assert ea == eb
    for p, q in zip(other.parameters, model.parameters):
        assert np.array_equal(np.array(p.value), np.array(q.value)), p.pathname
    model.close(), other.close()
    # the clip's global norm counts the vector: NumPy on the torch gradient in the unconstrained space
    model = build_from_spec(copy.deepcopy(spec), X, Y)
    model.set_grad_clip(float("inf"))
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.adam_step(0.01, 1)
    sq = 0.0
    for l, groups in zip(spec["convs"] + [spec["head"]], want):
        for name, g in groups.items():
            x = np.asarray(l[ls.SPEC_KEY[name]], np.float64)
            gu = g * (1.0 - np.exp(-(x - 1e-6))) if name in ls.POSITIVE else g
            sq += float(np.sum(np.square(gu)))
    without = sq - sum(float(np.sum(np.square(want[li]["lengthscales"] * (1.0 - np.exp(-(vec0[li] - 1e-6)))))) for li in range(len(vec0)))
    got = model.last_grad_norms[0]
    print("ARD clip norm got %.15g want %.15g (without the vectors %.15g)" % (got, np.sqrt(sq), np.sqrt(without)))
    # (the bound tells the two apart only if the vectors' share of the norm is well above it: ten times here)
    assert abs(np.sqrt(without) - np.sqrt(sq)) > 10 * 1e-7 * np.sqrt(sq)
    assert abs(got - np.sqrt(sq)) <= 1e-7 * np.sqrt(sq)
    model.close()


# ---- 6. composition --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _compose_case(cid):
    pytest.importorskip("torch")
    import compose_cases as cc
    import compose_ref as cr
    spec, X, Y, zs, lik = cc.make_case(cc.BY_ID[cid])
    ar.ardify(spec)
    ref = cr.reference(spec, X, Y, zs, lik)
    ar.assert_live(cid, ref["want"])
    return spec, X, Y, zs, lik, ref


@DEDUP
@pytest.mark.parametrize("cid", ar.COMPOSE_CASES)
def test_composition_with_padding_means_likelihoods_and_whitening(ctx, cid, dedup):
    import compose_ref as cr
    spec, X, Y, zs, lik, ref = _compose_case(cid)
    tag = "ARD %s-%s" % (cid, "dedup" if dedup else "tiled")
    model = build_from_spec(copy.deepcopy(spec), X.copy(), Y.copy(), likelihood=cr.make_likelihood(lik))
    model.dedup_layer0 = dedup
    e_t = ref["parts"][0]
    e, grads = model.compute_gradients(X, Y, zs=zs)
    print("%s elbo rel %.3e" % (tag, abs(e - e_t) / abs(e_t)))
    assert abs(e - e_t) <= TOL_ELBO * abs(e_t), (tag, e, e_t)
    _check_gradients(tag, grads, ref["want"])
    # the data path through the ARD layers: the input gradient of the elbo objective, evaluate against predict_y
    J, dX = model.input_gradient(X, Y, objective="elbo", zs=zs)
    bound = INPUT_GRAD_TOL * max(1.0, np.abs(ref["dX"]).max())
    print("%s input gradient %.3e bound %.1e J %.3e" % (tag, np.abs(dX - ref["dX"]).max(), bound, rel(J, ref["J"])))
    assert rel(J, ref["J"]) <= TOL_ELBO and np.abs(dX - ref["dX"]).max() <= bound and np.abs(ref["dX"]).max() > 0
    pm, _ = model.predict_y(X, spec["S"], zs=zs)
    assert rel(pm, ref["py_mean"]) <= 1e-9
    r = model.evaluate(X, Y, S=spec["S"], batch_size=2, zs=zs, per_image=True)
    assert rel(r["log_density"], ref["density"].sum(1)) <= 1e-9
    model.close()


@DEDUP
@pytest.mark.parametrize("name", ar.MIXING_CASES)
def test_composition_with_mixed_layers(ctx, name, dedup):
    pytest.importorskip("torch")
    import mixing_ref as mx
    spec, X, Y, zs = mx.make_case(name)
    ar.ardify(spec)
    ref = tr.reference(spec, X, Y, zs)
    e_t, want = ref["parts"][0], ref["want"]
    tag = "ARD mix %s-%s" % (name, "dedup" if dedup else "tiled")
    model = build_from_spec(copy.deepcopy(spec), X, Y)
    model.dedup_layer0 = dedup
    e, grads = model.compute_gradients(X, Y, zs=zs)
    print("%s elbo rel %.3e" % (tag, abs(e - e_t) / abs(e_t)))
    assert abs(e - e_t) <= TOL_ELBO * abs(e_t), (tag, e, e_t)
    _check_gradients(tag, grads, want)
    model.close()


# ---- 7. the data path ----------------------------------------------------------------------------------------------------------------------
@DEDUP
def test_input_gradient_of_both_objectives_and_saliency(ctx, dedup):
    """small3_M20: the elbo objective against compose_ref.torch_input_gradient, the density objective against mixing_ref.torch_input_gradient
    (the same forward with tests/input_grad_ref.py's per-row RobustMax quantity as its tail); dX in the caller's geometry."""
    pytest.importorskip("torch")
    import compose_ref as cr
    import mixing_ref as mx
    spec, X, Y, zs, _, _ = _case("small3_M20")
    model = build_from_spec(copy.deepcopy(spec), X, Y)
    model.dedup_layer0 = dedup
    for objective, (Jw, gw) in (("elbo", cr.torch_input_gradient(spec, X, Y, zs, ("robustmax", 10))),
                                ("density", tr.input_gradient(spec, X, Y, zs, tr.robustmax_density(Y)))):
        J, dX = model.input_gradient(X, Y, objective=objective, zs=zs)
        bound = INPUT_GRAD_TOL * max(1.0, np.abs(gw).max())
        print("ARD input gradient %s dedup=%s: %.3e bound %.1e |want|max %.3e J %.3e" % (objective, dedup, np.abs(dX - gw).max(), bound, np.abs(gw).max(),
                                                                                        rel(J, Jw)))
        assert dX.shape == X.shape and rel(J, Jw) <= 1e-9 and np.abs(dX - gw).max() <= bound and np.abs(gw).max() > 0
    sal = model.saliency(X, Y, zs=zs)
    assert sal.shape == (X.shape[0], 14, 14, 1) and np.array_equal(sal.reshape(X.shape), model.input_gradient(X, Y, zs=zs)[1])
    model.close()


def test_uncertainty_views_and_augmented_train_run(ctx):
    """evaluate(views=) / evaluate_uncertainty run through the ARD layers and agree with the plain evaluation where they must; train_run
    with augmentation and clipping on against the per-step loop on mirror-augmented batches, bit for bit."""
    from deepcgp_amd import augment
    from deepcgp_amd.augment import Augmentation
    spec, X, Y, zs, _, _ = _case("small3_M20")
    S, N = spec["S"], X.shape[0]
    model = build_from_spec(copy.deepcopy(spec), X, Y)
    r = model.evaluate(X, Y, S=S, batch_size=N, zs=zs, per_image=True)
    u = model.evaluate_uncertainty(X, Y, S=S, batch_size=N, zs=zs, per_image=True)
    assert np.array_equal(u["log_density"], r["log_density"]) and np.isfinite(u["mean_predictive_entropy"])
    rv = model.evaluate(X, Y, S=S, batch_size=N, seed=3, views=np.array([(0, 0, 0)], np.int32), per_image=True)
    r0 = model.evaluate(X, Y, S=S, batch_size=N, seed=3, per_image=True)
    assert rel(rv["log_density"], r0["log_density"]) <= 1e-12
    model.close()
    rng = np.random.default_rng(5)
    pool, batch, aug, hwc = 11, 3, Augmentation(2, True), (14, 14, 1)
    Xp, _ = syn.make_batch(hwc, pool, seed=7)
    Yp = rng.integers(0, 10, pool).astype(np.int32)
    idx = np.stack([rng.choice(pool, batch, replace=False) for _ in range(3)]).astype(np.int64)
    lrs = np.array([0.01, 0.01, 0.001])
    a, b = build_from_spec(copy.deepcopy(spec), Xp.copy(), Yp.copy()), build_from_spec(copy.deepcopy(spec), Xp.copy(), Yp.copy())
    for m in (a, b):
        m.set_grad_clip(50.0)
    ha = []
    for i in range(3):
        Xb = augment.apply(a.X[idx[i]].reshape((batch,) + hwc), *augment.draw(21 + i, batch, aug.max_shift, aug.hflip)).reshape(batch, -1)
        ha.append(a.train_step(Xb, a.Y[idx[i]], lrs[i], seed=21 + i))
    b.attach_dataset()
    b.set_augmentation(aug)
    hb = b.train_run(idx, lrs, seed=21)
    print("ARD loop %s run %s" % (ha, hb))
    assert np.all(np.isfinite(ha)) and np.array_equal(np.array(ha), hb)
    a.pull_parameters(), b.pull_parameters()
    for p, q in zip(a.parameters, b.parameters):
        assert np.array_equal(np.array(p.value), np.array(q.value)), p.pathname
    assert not np.array_equal(a.layers[0].base_kernel.lengthscales, spec["convs"][0]["ls"])
    b.detach_dataset()
    a.close(), b.close()


# ---- 8. the flag, training and checkpoints ----------------------------------------------------------------------------------------------------
def test_model_builder_trains_saves_and_reloads_an_ard_model(ctx, tmp_path):
    """--ard through ModelBuilder on digits-sized synthetic data: 20 Adam steps, save_model_parameters, a rebuild with --ard --load-model
    gives the same ELBO to 1e-12 (test_gpu_matern's bound); a scalar checkpoint broadcasts; the vector one without --ard is refused."""
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder, save_model_parameters
    rng = np.random.default_rng(3)
    X = rng.random((40, 8, 8, 1))
    Y = rng.integers(0, 10, size=(40, 1)).astype(np.int32)
    args = ['--name', 't', '-M', '6,7', '--feature-maps', '3', '--filter-sizes', '3,3', '--strides', '1,1', '--num-samples', '2', '--batch-size', '8']
    flags = default_parser().parse_args(args + ['--ard'])
    np.random.seed(0)
    a = ModelBuilder(flags, X, Y).build()
    k = a.layers[0].base_kernel
    assert k.ARD and np.array_equal(k.lengthscales, np.full(9, 5.0)) and k.variance == 5.0 and not a.layers[1].kern.base_kernel.ARD
    Xb, Yb = X[:8].reshape(8, -1), Y[:8]
    zs = [rng.standard_normal((2, 8, l.num_outputs)) for l in a.layers]
    e0 = a.compute_log_likelihood(Xb, Yb, zs=zs)
    a.set_trainable(0, "Z", False)      # (a rebuilt model takes the KL prior's frozen patches from the checkpoint's Z: see test_gpu_matern)
    for t in range(1, 21):
        a.train_step(Xb, Yb, 0.02, zs=zs, t=t)
    a.pull_parameters()
    e_a = a.compute_log_likelihood(Xb, Yb, zs=zs)
    vec = a.layers[0].base_kernel.lengthscales
    assert np.isfinite(e_a) and e_a != e0 and vec.shape == (9,) and np.all(vec > 0) and np.ptp(vec) > 0
    path = os.path.join(str(tmp_path), "t.npy")
    saved = save_model_parameters(a, path, global_step=20)
    assert np.array_equal(saved['DGP/layers/0/conv_kernel/base_kernel/lengthscales'], vec)
    flags.load_model = 't'
    bld = ModelBuilder(flags, X, Y, model_path=path)
    b = bld.build()
    e_b = b.compute_log_likelihood(Xb, Yb, zs=zs)
    print("ARD checkpoint: elbo %.15g reloaded %.15g" % (e_a, e_b))
    assert bld.global_step == 20 and abs(e_b - e_a) <= 1e-12 * abs(e_a)
    plain = default_parser().parse_args(args + ['--load-model', 't'])
    with pytest.raises(ValueError, match="--ard"):
        ModelBuilder(plain, X, Y, model_path=path).build()
    a.close(), b.close()

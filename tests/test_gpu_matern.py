"""Matern-3/2 and Matern-5/2 base kernels of the conv layers on the device (--base-kernel matern32 | matern52): the operator entry points
against the NumPy classes of tests/matern_ref.py, a ConvLayer against the oracle's layer fed the NumPy kernel, and the model path -- ELBO,
every gradient group, the three optimisers, prediction, evaluation, input gradients, a Gaussian likelihood, a checkpoint round trip --
against torch autograd of tests/matern_ref.py's textbook forward (float64, CPU).

The model cases are tests/live_specs.py's with every conv layer's `base` set to the Matern type; their reference gradients are live
(asserted without a GPU in tests/test_host_matern.py).  Bars: ELBO 1e-9 relative, every group 1e-7 of the group's maximum, entry-wise 1e-5
over live_specs.errors' kept entries -- tests/test_gpu_grad_m256.py's.

Largest device-vs-autograd error seen per case on an MI355X (ELBO relative / group-wise / entry-wise), matern32 then matern52:

    small3_M20        0.0e+00 / 3.5e-13 / 2.0e-11    2.4e-16 / 1.0e-12 / 1.6e-11
    small3_white_M20  1.2e-16 / 1.1e-11 / 4.1e-11    0.0e+00 / 2.4e-11 / 2.4e-11
    odd_M33           2.1e-15 / 3.0e-12 / 3.7e-09    2.0e-15 / 3.3e-12 / 2.2e-09
    mnist3_M72        1.5e-14 / 4.0e-11 / 6.1e-09    2.8e-15 / 1.9e-11 / 8.3e-09
    ch_M200           2.5e-15 / 4.5e-11 / 6.4e-08    4.7e-16 / 8.4e-12 / 1.7e-08
    ch_M384           1.3e-15 / 1.1e-11 / 8.3e-08    6.2e-15 / 1.2e-11 / 1.0e-07

Operators: K_uu within 6.7e-16 and K_uf within 3.6e-15 of the NumPy classes (variance 1.7; bound 1.7e-12), the coincident patch included; the
layer within 2.4e-15; three Adam steps within 6.5e-14, the SGD step 2.0e-14, the NatGrad step 7.7e-14; head marginals 2.4e-14, the input
gradient 5.1e-15 of |dX|max, the Gaussian ELBO 3.4e-16.
"""
import copy
import functools
import math
import os

import numpy as np
import pytest

from deepcgp_amd import synthetic as syn
from deepcgp_amd.models import build_from_spec
import live_specs as ls
import matern_ref as mr
import torch_ref as tr

pytestmark = pytest.mark.gpu

TOL_ELBO, TOL_GROUP, TOL_E = 1e-9, 1e-7, 1e-5
BASES = ("matern32", "matern52")
CASES = ("small3_M20", "small3_white_M20", "odd_M33", "mnist3_M72", "ch_M200", "ch_M384")
# (H, W, C, f, s, M): M not a multiple of 16, ragged strips, 250-entry patches, the 28 x 28 stride-2 first layer
GEOMS = [(12, 12, 1, 3, 1, 6), (13, 13, 2, 4, 3, 33), (14, 14, 10, 5, 1, 72), (28, 28, 1, 5, 2, 200)]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def _classes(base):
    from deepcgp_amd import kernels as K
    return (K.Matern32, mr.Matern32) if base == "matern32" else (K.Matern52, mr.Matern52)


# ---- operators ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("H,W,C,f,s,M", GEOMS)
def test_kuu_and_kuf_patches(ctx, base, H, W, C, f, s, M):
    """Kuu and kuf_patches (both output layouts) against the NumPy class, 1e-12 relative to the variance; Z[0] IS a patch of image 1
    (r2 = 0 off K_uu's diagonal): finite and within the same bound."""
    from oracle.views import FullView as OFullView
    from deepcgp_amd.layers import MultiOutputConvKernel
    from deepcgp_amd.views import FullView
    dcls, rcls = _classes(base)
    rng = np.random.default_rng(H + M)
    N, var = 3, 1.7
    X = rng.standard_normal((N, H, W, C))
    v, ov = FullView((H, W), f, C, s), OFullView((H, W), f, C, s)
    L, P = v.patch_length, v.patch_count
    PNL = ov.extract_patches_PNL(X)                                # [P, N, L]
    Z = rng.standard_normal((M, L))
    Z[0] = PNL[P // 2, 1]
    lsc = 0.9 * math.sqrt(L)
    k, rk = dcls(L, var, lsc), rcls(L, var, lsc)
    got = k.K(Z)
    want = rk.K(Z)
    assert np.all(np.isfinite(got)) and np.abs(got - want).max() <= 1e-12 * var, np.abs(got - want).max()
    gj = k._gram(Z, 1e-3)
    assert np.abs(gj - (want + 1e-3 * np.eye(M))).max() <= 1e-12 * var
    mok = MultiOutputConvKernel(k, H * W * C, P)
    pmn = mok.Kuf(Z, (X, v))                                       # layout 0: [P, M, N]
    want_pmn = np.stack([rk.K(Z, PNL[p]) for p in range(P)])
    assert pmn.shape == (P, M, N) and np.all(np.isfinite(pmn))
    err = np.abs(pmn - want_pmn).max()
    print("%s %s Kuu err %.2e Kuf err %.2e  coincident entry: got %.17g want %.17g" % (base, (H, W, C, f, s, M), np.abs(got - want).max(), err,
                                                                                      pmn[P // 2, 0, 1], want_pmn[P // 2, 0, 1]))
    assert err <= 1e-12 * var, err
    dX, dZ, out = ctx.to_device(X), ctx.to_device(Z), ctx.empty((M, N * P))
    k._kuf(ctx, dX, N, H, W, C, f, s, dZ, M, out, 1)               # layout 1: [M, N * P], column n * P + p
    assert np.array_equal(out.numpy().reshape(M, N, P), np.transpose(pmn, (1, 2, 0)))
    assert np.all(mok.Kdiag(PNL) == var)


def test_operator_argument_checks(ctx):
    from deepcgp_amd import device as dev
    from deepcgp_amd.kernels import Matern32
    Z = ctx.to_device(np.zeros((4, 9)))
    out = ctx.empty((4, 4))
    L = dev.lib()
    assert L.dcgp_kuu_matern(ctx.handle, Z.ptr, 4, 9, 4, 1.0, 1.0, 0.0, out.ptr) == dev.ERR_ARG      # nu2 not in {3, 5}
    assert L.dcgp_kuu_matern(ctx.handle, Z.ptr, 4, 9, 3, 1.0, 0.0, 0.0, out.ptr) == dev.ERR_ARG
    assert L.dcgp_kuf_patches_matern(ctx.handle, Z.ptr, 1, 2, 2, 1, 3, 1, Z.ptr, 4, 5, 1.0, 1.0, out.ptr, 0) == dev.ERR_ARG   # f > H
    with pytest.raises(ValueError):
        Matern32(9).K(np.zeros((4, 8)))


# ---- layer ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [False, True])
def test_conv_layer_against_the_oracle_layer(ctx, white):
    from oracle.layers import ConvLayer as OConvLayer
    from oracle.views import FullView as OFullView
    from deepcgp_amd.kernels import Matern52, PatchInducingFeatures
    from deepcgp_amd.layers import ConvLayer
    from deepcgp_amd.views import FullView
    rng = np.random.default_rng(12)
    H, W, C, f, s, M, R, N = 12, 12, 3, 5, 1, 24, 4, 3
    X = rng.standard_normal((N, H * W * C))
    v, ov = FullView((H, W), f, C, s), OFullView((H, W), f, C, s)
    Z, q_mu = rng.standard_normal((M, v.patch_length)), rng.standard_normal((M, R))
    q_sqrt = np.tril(rng.standard_normal((R, M, M))) * 0.2 + np.eye(M)[None]
    layer = ConvLayer(Matern52(v.patch_length, 1.3, 7.0), None, PatchInducingFeatures(Z), v, white=white, gp_count=R, q_mu=q_mu, q_sqrt=q_sqrt)
    olayer = OConvLayer(mr.Matern52(v.patch_length, 1.3, 7.0), None, Z, ov, white=white, gp_count=R, q_mu=q_mu, q_sqrt=q_sqrt)
    m, var = layer.conditional_ND(X)
    om, ovar = olayer.conditional_ND(X)
    print("layer white=%s mean %.2e var %.2e" % (white, rel(m, om), rel(var, ovar)))
    assert rel(m, om) <= 1e-9 and rel(var, ovar) <= 1e-9
    assert abs(layer.KL() - olayer.KL()) <= 1e-9 * abs(olayer.KL())
    z = rng.standard_normal((1, N, layer.num_outputs))
    smp, m2, v2 = layer.sample_from_conditional(X[None], z=z)
    assert rel(smp[0], om + z[0] * np.sqrt(ovar + 1e-3)) <= 1e-9 and np.array_equal(m2[0], m)


# ---- model value and gradients --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name, base):
    """(spec, X, Y, zs, e_t, want): the case with Matern conv layers and its torch reference, computed once per process."""
    pytest.importorskip("torch")
    spec, X, Y, zs = mr.matern_case(name, base)
    ref = tr.reference(spec, X, Y, zs)
    e_t, want = ref["parts"][0], ref["want"]
    ls.assert_live(name, want)
    return spec, X, Y, zs, e_t, want


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("case", CASES)
def test_elbo_and_gradient_match_torch_autograd(ctx, case, base):
    spec, X, Y, zs, e_t, want = _case(case, base)
    tag = "%s-%s" % (case, base)
    model = build_from_spec(spec, X, Y)
    e, grads = model.compute_gradients(X, Y, zs=zs)
    e_f = model.compute_log_likelihood(X, Y, zs=zs)
    rows = []
    for li, groups in enumerate(want):
        assert set(groups) == set(grads[li]), (tag, li)
        for name, w in groups.items():
            rows.append((li, name) + ls.errors(name, np.asarray(grads[li][name], np.float64), w))
            print("%s L%d %-14s group %.3e  entry %.3e  |want|max %.3e" % ((tag,) + rows[-1] + (np.abs(w).max(),)))
    print("%s elbo rel %.3e  WORST group %.3e entry %.3e" % (tag, abs(e - e_t) / abs(e_t), max(r[2] for r in rows), max(r[3] for r in rows)))
    assert abs(e - e_t) <= TOL_ELBO * abs(e_t), (tag, e, e_t)
    assert abs(e_f - e_t) <= TOL_ELBO * abs(e_t), (tag, "forward-only", e_f, e_t)
    for li, name, err_g, err_e in rows:
        assert err_g <= TOL_GROUP, (tag, li, name, "group-wise", err_g)
        assert err_e <= TOL_E, (tag, li, name, "entry-wise", err_e)
    for li, g in enumerate(grads):
        assert not np.triu(g["q_sqrt"], 1).any(), (tag, li, "q_sqrt above the diagonal")
    model.close()


def test_head_refuses_a_matern_base_kernel(ctx):
    """The device check `the head kernels are RBF-based` fires for the new types."""
    from deepcgp_amd import device as dev
    spec, X, Y, zs, _, _ = _case("small3_M20", "matern32")
    model = build_from_spec(spec, X, Y)
    model._build()
    desc = np.array([2.0, 1.0, 1.0, 0.0])
    rc = dev.lib().dcgp_model_set_param(model._model, len(model.layers) - 1, b"base_kernel", desc.ctypes.data, 4)
    assert rc == dev.ERR_ARG and b"RBF-based" in dev.lib().dcgp_last_error(ctx.handle)
    desc[0] = 4.0
    assert dev.lib().dcgp_model_set_param(model._model, 0, b"base_kernel", desc.ctypes.data, 4) == dev.ERR_ARG
    model.close()


# ---- optimisers -----------------------------------------------------------------------------------------------------------------------
def test_adam_steps_match_numpy_on_torch_gradients(ctx):
    """Three steps of the one-call Adam step on small3_M20 (Matern52) against NumPy Adam on torch gradients recomputed after every step:
    the scheme and the tolerances of test_adam_one_call_steps_match_numpy_on_torch_gradients_at_M200."""
    spec, X, Y, zs, _, _ = _case("small3_M20", "matern52")
    spec = copy.deepcopy(spec)
    N, lr, state = X.shape[0], 0.05, {}
    model = build_from_spec(spec, X, Y)
    for t in range(1, 4):
        z = syn.make_noise(spec, N, seed=100 + t)
        e = model.train_step(X, Y, lr, zs=z, t=t)
        ref = tr.reference(spec, X, Y, z)
        e_t, g = ref["parts"][0], ref["want"]
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
    assert type(model.layers[0].base_kernel).__name__ == "Matern52"
    model.close()


def test_sgd_step_follows_the_torch_gradient(ctx):
    """One sgd_step(lr) on small3_M20 (Matern52): every group = theta + lr * (torch gradient), the positive ones through the softplus, 1e-9
    relative (test_sgd_step_follows_the_torch_gradient_at_M200's scheme)."""
    spec, X, Y, zs, _, want = _case("small3_M20", "matern52")
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


def test_natgrad_step_matches_numpy_on_torch_gradients(ctx):
    """One natgrad_step on small3_M20 (Matern52) against tests/natgrad_ref.py fed the torch gradients, rel < 1e-8 (that file's bound in
    test_natgrad_step_matches_numpy_on_torch_gradients_at_M200)."""
    from natgrad_ref import natgrad_reference
    spec, X, Y, zs, _, want = _case("small3_M20", "matern52")
    gamma = 1e-5
    model = build_from_spec(spec, X, Y)
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.natgrad_step(gamma)
    model.pull_parameters()
    for li, (l, m) in enumerate(zip(spec["convs"] + [spec["head"]], model.layers)):
        mu1, L1 = natgrad_reference(np.asarray(l["q_mu"]), np.asarray(l["q_sqrt"]), want[li]["q_mu"], want[li]["q_sqrt"], gamma)
        print("natgrad L%d rel q_mu %.3e q_sqrt %.3e (moved %.3e / %.3e)" % (li, rel(m.q_mu, mu1), rel(m.q_sqrt, L1), rel(mu1, l["q_mu"]),
                                                                           rel(L1, l["q_sqrt"])))
        assert rel(m.q_mu, mu1) < 1e-8 and rel(m.q_sqrt, L1) < 1e-8, (li, rel(m.q_mu, mu1), rel(m.q_sqrt, L1))
    model.close()


# ---- downstream entry points ----------------------------------------------------------------------------------------------------------
def test_prediction_evaluation_and_input_gradient(ctx):
    """small3_M20 (Matern32): propagate / predict_y head marginals and class probabilities, evaluate's accuracy and mean log density, and
    input_gradient(objective="elbo") against the torch forward and its autograd with respect to X."""
    torch = pytest.importorskip("torch")
    import test_oracle_autograd as toa
    spec, X, Y, zs, _, _ = _case("small3_M20", "matern32")
    S, N = spec["S"], X.shape[0]
    out = tr.forward(spec, X, Y, zs, x_leaf=True)
    (gX,) = torch.autograd.grad(out["data"].sum(), out["X"])
    mean, var = out["mean"].detach(), out["var"].detach()
    model = build_from_spec(spec, X, Y)
    _, Fm, Fv = model.propagate(X, S=S, zs=zs)
    print("propagate mean %.2e var %.2e" % (rel(Fm[-1], mean.numpy()), rel(Fv[-1], var.numpy())))
    assert rel(Fm[-1], mean.numpy()) <= 1e-9 and rel(Fv[-1], var.numpy()) <= 1e-9
    p = toa._robustmax_predict(mean.reshape(S * N, -1), var.reshape(S * N, -1)).reshape(S, N, -1).numpy()
    py, pv = model.predict_y(X, S, zs=zs)
    assert rel(py, p) <= 1e-9 and rel(pv, p - p * p) <= 1e-9
    r = model.evaluate(X, Y, S=S, batch_size=N, zs=zs, per_image=True)
    want_ld = np.log(p[:, np.arange(N), Y].mean(0))
    assert r["accuracy"] == np.mean(p.mean(0).argmax(1) == Y)
    assert rel(r["log_density"], want_ld) <= 1e-9 and abs(r["mean_log_density"] - want_ld.mean()) <= 1e-9 * abs(want_ld.mean())
    J, dX = model.input_gradient(X, Y, objective="elbo", zs=zs)
    print("input gradient J %.2e dX %.2e of |dX|max %.3e" % (rel(J, out["data"].detach().numpy()), rel(dX, gX.numpy()), np.abs(gX.numpy()).max()))
    assert rel(J, out["data"].detach().numpy()) <= 1e-9
    assert np.abs(dX - gX.numpy()).max() <= 1e-9 * np.abs(gX.numpy()).max()
    model.close()


def test_gaussian_likelihood_elbo(ctx):
    from deepcgp_amd.likelihoods import Gaussian
    spec, X, _, zs, _, _ = _case("small3_M20", "matern52")
    Yf = np.random.default_rng(2).standard_normal((X.shape[0], spec["head"]["R"]))
    e_t = tr.forward(spec, X, Yf, zs, ve=tr.gaussian_rule(Yf, 0.7))["elbo"].item()
    model = build_from_spec(spec, X, Yf, likelihood=Gaussian(0.7))
    e = model.compute_log_likelihood(X, Yf, zs=zs)
    print("gaussian elbo rel %.3e" % (abs(e - e_t) / abs(e_t)))
    assert abs(e - e_t) <= 1e-9 * abs(e_t)
    model.close()


# ---- the flag, training and checkpoints -----------------------------------------------------------------------------------------------
def test_model_builder_trains_and_reloads_a_matern52_model(ctx, tmp_path):
    """--base-kernel matern52 through ModelBuilder: two Adam steps, save_model_parameters, a rebuild with --load-model under the same flag
    gives the same ELBO to 1e-12; then train() with Adam and with NatGrad on the device."""
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.kernels import Matern52, RBF
    from deepcgp_amd.models import ModelBuilder, save_model_parameters, train
    rng = np.random.default_rng(3)
    X = rng.random((40, 12, 12, 1))
    Y = rng.integers(0, 10, size=(40, 1)).astype(np.int32)
    flags = default_parser().parse_args(['--name', 't', '-M', '6,7', '--feature-maps', '3', '--filter-sizes', '3,3', '--strides', '2,1',
                                         '--num-samples', '2', '--batch-size', '8', '--base-kernel', 'matern52'])
    np.random.seed(0)
    a = ModelBuilder(flags, X, Y).build()
    assert type(a.layers[0].base_kernel) is Matern52 and type(a.layers[1].kern.base_kernel) is RBF
    Xb, Yb = X[:8].reshape(8, -1), Y[:8]
    zs = [rng.standard_normal((2, 8, l.num_outputs)) for l in a.layers]
    e0 = a.compute_log_likelihood(Xb, Yb, zs=zs)
    # (the conv layer's inducing patches stay where they are: a rebuilt model takes the KL prior's frozen patches from the checkpoint's Z,
    # conv_gp/layers.py:149-152, so a model whose Z has moved away from its prior's does not reload to the same ELBO with any base kernel)
    a.set_trainable(0, "Z", False)
    for t in (1, 2):
        a.train_step(Xb, Yb, 0.02, zs=zs, t=t)
    a.pull_parameters()
    e_a = a.compute_log_likelihood(Xb, Yb, zs=zs)
    assert np.isfinite(e_a) and e_a != e0 and a.layers[0].base_kernel.lengthscales != 5.0
    path = os.path.join(str(tmp_path), "t.npy")
    saved = save_model_parameters(a, path, global_step=2)
    assert saved['DGP/layers/0/conv_kernel/base_kernel/lengthscales'] == a.layers[0].base_kernel.lengthscales      # RBF's keys
    flags.load_model = 't'
    bld = ModelBuilder(flags, X, Y, model_path=path)
    b = bld.build()
    flags.load_model = None
    assert bld.global_step == 2 and type(b.layers[0].base_kernel) is Matern52
    e_b = b.compute_log_likelihood(Xb, Yb, zs=zs)
    print("checkpoint: elbo %.15g reloaded %.15g" % (e_a, e_b))
    assert abs(e_b - e_a) <= 1e-12 * abs(e_a)
    for opt in ("Adam", "NatGrad"):
        hist = train(b, 2, lr=0.01, seed=4, optimizer=opt)
        assert len(hist) == 2 and all(np.isfinite(hist)), (opt, hist)
    a.close(), b.close()

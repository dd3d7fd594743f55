"""Input gradients on the device (DGP_Base.input_gradient / dcgp_model_input_grad, csrc/input_grad.hip) against PyTorch autograd through
the independently written forward of tests/input_grad_ref.py and against the float64 oracle's per-image objectives; the training state
the call must leave alone; reproducibility; FGSM at the model level; error paths."""
import numpy as np
import pytest

import input_grad_ref as R
from deepcgp_amd.likelihoods import Bernoulli, Gaussian
from deepcgp_amd.models import adversarial_examples, build_from_spec

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


# (family, objective, white, dedup_layer0, M, S, N): a pruned product -- every family with both objectives, white and dedup both ways, M on
# either side of 256 (the one-launch and the sweep + GEMM forward routes), S in {1, 3}, N in {1, 5, 33}
CASES = [
    ("head_mnist", "density", False, False, 17, 3, 5), ("head_mnist", "elbo", True, True, 256, 1, 5), ("head_mnist", "density", True, False, 384, 3, 1),
    ("conv_head_cfg2", "density", False, True, 17, 3, 5), ("conv_head_cfg2", "elbo", False, False, 256, 3, 1), ("conv_head_cfg2", "elbo", True, False, 17, 1, 5),
    ("three_ragged", "density", False, False, 17, 3, 5), ("three_ragged", "elbo", True, True, 17, 3, 33), ("three_ragged", "elbo", False, True, 17, 1, 1),
    ("cifar3", "density", True, True, 17, 3, 5), ("cifar3", "elbo", False, False, 17, 3, 5),
    ("acos", "density", False, False, 17, 3, 5), ("acos", "elbo", True, True, 17, 3, 5),
    ("identity_mean", "density", False, True, 17, 3, 5), ("identity_mean", "elbo", True, False, 17, 3, 5),
    ("dense_ard", "density", False, False, 17, 3, 5), ("dense_ard", "elbo", True, True, 17, 3, 33),
    ("additive", "density", True, False, 17, 3, 5), ("additive", "elbo", False, True, 17, 3, 5),
    ("conv_small", "density", False, False, 384, 1, 33), ("conv_small", "elbo", False, True, 256, 3, 5), ("conv_small", "density", True, True, 17, 3, 33),
    ("head_small", "elbo", False, True, 17, 3, 5),
    # 256 rows and more at a short-patch RBF layer: the fused patch adjoint (below that the product + col2im pair); L = 9, 18 and 48 elements
    ("conv_small", "density", False, False, 17, 8, 33), ("head_small", "elbo", True, False, 17, 8, 33), ("cifar3", "density", False, False, 17, 8, 33),
    ("identity_mean", "elbo", False, False, 17, 8, 33),
]


@pytest.mark.parametrize("name,objective,white,dedup,M,S,N", CASES)
def test_input_gradient_matches_torch_autograd(ctx, name, objective, white, dedup, M, S, N):
    """dX against autograd at the project's gradient tolerance (test_device_gradient_matches_torch_autograd's), J against the oracle's
    per-image objective (predict_y-derived density / E_log_p_Y) and against predict_density, 1e-9 relative."""
    spec, X, Y, zs = R.make_case(name, white=white, M=M, S=S, N=N)
    Jw, want = R.autograd_input_gradient(spec, X, Y, zs, objective=objective)
    Jo = R.oracle_objective(R.oracle_for(spec, X, Y), spec, X, Y, zs, objective=objective)
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    J, got = model.input_gradient(X, Y, objective=objective, zs=zs)
    assert got.shape == X.shape and J.shape == (N,)
    err = np.abs(got - want).max()
    print("%s %s white=%d dedup=%d M=%d S=%d N=%d: |dX - autograd| = %.3e, |want|max = %.3e, J vs oracle %.3e, vs torch %.3e"
          % (name, objective, white, dedup, M, S, N, err, np.abs(want).max(), rel(J, Jo), rel(J, Jw)))
    if objective == "density":   # the value predict_density returns for the same noise
        ld = model.predict_density(X, Y, S, zs=zs).reshape(-1)
        print("   J vs predict_density %.3e" % rel(J, ld))
        assert rel(J, ld) <= 1e-9
    # ... and the oracle's per-image objective, 1e-9: what "elbo" is checked against, and asserted for "density" as well.  One family's
    # density is held to 2e-8 instead: the unwhitened ArcCosine model's VALUE is not pinned to 1e-9 by float64 itself.  K_uu's diagonal is
    # acos at 1 - 1e-15, where one ulp of the cosine moves K by ~1e-9 (the device evaluates that cosine in its own order, common.h
    # BaseKernel), and two CPU references -- the oracle, and input_grad_ref's forward with K_uu evaluated by torch instead of NumPy --
    # disagree by 4.4e-9 on this very case (1.7e-10 whitened); 2e-8 is under five times that.  The device's figure here is 2.6e-9.
    bound = 2e-8 if (objective == "density" and name == "acos" and not white) else 1e-9
    assert rel(J, Jo) <= bound, (J, Jo)
    assert err <= 1e-7 * max(1.0, np.abs(want).max()), (err, np.abs(want).max())
    model.close()


@pytest.mark.parametrize("like,dedup,white", [("gaussian", False, False), ("gaussian", True, True), ("bernoulli", True, False), ("bernoulli", False, True)])
def test_float_target_models_elbo_objective(ctx, like, dedup, white):
    spec, X, Ylab, zs = R.make_case("conv_small", white=white, head_outputs=3)
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((X.shape[0], 3)) if like == "gaussian" else (rng.random((X.shape[0], 3)) > 0.5).astype(np.float64)
    kw = dict(objective="elbo", likelihood=like, s2=0.7 if like == "gaussian" else None)
    Jw, want = R.autograd_input_gradient(spec, X, Y, zs, **kw)
    Jo = R.oracle_objective(R.oracle_for(spec, X, Ylab), spec, X, Y, zs, **kw)
    model = build_from_spec(spec, X, Y, likelihood=Gaussian(0.7) if like == "gaussian" else Bernoulli())
    model.dedup_layer0 = dedup
    J, got = model.input_gradient(X, Y, objective="elbo", zs=zs)
    err = np.abs(got - want).max()
    print("%s dedup=%d white=%d: |dX - autograd| = %.3e, |want|max = %.3e, J vs oracle %.3e" % (like, dedup, white, err, np.abs(want).max(), rel(J, Jo)))
    assert rel(J, Jo) <= 1e-9
    assert err <= 1e-7 * max(1.0, np.abs(want).max())
    with pytest.raises(NotImplementedError):
        model.input_gradient(X, Y, objective="density", zs=zs)
    model.close()


def _grad_blocks(model):
    from deepcgp_amd import device as dev
    L, out = dev.lib(), []
    for li, l in enumerate(model.layers):
        head = li == len(model.layers) - 1
        M, Rr = l.num_inducing, (l.num_outputs if head else l.gp_count)
        shapes = {"Z": (M, np.shape(l.feature.Z)[1]), "q_mu": (M, Rr), "q_sqrt": (Rr, M, M), "variance": (), "lengthscale": ()}
        if head:
            shapes["w"] = (np.size(l.kern.patch_weights),)
        for which, shp in shapes.items():
            buf = np.empty(shp, np.float64)
            model._ctx._check(L.dcgp_model_get_grad(model._model, li, which.encode(), buf.ctypes.data, buf.size))
            out.append(buf)
    return out


def _params(model):
    model.pull_parameters()
    out = []
    for li, l in enumerate(model.layers):
        kern = l.kern.base_kernel if li == len(model.layers) - 1 else l.base_kernel
        out += [np.array(l.feature.Z), np.array(l.q_mu), np.array(l.q_sqrt), np.array(kern.variance), np.array(kern.lengthscales)]
    out.append(np.array(model.layers[-1].kern.patch_weights))
    return out


@pytest.mark.parametrize("objective", ["density", "elbo"])
def test_training_state_is_untouched(ctx, objective):
    spec, X, Y, zs = R.make_case("three_ragged", M=17, S=3, N=5)
    a, b = build_from_spec(spec, X, Y), build_from_spec(spec, X, Y)
    for m in (a, b):
        m.compute_gradients(X, Y, zs=zs, fetch=False)
    before = _grad_blocks(a)
    a.input_gradient(X, Y, objective=objective, zs=zs)
    a.dedup_layer0 = True
    a.input_gradient(X, Y, objective=objective, seed=3)
    a.dedup_layer0 = False
    after = _grad_blocks(a)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    for m in (a, b):
        m.adam_step(0.01)
    assert all(np.array_equal(x, y) for x, y in zip(_params(a), _params(b)))
    # a second step: the moments and the step count were left alone as well
    for m in (a, b):
        m.compute_gradients(X, Y, zs=zs, fetch=False)
    a.input_gradient(X, Y, objective=objective, zs=zs)
    for m in (a, b):
        m.adam_step(0.01)
    assert all(np.array_equal(x, y) for x, y in zip(_params(a), _params(b)))
    a.close(), b.close()


def test_factor_reuse_keeps_its_chain(ctx):
    """With factor reuse on, an evaluation's chain stands across input_gradient calls (which use it) and the evaluation after them."""
    spec, X, Y, zs = R.make_case("conv_small", M=17, S=3, N=5)
    model = build_from_spec(spec, X, Y)
    model.set_factor_reuse(1)
    p0 = model.predict_proba(X, 3, zs=zs)
    k0 = model.chain_skips
    J1, g1 = model.input_gradient(X, Y, zs=zs)
    k1 = model.chain_skips
    assert k1 == k0 + 1                       # the call reused the chain ...
    p1 = model.predict_proba(X, 3, zs=zs)
    assert model.chain_skips == k1 + 1        # ... and left it valid
    assert np.array_equal(p0, p1)
    model.set_factor_reuse(0)
    J2, g2 = model.input_gradient(X, Y, zs=zs)
    assert model.chain_skips == k1 + 1
    assert np.array_equal(g1, g2) and np.array_equal(J1, J2)
    model.close()


@pytest.mark.parametrize("name,M,N,dedup_bound", [("conv_head_cfg2", 256, 5, 1e-12), ("three_ragged", 17, 33, 1e-12), ("head_mnist", 384, 5, 5e-12)])
def test_bitwise_repeatable_and_dedup_agrees(ctx, name, M, N, dedup_bound):
    """Two calls with the same arguments: the same bits.  dedup_layer0 on / off differ in summation order only: 1e-12 relative, measured
    6.4e-14 (conv + head, M = 256) and 1.2e-15 (three layers).  The head-only model at M = 384 measures 1.5e-12 -- with dedup_layer0 its one
    layer runs on N rows instead of S N, so every product of the sweep + GEMM route is tiled and split differently, behind a 384 x 384
    factorisation -- and is held to 5e-12, about three times the measured figure."""
    spec, X, Y, zs = R.make_case(name, M=M, S=3, N=N)
    model = build_from_spec(spec, X, Y)
    res = {}
    for dedup in (False, True):
        model.dedup_layer0 = dedup
        J1, g1 = model.input_gradient(X, Y, zs=zs)
        J2, g2 = model.input_gradient(X, Y, zs=zs)
        assert np.array_equal(g1, g2) and np.array_equal(J1, J2)
        s1 = model.input_gradient(X, Y, seed=11)[1]
        assert np.array_equal(s1, model.input_gradient(X, Y, seed=11)[1])
        res[dedup] = g1
    d = rel(res[True], res[False])
    print("%s: dedup on / off differ by %.3e relative" % (name, d))
    assert d <= dedup_bound
    model.close()


def test_saliency_shape_and_own_prediction(ctx):
    spec, X, Y, zs = R.make_case("cifar3", M=17, S=3, N=5)
    model = build_from_spec(spec, X, Y)
    sal = model.saliency(X, zs=zs)
    assert sal.shape == (5, 12, 12, 3)
    yhat = model.predict_proba(X, 3, zs=zs).argmax(1)
    assert np.array_equal(sal.reshape(5, -1), model.input_gradient(X, yhat, zs=zs)[1])
    model.close()


def test_fgsm_lowers_the_density(ctx):
    """epsilon is chosen on the CPU from the oracle: the largest of 1e-2, 1e-3, 1e-4 at which the oracle's own density drops for every image
    under the autograd-sign perturbation (the condition on the inputs); the device is then held to the same."""
    spec, X, Y, zs = R.make_case("conv_small", M=17, S=3, N=5)
    ref = R.oracle_for(spec, X, Y)
    J0, g = R.autograd_input_gradient(spec, X, Y, zs)
    assert np.all(np.abs(g).max(1) > 0)
    lo, hi = float(X.min()), float(X.max())
    eps = None
    for e in (1e-2, 1e-3, 1e-4):
        Xa = np.clip(X - e * np.sign(g), lo, hi)
        if np.all(R.oracle_objective(ref, spec, Xa, Y, zs) < R.oracle_objective(ref, spec, X, Y, zs)):
            eps = e
            break
    assert eps is not None
    model = build_from_spec(spec, X, Y)
    adv = adversarial_examples(model, X, Y, eps, clip=(lo, hi), zs=zs)
    assert adv.shape == X.shape and np.abs(adv - X).max() <= eps * (1 + 1e-12) and adv.min() >= lo and adv.max() <= hi
    clean, attacked = model.predict_density(X, Y, 3, zs=zs), model.predict_density(adv, Y, 3, zs=zs)
    print("eps %g: density clean %s -> adversarial %s" % (eps, clean.ravel(), attacked.ravel()))
    assert np.all(attacked < clean)
    it = adversarial_examples(model, X, Y, eps, steps=3, clip=(lo, hi), zs=zs)
    assert np.abs(it - X).max() <= eps * (1 + 1e-12) and it.min() >= lo and it.max() <= hi
    assert np.all(model.predict_density(it, Y, 3, zs=zs) < clean)
    model.close()


def test_error_paths(ctx):
    from deepcgp_amd import device as dev
    spec, X, Y, zs = R.make_case("conv_small", M=17, S=3, N=5)
    model = build_from_spec(spec, X, Y)
    J, g = model.input_gradient(X[:0], Y[:0])
    assert J.shape == (0,) and g.shape == (0, X.shape[1])
    assert model._model is None                # N = 0 made no device call: the device model does not exist yet
    model.input_gradient(X, Y, zs=zs)
    bad = Y.copy()
    bad[2] = 10
    with pytest.raises(ValueError):
        model.input_gradient(X, bad, zs=zs)
    with pytest.raises(Exception) as ei:       # labels already on the device: the library's own check
        model.input_gradient(X, model._ctx.to_device(bad, np.int32), zs=zs)
    assert "labels outside" in str(ei.value)
    with pytest.raises(ValueError):
        model.input_gradient(X, Y, objective="logit")
    with pytest.raises(ValueError):
        model.input_gradient(X, Y, S=0)
    info = dev.C.c_int(0)
    dX = model._ctx.to_device(X)
    dY = model._ctx.to_device(Y, np.int32)
    out = model._ctx.empty(X.shape)
    rc = dev.lib().dcgp_model_input_grad(model._model, dX.ptr, dY.ptr, 5, 3, None, 0, 7, None, out.ptr, dev.C.byref(info))
    assert rc == dev.ERR_ARG
    rc = dev.lib().dcgp_model_input_grad(model._model, dX.ptr, dY.ptr, 0, 3, None, 0, 0, None, out.ptr, dev.C.byref(info))
    assert rc == dev.ERR_ARG
    # the model still works
    assert np.all(np.isfinite(model.input_gradient(X, Y, zs=zs)[1]))
    model.close()

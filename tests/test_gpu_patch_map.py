"""GPU: per-patch evidence maps (csrc/patch_map.hip) -- dcgp_convkernel_patch_mean against the NumPy restatement and against
dcgp_convkernel_kzx, SVGP_Layer.patch_contributions, DGP_Base.predict_patch_contributions (dcgp_model_patch_evidence) and the error paths.
Tolerances are those of test_gpu_full_cov.py: 1e-10 operator level against float64 NumPy, 1e-9 model level, 1e-8 against the oracle's
hidden-layer samples; rel(a, b) = max|a - b| / max|b|.  A sum over patches cancels, so it is held against the absolute sum."""
import ctypes as C

import numpy as np
import pytest

import oracle.dgp as odgp
from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.kernels import JITTER, RBF, AdditivePatchKernel, ConvKernel
from deepcgp_amd.likelihoods import Bernoulli, Gaussian
from deepcgp_amd.models import build_from_spec, build_layers_from_spec
from deepcgp_amd.views import FullView
from oracle_build import oracle_layers
from patch_map_ref import head_patch_mean, patch_mean

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def sum_err(c, total):
    """max|sum_p c - total| relative to max_n sum_p |c| (c [..., P, R], total [..., R])."""
    return np.max(np.abs(c.sum(-2) - total)) / max(np.max(np.sum(np.abs(c), -2)), 1e-300)


GEOMS = {   # (H, W, C, f, stride)
    "mnist_head": (28, 28, 1, 5, 1),        # cfg1 / cfg2 / cfg5 head-only: P = 576, L = 25
    "mnist_conv_head": (12, 12, 10, 5, 1),  # behind one conv layer (cfg2 / cfg5 conv + head): P = 64, L = 250
    "mnist3_head": (9, 9, 10, 5, 1),        # behind two conv layers (cfg3): P = 25, L = 250
    "cifar3_head": (11, 11, 10, 5, 1),      # behind two conv layers (cfg4): P = 49
    "cifar_rgb": (32, 32, 3, 4, 2),         # a CIFAR-shaped 3-channel image: P = 225, L = 48
    "ragged": (7, 6, 2, 3, 2),              # stride 2, H != W: P = 6, L = 18
    "wide": (6, 13, 1, 3, 1),               # H != W, L = 9
}
# every M in {1, 17, 32, 256, 384, 1024}, R in {1, 10, 16, 23}, N in {1, 3, 33}
CASES = [
    ("mnist_head", 32, 10, 3), ("mnist_head", 256, 10, 33), ("mnist_head", 1024, 23, 3), ("mnist_head", 1, 1, 1),
    ("mnist_conv_head", 256, 10, 33), ("mnist_conv_head", 1024, 16, 3), ("mnist_conv_head", 17, 23, 1),
    ("mnist3_head", 256, 10, 33), ("mnist3_head", 17, 1, 3),
    ("cifar3_head", 384, 10, 33), ("cifar3_head", 384, 23, 3),
    ("cifar_rgb", 384, 16, 3), ("cifar_rgb", 17, 10, 33),
    ("ragged", 17, 23, 33), ("ragged", 1, 16, 1), ("ragged", 32, 1, 3),
    ("wide", 32, 10, 33), ("wide", 17, 16, 1),
]


def make_problem(geom, M, R, N, seed=0, additive=False, scale=1.0, ls=None):
    H, W, Cc, f, s = geom
    view = FullView((H, W, Cc), f, Cc, s)
    rng = np.random.default_rng(seed)
    w = 0.5 + rng.random(view.patch_count)
    ls = ls if ls is not None else 0.4 * np.sqrt(view.patch_length) + 0.5
    kern = (AdditivePatchKernel if additive else ConvKernel)(RBF(view.patch_length, 5.0, ls), view, patch_weights=w)
    X = rng.standard_normal((N, H * W * Cc)) * 0.7 * scale
    # inducing patches: patches of the images themselves, moved by a fraction of the lengthscale (kernel values of order one)
    pt = view_patches(X, geom)
    rows = rng.integers(0, pt.shape[0], M)
    Z = pt[rows] + 0.3 * ls / np.sqrt(view.patch_length) * rng.standard_normal((M, view.patch_length))
    beta = rng.standard_normal((M, R))
    return kern, X, Z, beta


def view_patches(X, geom):
    from patch_map_ref import patches
    p = patches(X, geom)
    return p.reshape(-1, p.shape[-1])


@pytest.mark.parametrize("name,M,R,N", CASES)
def test_patch_mean_vs_numpy(ctx, name, M, R, N):
    geom = GEOMS[name]
    kern, X, Z, beta = make_problem(geom, M, R, N, seed=M + R + N, additive=(M + N) % 2 == 1)
    got = kern.patch_mean(Z, X, beta)
    assert got.shape == (N, kern.patch_count, R)
    bk = kern.base_kernel
    want = patch_mean(X, geom, Z, bk.variance, bk.lengthscales, kern.patch_weights, beta)
    print("patch_mean", name, M, R, N, "rel", rel(got, want))
    assert np.all(np.isfinite(got))
    assert rel(got, want) <= 1e-10, rel(got, want)


@pytest.mark.parametrize("name,M,R,N", [c for c in CASES if c[1] <= 384])
def test_patch_mean_sums_to_kzx(ctx, name, M, R, N):
    """The defining invariant on the device alone: sum_p out[n, p, :] = Kzx^T beta."""
    kern, X, Z, beta = make_problem(GEOMS[name], M, R, N, seed=7 + M + N)
    got = kern.patch_mean(Z, X, beta)
    total = kern.Kzx(Z, X).T @ beta
    e = sum_err(got, total)
    print("sum invariant", name, M, R, N, e)
    assert e <= 1e-10, e


@pytest.mark.parametrize("ls", [0.3, 50.0])
@pytest.mark.parametrize("name", ["ragged", "cifar3_head", "mnist_head"])
def test_patch_mean_large_arguments(ctx, name, ls):
    """Inputs scaled by 30: c |x|^2 far above 1024 at the short lengthscale, columns beyond the last patch must stay finite.  The
    inducing patches sit within a fraction of a lengthscale of the image's patches, so that the kernel values are of order one and the
    comparison says something (random ones give exact zeros at lengthscale 0.3); the reference takes its squared distances from the
    differences themselves.  Strips with c |x|^2 > 2^16 run the kernel's exact form (every case at 0.3); the MFMA form alone measured
    8.3e-10 at cifar3_head 0.3, which is why the exact form exists."""
    geom = GEOMS[name]
    for N in (1, 6):
        kern, X, Z, beta = make_problem(geom, 24, 10, N, seed=40 + N, scale=30.0 / 0.7, ls=ls)
        got = kern.patch_mean(Z, X, beta)
        assert np.all(np.isfinite(got))
        want = patch_mean(X, geom, Z, 5.0, ls, kern.patch_weights, beta, exact=True)
        print("large arguments", name, ls, N, "rel", rel(got, want), "max|want|", np.max(np.abs(want)))
        assert rel(got, want) <= 1e-10, rel(got, want)


def test_patch_mean_needs_scalar_rbf(ctx):
    kern, X, Z, beta = make_problem(GEOMS["ragged"], 4, 2, 2)
    L = dev.lib()
    dX, dZ, dw, db = (ctx.to_device(a) for a in (X, Z, kern.patch_weights, beta))
    out = ctx.to_device(np.full((2, 6, 2), 7.0))
    args = lambda N, f, R: (ctx.handle, dX.ptr, N, 7, 6, 2, f, 2, dZ.ptr, 4, 5.0, 1.0, dw.ptr, db.ptr, R, out.ptr)
    assert L.dcgp_convkernel_patch_mean(*args(-1, 3, 2)) == dev.ERR_ARG
    assert L.dcgp_convkernel_patch_mean(*args(2, 8, 2)) == dev.ERR_ARG      # f > H
    assert L.dcgp_convkernel_patch_mean(*args(2, 3, 0)) == dev.ERR_ARG      # R < 1
    assert L.dcgp_convkernel_patch_mean(ctx.handle, None, 2, 7, 6, 2, 3, 2, dZ.ptr, 4, 5.0, 1.0, dw.ptr, db.ptr, 2, out.ptr) == dev.ERR_ARG
    assert L.dcgp_convkernel_patch_mean(*args(0, 3, 2)) == 0                # N == 0: nothing written
    assert np.all(out.numpy() == 7.0)


HEADS = {"conv": ((12, 12, 10), (5, 1), 24, "conv"), "add": ((11, 11, 10), (5, 1), 20, "add"), "mnist": ((28, 28, 1), (5, 1), 32, "conv")}


def head_layer(case, white, seed=3):
    hwc, head, M, hk = HEADS[case]
    spec = syn.make_spec(hwc, [], head, M, seed=seed, white=white, head_q_sqrt_scale=0.7)
    if hk == "add":
        spec["head"]["kernel"] = "add"
    spec["head"]["w"] = 0.5 + np.random.default_rng(seed).random(spec["head"]["w"].size)
    return spec, build_layers_from_spec(spec)[-1]


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("case", list(HEADS))
def test_layer_patch_contributions(ctx, case, white):
    spec, layer = head_layer(case, white)
    X, _ = syn.make_batch(HEADS[case][0], 9, seed=7)
    c = layer.patch_contributions(X)
    R, P = spec["head"]["R"], layer.kern.patch_count
    assert c.shape == (9, P, R)
    mean, _ = layer.conditional_ND(X)
    e = sum_err(c, mean)
    print("layer", case, white, e)
    assert e <= 1e-9, e
    assert rel(c, head_patch_mean(spec["head"], X, JITTER)) <= 1e-9
    assert layer.patch_contributions(X[:0]).shape == (0, P, R)
    maps = layer.kern.view.as_maps(c)
    assert maps.shape == (9, layer.kern.view.out_image_height, layer.kern.view.out_image_width, R)


def test_layer_patch_contributions_errors(ctx):
    _, layer = head_layer("conv", False)
    X, _ = syn.make_batch(HEADS["conv"][0], 3, seed=1)
    import deepcgp_amd.layers as L
    old = L.JITTER
    try:
        L.JITTER = -1e6   # K_uu + jitter I with a negative first pivot
        with pytest.raises(dev.NotPositiveDefinite) as e:
            layer.patch_contributions(X)
        assert e.value.column == 1
    finally:
        L.JITTER = old
    spec = syn.make_spec((6, 6, 4), [], (5, 1), 16, seed=3, head_kernel="rbf")
    dense = build_layers_from_spec(spec)[-1]
    with pytest.raises((TypeError, NotImplementedError)):
        dense.patch_contributions(np.zeros((2, 6 * 6 * 4)))


MODELS = {   # hwc, convs, head, M, N, S
    "head_only": ((28, 28, 1), [], (5, 1), 32, 5, 3),
    "conv_head": ((28, 28, 1), [(5, 2, 10)], (5, 1), 24, 5, 2),
    "cifar3": ((32, 32, 3), [(4, 2, 10), (5, 1, 10)], (5, 1), 16, 4, 2),
}


def make_model(case, lik, white=False, seed=21):
    hwc, convs, head, M, N, S = MODELS[case]
    D = {"multiclass": 10, "gaussian": 3, "bernoulli": 2}[lik]
    spec = syn.make_spec(hwc, convs, head, M, S=S, num_data=1000, seed=seed, conv_q_sqrt_scale=0.2, white=white, head_outputs=D)
    spec["head"]["w"] = 0.5 + np.random.default_rng(seed).random(spec["head"]["w"].size)
    X, Ylab = syn.make_batch(hwc, N, seed=seed)
    rng = np.random.default_rng(seed)
    if lik == "gaussian":
        Y, like = rng.standard_normal((N, D)), Gaussian(0.7)
    elif lik == "bernoulli":
        Y, like = (rng.random((N, D)) < 0.5).astype(np.float64), Bernoulli()
    else:
        Y, like = Ylab, None
    model = build_from_spec(spec, X, Y) if like is None else build_from_spec(spec, X, Y, likelihood=like)
    return spec, X, Y, model, N, S


def oracle_maps(spec, X, S, zs):
    """The restatement on the oracle's own hidden-layer samples."""
    layers = oracle_layers(spec)
    F = np.tile(X[None], [S, 1, 1])
    for layer, z in zip(layers[:-1], zs[:-1]):
        F, _, _ = odgp.sample_from_conditional(layer, F, z=z)
    return np.stack([head_patch_mean(spec["head"], F[s_], JITTER) for s_ in range(S)])


def check_model(model, spec, X, S, N, seed):
    c, fm = model.predict_patch_contributions(X, S, seed=seed)
    P, R = model.layers[-1].kern.patch_count, spec["head"]["R"]
    assert c.shape == (S, N, P, R) and fm.shape == (S, N, R)
    want_fm, _ = model.predict_f(X, S, seed=seed)
    assert np.array_equal(fm, want_fm)
    e = sum_err(c, fm)
    print("model sum", e)
    assert e <= 1e-9, e
    return c, fm


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("lik", ["multiclass", "gaussian", "bernoulli"])
@pytest.mark.parametrize("case", list(MODELS))
def test_model_patch_contributions(ctx, case, lik, white):
    spec, X, Y, model, N, S = make_model(case, lik, white)
    try:
        c, fm = check_model(model, spec, X, S, N, seed=4)
        # two identical calls: bit-identical
        c2, fm2 = model.predict_patch_contributions(X, S, seed=4)
        assert np.array_equal(c, c2) and np.array_equal(fm, fm2)
        # explicit noise: against the restatement on the oracle's hidden-layer samples
        zs = syn.make_noise(spec, N, seed=21)
        cz, fz = model.predict_patch_contributions(X, S, zs=zs)
        want = oracle_maps(spec, X, S, zs)
        print("model vs oracle", case, lik, white, rel(cz, want))
        assert rel(cz, want) <= 1e-8, rel(cz, want)
        assert np.array_equal(fz, model.predict_f(X, S, zs=zs)[0])
        e0 = model.predict_patch_contributions(X[:0], S)
        assert e0[0].shape == (S, 0, c.shape[2], c.shape[3]) and e0[1].shape == (S, 0, c.shape[3])
    finally:
        model.close()


@pytest.mark.parametrize("case", ["head_only", "conv_head"])
def test_model_patch_contributions_follow_training(ctx, case):
    spec, X, Y, model, N, S = make_model(case, "multiclass")
    try:
        before, _ = check_model(model, spec, X, S, N, seed=2)
        model.train_step(X, Y, 1e-2, seed=1)
        after, _ = check_model(model, spec, X, S, N, seed=2)
        assert not np.array_equal(before, after)
        again, _ = model.predict_patch_contributions(X, S, seed=2)
        assert np.array_equal(after, again)
    finally:
        model.close()


def test_model_patch_contributions_errors(ctx):
    # a dense RBF-ARD head has no patches: the Python method and the C entry both say so
    hwc = (10, 10, 1)
    spec = syn.make_spec(hwc, [(3, 1, 2)], (3, 1), 9, S=2, num_data=300, seed=7, head_kernel="rbf")
    X, Y = syn.make_batch(hwc, 4, seed=7)
    dense = build_from_spec(spec, X, Y)
    try:
        with pytest.raises((TypeError, NotImplementedError)):
            dense.predict_patch_contributions(X, 2)
        dense.predict_f(X, 2)   # builds the device model
        dX, out = ctx.to_device(X), ctx.empty((2 * 4 * 10,))
        info = C.c_int(0)
        rc = dev.lib().dcgp_model_patch_evidence(dense._model, dX.ptr, 4, 2, None, 0, out.ptr, None, C.byref(info))
        assert rc == dev.ERR_ARG
    finally:
        dense.close()
    # a K_uu that cannot be factored: the code comes back, nothing faults
    spec, X, Y, model, N, S = make_model("conv_head", "multiclass")
    try:
        good, _ = model.predict_patch_contributions(X, S, seed=1)
        L = dev.lib()
        dX = ctx.to_device(X)
        out = ctx.to_device(np.full(good.shape, 7.0))
        info = C.c_int(0)
        assert L.dcgp_model_patch_evidence(model._model, dX.ptr, 0, S, None, 0, out.ptr, None, C.byref(info)) == 0   # N == 0
        assert np.all(out.numpy() == 7.0)
        assert L.dcgp_model_patch_evidence(model._model, dX.ptr, -1, S, None, 0, out.ptr, None, C.byref(info)) == dev.ERR_ARG
        assert L.dcgp_model_patch_evidence(model._model, dX.ptr, N, 0, None, 0, out.ptr, None, C.byref(info)) == dev.ERR_ARG
        assert L.dcgp_model_patch_evidence(model._model, None, N, S, None, 0, out.ptr, None, C.byref(info)) == dev.ERR_ARG
        assert L.dcgp_model_patch_evidence(model._model, dX.ptr, N, S, None, 0, None, None, C.byref(info)) == dev.ERR_ARG
        Z = model.layers[-1].feature.Z.copy()
        model.layers[-1].feature.Z = np.full_like(Z, np.nan)
        model.sync_parameters()
        with pytest.raises(dev.NotPositiveDefinite):
            model.predict_patch_contributions(X, S, seed=1)
        model.layers[-1].feature.Z = Z
        model.sync_parameters()
        back, _ = model.predict_patch_contributions(X, S, seed=1)
        assert np.array_equal(back, good)
    finally:
        model.close()

"""GPU: the operators of csrc/transfer.hip -- dcgp_cross_gram and dcgp_inducing_transfer -- against the NumPy mirror of tests/reselect_ref.py,
and ``DGP_Base.reselect_inducing`` on small live models (second half of the file): candidates, optimiser state, a fresh model's ELBO and steps.

Tolerances.  cross_gram: 1e-12 of the variance (one kernel evaluation; the rounding of a distance of size d ~ 250 is ~1e-13 relative to it and
enters the entry through the exponent).  Transfer: 1e-8 of the tensor's largest entry.  cond(K + jI) <= (M variance + j) / j ~ 3.5e5 at M = 70,
variance 5, j = 1e-3; times 2.2e-16 that is ~1e-10, two orders inside the bound, and S' keeps its smallest eigenvalue above j (test_host_reselect).

Shapes: M, M' below and above one another, no multiples of the 16-row padding, and 70 crosses the factorisation's 32- and 64-column panels; L
shorter and longer than the cross Gram kernel's 32-element staging step (d = 250: eight steps, the last partial)."""
import ctypes as C

import numpy as np
import pytest

import reselect_ref as rr

pytestmark = pytest.mark.gpu

VARIANCE = 5.0
JITTER = 1e-3
KERNELS = ["rbf", "rbf_ard", "acos", "matern32", "matern52"]
SHAPES = [(24, 24), (24, 16), (16, 40), (70, 33), (70, 70)]


def make_kernel(kern, d, rng):
    """(device kernel object, the mirror's keyword arguments)."""
    from deepcgp_amd.kernels import RBF, ArcCosine, Matern32, Matern52
    ls = float(np.sqrt(d))
    if kern == "rbf":
        return RBF(d, VARIANCE, ls), dict(kind="rbf", variance=VARIANCE, p1=ls, p2=0.0, ard=None)
    if kern == "rbf_ard":
        ard = ls * rng.uniform(0.5, 1.5, d)
        return RBF(d, VARIANCE, ard, ARD=True), dict(kind="rbf", variance=VARIANCE, p1=1.0, p2=0.0, ard=ard)
    if kern == "matern32":
        return Matern32(d, VARIANCE, ls), dict(kind="matern32", variance=VARIANCE, p1=ls, p2=0.0, ard=None)
    if kern == "matern52":
        return Matern52(d, VARIANCE, ls), dict(kind="matern52", variance=VARIANCE, p1=ls, p2=0.0, ard=None)
    return ArcCosine(d, 0, VARIANCE, 1.0, 1.0), dict(kind="acos", variance=VARIANCE, p1=1.0, p2=1.0, ard=None)


def close(a, b, tol, name, scale=None):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    scale = float(np.max(np.abs(b))) if scale is None else scale
    err = float(np.max(np.abs(a - b))) / scale
    print("%s: max err / scale %.3e" % (name, err))
    assert err <= tol, "%s: max err / scale %.3e > %.1e" % (name, err, tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# cross_gram
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("d", [9, 250])
@pytest.mark.parametrize("m,n", [(24, 24), (24, 70), (70, 24), (70, 70)])
def test_cross_gram(ctx, m, n, d, kern):
    from deepcgp_amd.kernels import cross_gram
    rng = np.random.default_rng(1000 * m + 10 * n + d)
    A, B = rng.standard_normal((m, d)), rng.standard_normal((n, d))
    B[3] = A[5]                                    # a coincident pair: the off-diagonal form there too, no jitter
    bk, kw = make_kernel(kern, d, rng)
    got = cross_gram(A, B, bk)
    close(got, rr.cross(A, B, **kw), 1e-12, "cross_gram", scale=VARIANCE)
    off = rr.cross(A[5:6], A[5:6], **kw)[0, 0]     # what the formula gives on a coincident pair, not Kdiag + jitter
    assert abs(got[5, 3] - off) <= 1e-12 * VARIANCE


def test_cross_gram_errors(ctx):
    from deepcgp_amd.kernels import RBF, cross_gram
    bk = RBF(9, 1.0, 1.0)
    with pytest.raises(ValueError):
        cross_gram(np.zeros((4, 8)), np.zeros((4, 9)), bk)
    with pytest.raises(ValueError):
        cross_gram(np.zeros((4, 9)), np.zeros((0, 9)), bk)
    with pytest.raises(TypeError):
        cross_gram(np.zeros((4, 9)), np.zeros((4, 9)), object())


# ---------------------------------------------------------------------------------------------------------------------------------
# inducing_transfer
# ---------------------------------------------------------------------------------------------------------------------------------
_CASES = {}


def case(M, Mn, L, R, kern, scale=1.0):
    """Inputs of one transfer case: computed once, shared, never changed.  Z' shares two rows with Z."""
    key = (M, Mn, L, R, kern, scale)
    if key not in _CASES:
        rng = np.random.default_rng(100000 * M + 1000 * Mn + 10 * L + R)
        Z, Zn = rng.standard_normal((M, L)), rng.standard_normal((Mn, L))
        Zn[1], Zn[Mn - 1] = Z[2], Z[M - 1]
        bk, kw = make_kernel(kern, L, rng)
        q_mu, q_sqrt = rr.random_q(rng, M, R, scale)
        for v in (Z, Zn, q_mu, q_sqrt):
            v.setflags(write=False)
        _CASES[key] = (Z, Zn, bk, kw, q_mu, q_sqrt)
    return _CASES[key]


def check_transfer(M, Mn, L, R, kern, white):
    from deepcgp_amd.kernels import transfer_inducing
    Z, Zn, bk, kw, q_mu, q_sqrt = case(M, Mn, L, R, kern)
    mu, Ls = transfer_inducing(Z, Zn, bk, q_mu, q_sqrt, white=white, jitter=JITTER)
    mu_ref, Ls_ref = rr.transfer(Z, Zn, jitter=JITTER, q_mu=q_mu, q_sqrt=q_sqrt, white=white, **kw)
    close(mu, mu_ref, 1e-8, "q_mu'")
    close(Ls, Ls_ref, 1e-8, "q_sqrt'")
    iu = np.triu_indices(Mn, 1)
    assert np.all(Ls[:, iu[0], iu[1]] == 0.0), "upper triangle is not exact zeros"
    assert np.all(np.diagonal(Ls, axis1=1, axis2=2) > 0.0)
    return mu, Ls


@pytest.mark.parametrize("white", [0, 1])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("L", [9, 25])
@pytest.mark.parametrize("M,Mn", SHAPES)
def test_transfer_rbf(ctx, M, Mn, L, R, white):
    check_transfer(M, Mn, L, R, "rbf", white)


@pytest.mark.parametrize("white", [0, 1])
@pytest.mark.parametrize("kern", KERNELS[1:])
def test_transfer_kernels(ctx, kern, white):
    check_transfer(70, 33, 25, 3, kern, white)


@pytest.mark.parametrize("kern", ["rbf", "rbf_ard", "acos"])
def test_white_equals_unwhitened_on_converted_operands(ctx, kern):
    """The whitened call is the unwhitened call on (L m_w, L Lq_w), followed by inv(L') of its results."""
    from deepcgp_amd.kernels import transfer_inducing
    Z, Zn, bk, kw, m_w, Lq_w = case(70, 33, 25, 3, kern)
    Lk = np.linalg.cholesky(rr.gram(Z, jitter=JITTER, **kw))
    Ln = np.linalg.cholesky(rr.gram(Zn, jitter=JITTER, **kw))
    mu_w, Ls_w = transfer_inducing(Z, Zn, bk, m_w, Lq_w, white=True, jitter=JITTER)
    mu_u, Ls_u = transfer_inducing(Z, Zn, bk, Lk @ m_w, np.einsum("ij,rjk->rik", Lk, Lq_w), white=False, jitter=JITTER)
    close(Ln @ mu_w, mu_u, 1e-8, "L' q_mu'_w against q_mu'")
    close(np.einsum("ij,rjk->rik", Ln, Ls_w), Ls_u, 1e-8, "L' q_sqrt'_w against q_sqrt'")


@pytest.mark.parametrize("white", [0, 1])
def test_transfer_same_bits_every_run(ctx, white):
    from deepcgp_amd.kernels import transfer_inducing
    Z, Zn, bk, _, q_mu, q_sqrt = case(70, 70, 25, 3, "rbf")
    a = transfer_inducing(Z, Zn, bk, q_mu, q_sqrt, white=bool(white))
    b = transfer_inducing(Z, Zn, bk, q_mu, q_sqrt, white=bool(white))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def device_kl(ctx, q_mu, q_sqrt, K):
    from deepcgp_amd import device as dev
    M, R = q_mu.shape
    dm, dS = ctx.to_device(q_mu), ctx.to_device(q_sqrt)
    dK = ctx.to_device(K) if K is not None else None
    out, info = C.c_double(0.0), C.c_int(0)
    ctx._check(dev.lib().dcgp_gauss_kl(ctx.handle, dm.ptr, dS.ptr, dK.ptr if dK else None, M, R, C.byref(out), C.byref(info)), info)
    return out.value


@pytest.mark.parametrize("white", [0, 1])
@pytest.mark.parametrize("M,Mn", [(24, 16), (24, 24), (16, 40), (70, 33)])
def test_kl_does_not_rise(ctx, M, Mn, white):
    """KL[q' || p'] <= KL[q || p] (data processing: q' and p' are q and p pushed through the same conditional), through dcgp_gauss_kl."""
    from deepcgp_amd.kernels import transfer_inducing
    Z, Zn, bk, _, q_mu, q_sqrt = case(M, Mn, 9, 3, "rbf")
    mu, Ls = transfer_inducing(Z, Zn, bk, q_mu, q_sqrt, white=bool(white), jitter=JITTER)
    before = device_kl(ctx, q_mu, q_sqrt, None if white else bk._gram(Z, JITTER))
    after = device_kl(ctx, mu, Ls, None if white else bk._gram(Zn, JITTER))
    print("KL %.9g -> %.9g" % (before, after))
    assert np.isfinite(after) and after <= before * (1.0 + 1e-9)


def test_small_q_sqrt_transfers(ctx):
    """The 1e-5-scaled q_sqrt a conv layer starts with: chol(S') succeeds (S' >= Kn - B^T B, whose smallest eigenvalue is ~2 jitter)."""
    from deepcgp_amd.kernels import transfer_inducing
    Z, Zn, bk, kw, q_mu, q_sqrt = case(24, 24, 9, 3, "rbf", scale=1e-5)
    mu, Ls = transfer_inducing(Z, Zn, bk, q_mu, q_sqrt, jitter=JITTER)
    mu_ref, Ls_ref = rr.transfer(Z, Zn, jitter=JITTER, q_mu=q_mu, q_sqrt=q_sqrt, **kw)
    close(mu, mu_ref, 1e-8, "q_mu'")
    close(Ls, Ls_ref, 1e-8, "q_sqrt'")


def test_not_positive_definite_leaves_outputs(ctx):
    """jitter = 0 and a duplicated row in Z': K(Z', Z') is singular.  The not-PD code, info names a matrix, the output buffers keep their bits."""
    from deepcgp_amd import device as dev
    from deepcgp_amd.kernels import transfer_inducing
    Z, Zn, bk, _, q_mu, q_sqrt = case(24, 16, 9, 3, "rbf")
    Zd = Zn.copy()
    Zd[1] = Zd[0]
    M, Mn, L, R = 24, 16, 9, 3
    marker_mu, marker_S = np.full((Mn, R), 7.25), np.full((R, Mn, Mn), -3.5)
    dZ, dZn, dm, dS = ctx.to_device(Z), ctx.to_device(Zd), ctx.to_device(q_mu), ctx.to_device(q_sqrt)
    om, oS = ctx.to_device(marker_mu), ctx.to_device(marker_S)
    info = (C.c_int * 2)(0, 0)
    rc = dev.lib().dcgp_inducing_transfer(ctx.handle, dZ.ptr, M, dZn.ptr, Mn, L, 0, bk.variance, bk.lengthscales, 0.0, None, 0.0, 0, dm.ptr,
                                          dS.ptr, R, om.ptr, oS.ptr, info)
    print("rc %d info %d %d" % (rc, info[0], info[1]))
    assert rc == dev.ERR_NOT_PD
    assert info[0] >= 2 and info[1] >= 1           # K(Z', Z') or an S', never K(Z, Z)
    assert om.numpy().tobytes() == marker_mu.tobytes() and oS.numpy().tobytes() == marker_S.tobytes()
    with pytest.raises(dev.NotPositiveDefinite) as e:
        transfer_inducing(Z, Zd, bk, q_mu, q_sqrt, jitter=0.0)
    assert e.value.which == info[0] and e.value.column == info[1]
    # the same call with the jitter in place goes through
    transfer_inducing(Z, Zd, bk, q_mu, q_sqrt, jitter=JITTER)


def test_transfer_errors(ctx):
    from deepcgp_amd.kernels import RBF, transfer_inducing
    bk = RBF(9, 1.0, 1.0)
    Z, q_mu, q_sqrt = np.zeros((4, 9)), np.zeros((4, 2)), np.zeros((2, 4, 4))
    with pytest.raises(ValueError):
        transfer_inducing(Z, np.zeros((4, 8)), bk, q_mu, q_sqrt)
    with pytest.raises(ValueError):
        transfer_inducing(Z, Z, bk, np.zeros((5, 2)), q_sqrt)
    with pytest.raises(ValueError):
        transfer_inducing(Z, Z, bk, q_mu, np.zeros((2, 4, 5)))


# ---------------------------------------------------------------------------------------------------------------------------------
# DGP_Base.reselect_inducing
# ---------------------------------------------------------------------------------------------------------------------------------
# Small live specs (tests/live_specs.py): 10 x 10 images, two conv layers (3 x 3 patches, 2 maps) and a head, M = 16, 40 training images.
HWC, NTRAIN, M_MODEL, SEED = (10, 10, 1), 40, 16, 11
VARIANTS = ["rbf", "matern32", "matern52", "acos", "ard", "mixed", "padded", "white", "dense", "additive"]


def variant_spec(variant):
    import live_specs as ls
    kw = dict(hwc=HWC, convs=[(3, 1, 2), (3, 1, 2)], head=(3, 1), M=M_MODEL, c=1.0, a=0.1, S=2)
    if variant == "white":
        kw["white"] = True
    if variant == "dense":
        kw["head_kernel"] = "rbf"
    if variant == "additive":
        kw["additive"] = True
    spec = ls.live_spec(**kw)
    rng = np.random.default_rng(3)
    for c in spec["convs"]:
        if variant in ("matern32", "matern52"):
            c["base"] = variant
        if variant == "acos":
            c["base"], c["acos"] = "acos", (1.3, 0.8, 0.6)
        if variant == "ard":
            c["ls"] = c["ls"] * rng.uniform(0.7, 1.4, c["f"] * c["f"] * c["C"])
    if variant == "mixed":          # layer 0: two latent GPs mixed into the two maps layer 1 reads
        spec["convs"][0]["mix_W"] = np.array([[0.9, -0.4], [0.3, 1.1]])
    if variant == "padded":         # layer 1 sees a one-pixel border: its output, the head's input, grows to 8 x 8
        spec["convs"][1]["pad"] = 1
        spec["head"]["H"] = spec["head"]["W"] = 8
        spec["head"]["w"] = 0.5 + rng.random(36)
    return spec


def trained_model(variant):
    """A model that has taken three Adam steps: trained Z and hyperparameters, moments that are not zero."""
    from deepcgp_amd import synthetic as syn
    from deepcgp_amd.models import build_from_spec
    spec = variant_spec(variant)
    X, Y = syn.make_batch(HWC, NTRAIN, seed=7)
    model = build_from_spec(spec, X, Y)
    model.attach_dataset()
    model.train_run(np.random.default_rng(5).integers(0, NTRAIN, (3, 4)), 0.01, seed=5)
    return spec, X, Y, model


def spec_from_model(spec, model):
    """The spec a FRESH model of the same values is built from: every parameter as the model holds it, the conv layers' prior patches too."""
    import copy
    model.pull_parameters()
    out = copy.deepcopy(spec)
    for c, l in zip(out["convs"] + [out["head"]], model.layers):
        head = c is out["head"]
        c["Z"], c["q_mu"], c["q_sqrt"] = np.array(l.feature.Z), np.array(l.q_mu), np.array(l.q_sqrt)
        kern = (l.kern.base_kernel if hasattr(l.kern, "base_kernel") else l.kern) if head else l.base_kernel
        if hasattr(kern, "weight_variances"):
            c["acos"] = (kern.variance, kern.weight_variances, kern.bias_variance)
        else:
            c["variance"] = float(kern.variance)
            if head and "ls_ard" in c:
                c["ls_ard"] = np.array(kern.lengthscales)
            else:
                c["ls"] = np.array(kern.lengthscales) if np.ndim(kern.lengthscales) else float(kern.lengthscales)
        if head:
            if hasattr(l.kern, "patch_weights"):
                c["w"] = np.array(l.kern.patch_weights)
        else:
            c["Z0"] = np.array(l.Z_prior)
            if l.mixing is not None:
                c["mix_W"] = np.array(l.mixing)
    return out


def host_candidates(model, X, seed, images, candidates):
    """Every layer's candidates, cut again on the host from one propagation with the call's seeds -- written out here, not through the
    model's helpers: the image draw is RandomState([seed, 0]), layer li's patches RandomState([seed, 1 + li])."""
    from deepcgp_amd.models import draw_patches
    idx = np.random.RandomState(np.array([seed, 0], np.uint32)).choice(X.shape[0], size=min(images, X.shape[0]), replace=False)
    Fs, _, _ = model.propagate(X[idx], S=1, seed=seed)
    out = []
    for li, l in enumerate(model.layers):
        src = X[idx] if li == 0 else Fs[li - 1][0]
        head = li == len(model.layers) - 1
        v = getattr(l.kern, "view", None) if head else l.view
        if v is None:
            out.append(src.reshape(src.shape[0], -1))
            continue
        img = src.reshape(src.shape[0], v.input_size[0], v.input_size[1], v.feature_maps)
        p = v.padding
        img = np.pad(img, ((0, 0), (p, p), (p, p), (0, 0)))
        out.append(draw_patches(img, candidates * l.num_inducing, v.filter_size, np.random.RandomState(np.array([seed, 1 + li], np.uint32))))
    return out


def all_bits(model):
    model.pull_parameters()
    out = {p.pathname: np.array(p.value) for p in model.parameters}
    out.update({"prior/%d" % li: np.array(l.Z_prior) for li, l in enumerate(model.layers[:-1])})
    out.update({"opt/" + k: np.asarray(v) for k, v in model.optimizer_state().items()})
    return out


@pytest.mark.parametrize("variant", VARIANTS)
def test_reselect_model(ctx, variant):
    from deepcgp_amd.models import build_from_spec
    spec, X, Y, model = trained_model(variant)
    images, cands = 30, 20
    before = all_bits(model)
    want_cand = host_candidates(model, X, SEED, images, cands)
    np.random.seed(123)
    state = np.random.get_state()[1].copy()
    report = model.reselect_inducing(images=images, seed=SEED, candidates=cands)
    assert np.array_equal(np.random.get_state()[1], state), "the global generator was used"
    after = all_bits(model)
    assert [r["layer"] for r in report] == [0, 1, 2]
    nl = len(model.layers)
    for r in report:
        li, l = r["layer"], model.layers[r["layer"]]
        # every new inducing input is one of the candidates, the one the report names
        np.testing.assert_array_equal(l.feature.Z, want_cand[li][r["rows"]])
        assert len(set(r["rows"].tolist())) == M_MODEL and 0 <= r["n_greedy"] <= M_MODEL
        assert np.isfinite([r["trace_old"], r["trace_new"], r["kl_before"], r["kl_after"]]).all()
        assert r["trace_new"] >= 0.0 and r["trace_old"] >= -1e-9 * len(want_cand[li])
        print(variant, li, "n_greedy", r["n_greedy"], "trace %.6g -> %.6g" % (r["trace_old"], r["trace_new"]),
              "KL %.6g -> %.6g" % (r["kl_before"], r["kl_after"]))
        if li < nl - 1:
            np.testing.assert_array_equal(l.Z_prior, l.feature.Z)
        iu = np.triu_indices(M_MODEL, 1)
        assert np.all(l.q_sqrt[:, iu[0], iu[1]] == 0.0) and np.all(np.diagonal(l.q_sqrt, axis1=1, axis2=2) > 0.0)
    # the optimiser: the three groups' moments are zero, every other moment and t keep their bits
    assert after["opt/t"] == before["opt/t"] == 3
    for k in before:
        if not k.startswith("opt/") or k == "opt/t":
            continue
        group = k.split("/")[3] if k.startswith("opt/layers/") else k
        if group in ("Z", "q_mu", "q_sqrt"):
            assert np.any(before[k]) and not np.any(after[k]), k
        else:
            assert after[k].tobytes() == before[k].tobytes(), k
    # a FRESH model built from (Z', q_mu', q_sqrt', Z0 = Z') gives the same ELBO: no stale prior, factor or buffer survives
    fresh = build_from_spec(spec_from_model(spec, model), X, Y)
    Xb, Yb = X[:6], Y[:6]
    e_model, e_fresh = model.compute_log_likelihood(Xb, Yb, seed=9), fresh.compute_log_likelihood(Xb, Yb, seed=9)      # (the device's draws)
    print(variant, "ELBO %.12g fresh %.12g" % (e_model, e_fresh))
    assert np.isfinite(e_model) and abs(e_model - e_fresh) <= 1e-9 * abs(e_fresh)
    # five more steps: finite, and bit for bit the fresh model's from the same optimiser state
    fresh.set_optimizer_state(model.optimizer_state())
    fresh.attach_dataset()
    idx = np.random.default_rng(6).integers(0, NTRAIN, (5, 4))
    ea, eb = model.train_run(idx, 0.01, seed=40), fresh.train_run(idx, 0.01, seed=40)
    assert np.all(np.isfinite(ea)) and ea.tobytes() == eb.tobytes()
    a, b = all_bits(model), all_bits(fresh)
    assert set(a) == set(b)
    for k in a:
        assert np.all(np.isfinite(a[k])), k
        assert a[k].tobytes() == b[k].tobytes(), k
    model.close()
    fresh.close()


def test_reselect_with_a_kept_factor_chain(ctx):
    """set_factor_reuse(1): an evaluation keeps the parameter-only chain; the re-selection must invalidate it."""
    from deepcgp_amd.models import build_from_spec
    spec, X, Y, model = trained_model("rbf")
    model.set_factor_reuse(1)
    model.predict_y(X[:5], 2, seed=3)
    model.predict_y(X[:5], 2, seed=3)                    # (this one reuses the chain of the first)
    model.reselect_inducing(images=30, seed=SEED, candidates=20)
    fresh = build_from_spec(spec_from_model(spec, model), X, Y)
    got, want = model.predict_y(X[:5], 2, seed=3), fresh.predict_y(X[:5], 2, seed=3)
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w, rtol=1e-9, atol=1e-12)
    model.close()
    fresh.close()


def test_reselect_selected_layers_only(ctx):
    spec, X, Y, model = trained_model("rbf")
    before = all_bits(model)
    report = model.reselect_inducing(layers=[1], images=30, seed=SEED, candidates=20)
    after = all_bits(model)
    assert [r["layer"] for r in report] == [1]
    for k in before:
        touched = "/layers/1/" in k and k.split("/")[-1] in ("Z", "q_mu", "q_sqrt") or k == "prior/1" or k.startswith("opt/layers/1/") and \
            k.split("/")[3] in ("Z", "q_mu", "q_sqrt")
        if not touched:
            np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    assert not np.array_equal(after["DGP/layers/1/feature/Z"], before["DGP/layers/1/feature/Z"])
    model.close()


def test_failing_reselect_leaves_the_model(ctx, monkeypatch):
    """Too few candidates at the dense head (ValueError) and a transfer that fails at the LAST layer (NotPositiveDefinite), both after the
    layers below were computed: every parameter, prior and moment keeps its bits."""
    from deepcgp_amd import device as dev
    from deepcgp_amd import kernels
    spec, X, Y, model = trained_model("dense")
    before = all_bits(model)
    with pytest.raises(ValueError):
        model.reselect_inducing(images=M_MODEL - 1, seed=SEED, candidates=20)      # 15 flat rows for M = 16
    real, calls = kernels.transfer_inducing, []

    def failing(*a, **kw):
        calls.append(1)
        if len(calls) == 3:
            raise dev.NotPositiveDefinite(dev.ERR_NOT_PD, "inducing_transfer: S' of output 0 is not positive definite at column 1", 1)
        return real(*a, **kw)
    monkeypatch.setattr(kernels, "transfer_inducing", failing)
    with pytest.raises(dev.NotPositiveDefinite):
        model.reselect_inducing(images=30, seed=SEED, candidates=20)
    assert len(calls) == 3
    after = all_bits(model)
    assert set(after) == set(before)
    for k in before:
        assert after[k].tobytes() == before[k].tobytes(), k
    with pytest.raises(ValueError):
        model.reselect_inducing(layers=[5])
    model.global_batch = 8                                  # what set_shard leaves behind
    with pytest.raises(NotImplementedError):
        model.reselect_inducing()
    model.close()

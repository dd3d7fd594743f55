"""Dilated conv layers on the device (``FullView(dilation=d)``, ``--dilations``, dcgp_model_set_dilation; csrc/dilate.hip) against a torch
forward whose patch extraction is ``unfold(..., dilation=d)`` and against the undilated physical layer on NumPy space-to-batch
(tests/dilation_ref.py).

Tolerances are the project's own, imported: RTOL of tests/test_gpu_model.py (ELBO, data term, KL), RTOL of tests/test_gpu_ops.py (layer
outputs), the gradient bounds tests/test_gpu_padding.py's gradient test applies (``grad_bounds``: tests/test_gpu_grad_m256.py's, or
tests/test_gpu_grad_large_m.py's above M = 256), its INPUT_GRAD_TOL, and RTOL of tests/test_gpu_evaluate.py."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.models import build_from_spec

import dilation_ref as dr
import live_specs as ls
import stack_specs as ss
import test_gpu_padding as tgp
from test_gpu_evaluate import RTOL as RTOL_EVAL
from test_gpu_model import RTOL
from test_gpu_ops import RTOL as RTOL_OPS
import torch_ref as tr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]   # a hung launch ends the run instead of holding the device

rel, grad_bounds, INPUT_GRAD_TOL = tgp.rel, tgp.grad_bounds, tgp.INPUT_GRAD_TOL
STACKS = list(dr.STACKS)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(spec, X, Y, zs) of a stack, once per process; never written to."""
    return dr.make_stack(name)


@functools.lru_cache(maxsize=None)
def _torch(name):
    pytest.importorskip("torch")
    spec, X, Y, zs = _case(name)
    return tr.reference(spec, X, Y, zs)


# ---- 1. the stacks against torch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedup", [False, True], ids=["tiled", "dedup"])
@pytest.mark.parametrize("name", STACKS)
def test_dilated_stacks_match_the_torch_forward(ctx, name, dedup):
    """ELBO, data term, KL and every layer's mean and variance from ``predict_all_layers``."""
    spec, X, Y, zs = _case(name)
    t = _torch(name)
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    got = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    for what, g, w in zip(("elbo", "data", "kl"), got, t["parts"]):
        print("%s%s %-4s device %.9f torch %.9f rel %.3e" % (name, "-dedup" if dedup else "", what, g, w, abs(g - w) / max(abs(w), 1.0)))
    _, Fm, Fv = model.predict_all_layers(X, spec["S"], zs=zs)
    for i in range(len(Fm)):
        print("%s layer %d mean %.3e var %.3e" % (name, i, rel(Fm[i], t["means"][i]), rel(Fv[i], t["vars"][i])))
    e, data, kl = t["parts"]
    assert abs(got[0] - e) <= RTOL * abs(e) and abs(got[1] - data) <= RTOL * abs(data) and abs(got[2] - kl) <= RTOL * max(abs(kl), 1.0), (got, t["parts"])
    assert [m.shape[-1] for m in Fm] == [o for _, o in ss.output_dims(spec)]
    for i in range(len(Fm)):
        assert rel(Fm[i], t["means"][i]) < RTOL_OPS and rel(Fv[i], t["vars"][i]) < RTOL_OPS, (name, i)
    assert model.compute_log_likelihood(X, Y, zs=zs, return_parts=True) == got          # the other bank (and its split batch): the same bits
    model.close()


# ---- 2. the device identity --------------------------------------------------------------------------------------------------------------
def _physical(spec):
    """The undilated physical model of layer 0: that layer with the same parameters on its phase geometry, no padding, and a small patch head of
    its own on the phase output (the model needs one; its values are not compared)."""
    c = copy.deepcopy(spec["convs"][0])
    d, p = c.pop("dil"), c.pop("pad", 0)
    c["H"], c["W"] = ss.phase_size(c["H"], c["W"], p, d)
    Rout = c["R"] if c.get("mix_W") is None else np.shape(c["mix_W"])[1]
    Hq, Wq = c["H"] - c["f"] + 1, c["W"] - c["f"] + 1
    head = ls.live_spec((Hq, Wq, Rout), [], (2, 1), 12, 1.0, 0.1, S=spec["S"], seed=3)["head"]
    return {"S": spec["S"], "num_data": spec["num_data"], "convs": [c], "head": head}, d, p


def _identity(spec, X, Y, zs):
    """Layer 0's sample, mean and var of the dilated model against the physical layer fed s2b(pad(X)) and s2b(z), through NumPy b2s: to the bit,
    tiled and de-duplicated."""
    c0 = spec["convs"][0]
    phys, d, p = _physical(spec)
    S, N = spec["S"], X.shape[0]
    H, W, Cc = c0["H"], c0["W"], c0["C"]
    Ho, Wo = ss.out_size(H, W, c0["f"], 1, p, d)
    G = c0["R"]
    Xs = dr.s2b(np.pad(X.reshape(N, H, W, Cc), ((0, 0), (p, p), (p, p), (0, 0))), d)
    Xs = Xs.reshape(Xs.shape[0], -1)
    z0 = dr.s2b(zs[0].reshape(S * N, Ho, Wo, G), d).reshape(S, N * d * d, -1)
    zp = [z0, np.zeros((S, N * d * d, phys["head"]["R"]))]
    dilated, physical = build_from_spec(spec, X, Y), build_from_spec(phys, Xs, np.zeros(Xs.shape[0], np.int32))
    for dedup in (False, True):
        dilated.dedup_layer0 = physical.dedup_layer0 = dedup
        a = dilated.propagate(X, S=S, zs=zs)
        b = physical.propagate(Xs, S=S, zs=zp)
        for what, x, y in zip(("sample", "mean", "var"), a, b):
            Rout = x[0].shape[-1] // (Ho * Wo)
            back = dr.b2s(y[0].reshape(S * N * d * d, -(-Ho // d), -(-Wo // d), Rout), d, Ho, Wo).reshape(x[0].shape)
            print("dedup=%d layer 0 %s bit-identical %s (max diff %.3e)" % (dedup, what, np.array_equal(x[0], back), np.abs(x[0] - back).max()))
            assert np.array_equal(x[0], back), (dedup, what)
    dilated.close(), physical.close()


@pytest.mark.parametrize("name", ["dil2", "dil2_odd", "dil3_pad"])
def test_a_dilated_first_layer_is_the_physical_layer_on_space_to_batch(ctx, name):
    _identity(*_case(name))


# ---- 3. the default ----------------------------------------------------------------------------------------------------------------------
def test_all_one_dilations_is_the_model_without_the_flag(ctx):
    """``--dilations 1,1`` and no flag: the same model on the same path, the same bits (ELBO parts and a gradient)."""
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder
    rng = np.random.default_rng(0)
    X = rng.standard_normal((40, 14, 14, 1))
    Y = rng.integers(0, 10, (40, 1))
    args = ['--name', 't', '-M', '6,7,8', '--feature-maps', '3,2', '--filter-sizes', '3,3,3', '--strides', '2,1,1', '--num-samples', '2', '--batch-size', '8']
    models = []
    for extra in ([], ['--dilations', '1,1']):
        np.random.seed(0)
        models.append(ModelBuilder(default_parser().parse_args(args + extra), X, Y).build())
    a, b = models
    for la, lb in zip(a.layers, b.layers):
        assert np.array_equal(la.feature.Z, lb.feature.Z)
    Xb, Yb = X[:8].reshape(8, -1), Y[:8].reshape(-1)
    zs = [np.random.default_rng(3 + i).standard_normal((2, 8, l.num_outputs)) for i, l in enumerate(a.layers)]
    ea, eb = (m.compute_log_likelihood(Xb, Yb, zs=zs, return_parts=True) for m in (a, b))
    print("no flag %r  --dilations 1,1 %r" % (ea, eb))
    assert ea == eb and all(np.isfinite(ea))
    (_, ga), (_, gb) = (m.compute_gradients(Xb, Yb, zs=zs) for m in (a, b))
    for da, db in zip(ga, gb):
        for k in da:
            assert np.array_equal(da[k], db[k]), k
    a.close(), b.close()


def test_model_builder_with_dilations_from_flags(ctx):
    """``--dilations 2,1 --paddings 2,0,0`` through ModelBuilder (inducing patches clustered from dilated windows of the
    zero-padded images): the ELBO at explicit noise against the torch forward built from the same parameters, and three training steps."""
    pytest.importorskip("torch")
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder, train
    from oracle_build import spec_from_model
    rng = np.random.default_rng(0)
    np.random.seed(0)
    X = rng.standard_normal((40, 10, 10, 1))
    Y = rng.integers(0, 10, (40, 1))
    flags = default_parser().parse_args(['--name', 't', '-M', '6,7,8', '--feature-maps', '2,2', '--filter-sizes', '3,3,3', '--strides', '1,1,1',
                                         '--dilations', '2,1', '--paddings', '2,0,0', '--num-samples', '2', '--batch-size', '8'])
    model = ModelBuilder(flags, X, Y).build()
    views = [l.view for l in model.layers[:-1]] + [model.layers[-1].kern.view]
    assert [(v.input_size[0], v.padding, v.dilation, v.out_image_height) for v in views] == [(10, 2, 2, 10), (10, 0, 1, 8), (8, 0, 1, 6)]
    for l in model.layers:
        l.q_mu = 0.3 * rng.standard_normal(l.q_mu.shape)
    model.sync_parameters()
    spec = spec_from_model(model)
    for e, v in zip(spec["convs"], views):
        e.update(pad=v.padding, dil=v.dilation, H=v.input_size[0], W=v.input_size[1])
    Xb, Yb = X[:8].reshape(8, -1), Y[:8].reshape(-1)
    zs = ss.make_noise(spec, 8, seed=3)
    e = model.compute_log_likelihood(Xb, Yb, zs=zs)
    want = tr.reference(spec, Xb, Yb, zs)["parts"][0]
    print("--dilations 2,1: ELBO %.9f torch %.9f rel %.3e" % (e, want, abs(e - want) / abs(want)))
    assert abs(e - want) <= RTOL * abs(want), (e, want)
    hist = train(model, 3)
    assert len(hist) == 3 and np.all(np.isfinite(hist)), hist
    model.close()


# ---- 4. gradients ------------------------------------------------------------------------------------------------------------------------
def _check_gradients(tag, spec, X, Y, zs, t, dedup):
    ls.assert_live(tag, t["want"])
    tol_group, tol_e = grad_bounds(spec)
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    got_parts = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    e, grads = model.compute_gradients(X, Y, zs=zs)
    e2, grads2 = model.compute_gradients(X, Y, zs=zs)
    rows = []
    for li, groups in enumerate(t["want"]):
        assert set(groups) == set(grads[li]), (tag, li, sorted(groups), sorted(grads[li]))
        for gname, w in groups.items():
            got = np.asarray(grads[li][gname], np.float64)
            assert got.shape == np.shape(w), (tag, li, gname, got.shape, np.shape(w))
            rows.append((li, gname) + ls.errors(gname, got, w))
            print("%s L%d %-14s group %.3e  entry %.3e  |want|max %.3e" % ((tag,) + rows[-1] + (np.abs(w).max(),)))
    e_t = t["parts"][0]
    print("%s elbo rel %.3e  WORST group %.3e entry %.3e" % (tag, abs(e - e_t) / abs(e), max(r[2] for r in rows), max(r[3] for r in rows)))
    for g, w in zip(got_parts, t["parts"]):
        assert abs(g - w) <= RTOL * max(abs(w), 1.0), (tag, got_parts, t["parts"])
    assert abs(e - e_t) <= RTOL * abs(e), (tag, e, e_t)
    for li, gname, err_g, err_e in rows:
        assert err_g <= tol_group, (tag, li, gname, "group-wise", err_g)
        assert err_e <= tol_e, (tag, li, gname, "entry-wise", err_e)
    assert e == e2
    for a, b in zip(grads, grads2):
        for k in a:
            assert np.array_equal(a[k], b[k]), (tag, k, "repeat")
    model.close()


@pytest.mark.parametrize("dedup", [False, True], ids=["tiled", "dedup"])
@pytest.mark.parametrize("name", STACKS)
def test_gradient_matches_torch_autograd_through_unfold(ctx, name, dedup):
    """Every group of every layer, group-wise and entry-wise over the floor (tests/live_specs.py: errors); the ELBO parts against torch."""
    spec, X, Y, zs = _case(name)
    _check_gradients(name + ("-dedup" if dedup else ""), spec, X, Y, zs, _torch(name), dedup)


# ---- 5. input gradient -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedup", [False, True], ids=["tiled", "dedup"])
@pytest.mark.parametrize("objective", ["density", "elbo"])
@pytest.mark.parametrize("name", ["dil3_pad", "dil2_odd"])
def test_input_gradient_is_in_the_callers_geometry(ctx, name, objective, dedup):
    """dX [N, H W C] of the caller's unpadded, undilated images (batch-to-space, the crop and the replica sum of a tiled batch) against
    autograd through the pad and the unfold."""
    pytest.importorskip("torch")
    spec, X, Y, zs = _case(name)
    Jw, want = tr.input_gradient(spec, X, Y, zs, tr.robustmax_objective(Y, objective))
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    J, got = model.input_gradient(X, Y, objective=objective, zs=zs)
    err = np.abs(got - want).max()
    print("%s %s dedup=%d: |dX - autograd| %.3e  |want|max %.3e  J rel %.3e" % (name, objective, dedup, err, np.abs(want).max(), rel(J, Jw)))
    assert got.shape == X.shape == want.shape and J.shape == (X.shape[0],)
    assert np.abs(want).max() > 1e-6
    assert rel(J, Jw) <= RTOL
    assert err <= INPUT_GRAD_TOL * max(1.0, np.abs(want).max()), (err, np.abs(want).max())
    model.close()


# ---- 6. compositions ---------------------------------------------------------------------------------------------------------------------
def _compose(kind):
    """(spec, X, Y, zs) of a small dilated stack with one more feature on its dilated layer."""
    if kind == "ard":
        spec, X, Y, zs = dr.make_stack("dil2_odd")
        spec = copy.deepcopy(spec)
        c = spec["convs"][0]
        c["ls"] = c["ls"] * (0.8 + 0.4 * np.random.default_rng(7).random(c["f"] * c["f"] * c["C"]))
        return spec, X, Y, zs
    if kind == "matern52":
        spec, X, Y, zs = dr.make_stack("dil3_pad")
        spec = copy.deepcopy(spec)
        spec["convs"][0]["base"] = "matern52"
        return spec, X, Y, zs
    if kind == "mixing":      # G = 2 latent GPs -> R = 3 maps on a dilated layer with phantoms, S = 3
        from deepcgp_amd.layers import mixing_matrix
        k = dict(hwc=(9, 7, 2), head=(3, 1, 0), Ms=12, S=3)
        spec = ss.stack_spec(convs=[(3, 1, 3, 0, 2)], **k)
        lat = ss.stack_spec(convs=[(3, 1, 2, 0, 2)], **k)["convs"][0]
        lat.update(mix_W=0.7 * mixing_matrix("random", 2, 3, seed=5), mix_trainable=True)
        spec["convs"][0] = lat
        X, Y = syn.make_batch(k["hwc"], 3, seed=7)
        return spec, X, Y, ss.make_noise(spec, 3, seed=7)
    assert kind == "filter_mean"      # a dilated residual block: Cin == Cout, p = d, LinearConv2dMean("channels", trainable)
    from deepcgp_amd.mean_functions import conv_mean_filter
    spec = ss.stack_spec(hwc=(9, 9, 2), convs=[(3, 1, 2, 2, 2)], head=(3, 2, 0), Ms=12)
    spec["convs"][0].update(mean_filter=conv_mean_filter("channels", 3, 2, 2), mean_trainable=True)
    X, Y = syn.make_batch((9, 9, 2), 3, seed=7)
    return spec, X, Y, ss.make_noise(spec, 3, seed=7)


@pytest.mark.parametrize("dedup", [False, True], ids=["tiled", "dedup"])
@pytest.mark.parametrize("kind", ["ard", "matern52", "mixing", "filter_mean"])
def test_compositions_on_a_dilated_layer(ctx, kind, dedup):
    """The forward (in ``_check_gradients``: ELBO, data term, KL) and every gradient group -- ``lengthscales`` [L], ``mixing``, ``mean_filter``
    among them -- against torch autograd.  The mixed case has S = 3 and runs tiled and de-duplicated: its latent triple is in phase layout, the
    gradient from above in image layout."""
    pytest.importorskip("torch")
    spec, X, Y, zs = _compose(kind)
    t = tr.reference(spec, X, Y, zs)
    if kind == "filter_mean":
        c = spec["convs"][0]
        assert ss.out_size(c["H"], c["W"], c["f"], 1, c["pad"], c["dil"]) == (c["H"], c["W"])      # resolution kept
    _check_gradients("%s%s" % (kind, "-dedup" if dedup else ""), spec, X, Y, zs, t, dedup)
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    _, Fm, Fv = model.predict_all_layers(X, spec["S"], zs=zs)
    for i in range(len(Fm)):
        assert rel(Fm[i], t["means"][i]) < RTOL_OPS and rel(Fv[i], t["vars"][i]) < RTOL_OPS, (kind, i)
    model.close()


@pytest.mark.parametrize("kind", ["mixing", "filter_mean"])
def test_identity_for_the_mixed_and_the_filter_mean_layer(ctx, kind):
    _identity(*_compose(kind))


# ---- 7. train_run ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedup", [True, False], ids=["dedup", "tiled"])
def test_train_run_on_a_dilated_model_equals_the_loop_bit_for_bit(ctx, dedup):
    """``dil3_pad`` with augmentation (shift 1, flip) and a finite clip norm: five Adam steps through ``train_run`` on an attached dataset of the
    caller's 11 x 11 images against five ``train_step`` calls on host-augmented batches: ELBOs and every parameter to the bit."""
    from deepcgp_amd.augment import Augmentation
    from test_gpu_augment import _mirror_batch
    spec, _, _, _ = _case("dil3_pad")
    hwc = dr.STACKS["dil3_pad"]["hwc"]
    pool, batch, steps = 11, 4, 5
    X, _ = syn.make_batch(hwc, pool, seed=7)
    Y = np.random.default_rng(99).integers(0, 10, pool).astype(np.int32)
    idx = np.stack([np.random.default_rng(5 + i).choice(pool, batch, replace=False) for i in range(steps)])
    lrs = np.array([0.01, 0.01, 0.01, 0.001, 0.001])
    aug = Augmentation(1, True)
    models = []
    for _ in range(2):
        m = build_from_spec(copy.deepcopy(spec), X.copy(), Y.copy())
        m.dedup_layer0 = dedup
        m.set_grad_clip(50.0)
        models.append(m)
    a, b = models
    assert a._row_length() == 121
    ha = np.array([a.train_step(_mirror_batch(a.X[idx[i]], hwc, 11 + i, aug), a.Y[idx[i]], lrs[i], seed=11 + i) for i in range(steps)])
    b.attach_dataset()
    b.set_augmentation(aug)
    hb = b.train_run(idx, lrs, seed=11)
    print("loop %s\n run %s" % (ha, hb))
    assert np.all(np.isfinite(ha)) and np.array_equal(ha, hb)
    for m in (a, b):
        m.pull_parameters()
    for pa, pb in zip(a.parameters, b.parameters):
        assert pa.pathname == pb.pathname and np.array_equal(np.array(pa.value), np.array(pb.value)), pa.pathname
    before = build_from_spec(copy.deepcopy(spec), X, Y)
    moved = [pa.pathname for pa, p0 in zip(a.parameters, before.parameters) if not np.array_equal(np.array(pa.value), np.array(p0.value))]
    assert len(moved) >= len(a.parameters) - 1, moved
    b.detach_dataset()
    a.close(), b.close(), before.close()


# ---- 8. evaluation -----------------------------------------------------------------------------------------------------------------------
def test_evaluation_calls_on_a_dilated_stack(ctx):
    """7 test images in batches of 3 (a partial last batch) on ``dil3_pad``: ``evaluate``'s accuracy and log density against the RobustMax
    predictions tests/compose_ref.py computes from the torch marginals (RTOL of tests/test_gpu_evaluate.py); ``evaluate(views=)``,
    ``evaluate_uncertainty``, ``predict_y`` and ``predict_density`` run and agree with it where they state the same thing."""
    pytest.importorskip("torch")
    import compose_ref as cr
    N, S, bs, seed = 7, 2, 3, 11
    spec, _, _, _ = _case("dil3_pad")
    X, Y = syn.make_batch(dr.STACKS["dil3_pad"]["hwc"], N, seed=23)
    zs = ss.make_noise(spec, N, seed=23)
    t = tr.reference(spec, X, Y, zs)
    p, _, ld = cr.predictions(("robustmax", 10), t["means"][-1], t["vars"][-1], Y)
    model = build_from_spec(spec, X, Y)
    r = model.evaluate(X, Y, S=S, batch_size=bs, zs=zs, per_image=True)
    print("evaluate: log density %.3e  p_mean %.3e" % (rel(r["log_density"], ld[:, 0]), rel(r["p_mean"], p.mean(axis=0))))
    assert rel(r["log_density"], ld[:, 0]) < RTOL_EVAL and rel(r["p_mean"], p.mean(axis=0)) < RTOL_EVAL
    assert r["accuracy"] == np.mean(p.mean(axis=0).argmax(axis=1) == np.reshape(Y, (-1,)))
    assert abs(r["mean_log_density"] - ld.mean()) <= RTOL_EVAL * abs(ld.mean())
    py, _ = model.predict_y(X, S, zs=zs)
    assert rel(py, p) < RTOL_EVAL
    assert rel(model.predict_density(X, Y, S, zs=zs)[:, 0], ld[:, 0]) < RTOL_EVAL
    r = model.evaluate(X, Y, S=S, batch_size=bs, seed=seed, per_image=True)
    u = model.evaluate_uncertainty(X, Y, S=S, batch_size=bs, seed=seed, per_image=True)
    for key in ("accuracy", "mean_log_density", "n"):
        assert u[key] == r[key], key
    assert np.array_equal(u["log_density"], r["log_density"]) and np.all(np.isfinite(u["mutual_information"]))
    views = np.array([(0, 0, 0), (1, -1, 0), (0, 0, 1)], np.int32)      # the identity, a shift, a flip
    rv = model.evaluate(X, Y, S=S, batch_size=bs, seed=seed, views=views, per_image=True)
    assert rv["p_mean"].shape == r["p_mean"].shape and np.all(np.isfinite(rv["log_density"])) and not np.array_equal(rv["p_mean"], r["p_mean"])
    r1 = model.evaluate(X, Y, S=S, batch_size=bs, seed=seed, views=np.array([(0, 0, 0)], np.int32), per_image=True)
    assert np.array_equal(r1["p_mean"], r["p_mean"])
    model.close()


def test_layer_level_calls_split_on_the_host(ctx):
    """The layer and view objects on their own: ``extract_patches`` / ``extract_patches_PNL`` against ``unfold`` for the table's shapes;
    ``ConvLayer.conditional_ND`` and ``sample_from_conditional`` of a dilated layer (identity mean, phantoms, padding) against the torch forward's
    first layer (RTOL of tests/test_gpu_ops.py); ``full_cov=True`` refused with the dilation named, at the layer and at the model."""
    torch = pytest.importorskip("torch")
    from deepcgp_amd.models import build_layers_from_spec
    from deepcgp_amd.views import FullView
    for H, W, Cc, f, d in [(10, 10, 1, 3, 2), (9, 7, 3, 3, 2), (17, 17, 1, 3, 3), (12, 12, 2, 3, 2), (28, 28, 1, 5, 2), (11, 8, 2, 2, 3)]:
        x = np.random.default_rng(H).standard_normal((2, H, W, Cc))
        v = FullView((H, W), f, Cc, 1, dilation=d)
        want = dr.torch_patches(torch.tensor(x), f, 1, d).numpy()
        assert np.array_equal(v.extract_patches(x), want) and np.array_equal(v.extract_patches_PNL(x), want.transpose(1, 0, 2))
    for name in ("dil3_pad", "dil2_odd"):
        spec, X, Y, zs = _case(name)
        t = _torch(name)
        layer = build_layers_from_spec(spec)[0]
        m, v = layer.conditional_ND(X)
        print("%s conditional_ND: mean %.3e var %.3e" % (name, rel(m, t["means"][0][0]), rel(v, t["vars"][0][0])))
        assert rel(m, t["means"][0][0]) < RTOL_OPS and rel(v, t["vars"][0][0]) < RTOL_OPS
        S, N = spec["S"], X.shape[0]
        s, m2, v2 = layer.sample_from_conditional(np.tile(X[None], [S, 1, 1]), z=zs[0])
        assert rel(m2, t["means"][0]) < RTOL_OPS and rel(s, t["means"][0] + zs[0] * np.sqrt(t["vars"][0] + syn.JITTER)) < RTOL_OPS
        with pytest.raises(NotImplementedError, match="dilation %d" % layer.view.dilation):
            layer.conditional_ND(X, full_cov=True)
        model = build_from_spec(spec, X, Y)
        for call in (model.predict_f_full_cov, model.predict_all_layers_full_cov):
            with pytest.raises(NotImplementedError, match="dilat"):
                call(X, 2)
        model.close()


# ---- 9. two steps in flight --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dil3_pad", "ch_264_72_d2"])
def test_two_steps_in_flight_on_a_model_dilated_at_layer_0(ctx, name):
    """Two enqueued steps on different images (the split batch is per bank) against their synchronous values.  The pipelined plan may take
    another route than the synchronous one, so the bound is RTOL, the project's bound between two routes of one model."""
    spec, X, Y, zs = _case(name)
    X2, Y2 = syn.make_batch(dr.STACKS[name]["hwc"], X.shape[0], seed=19)
    zs2 = ss.make_noise(spec, X.shape[0], seed=19)
    model = build_from_spec(spec, X, Y)
    want = [model.compute_log_likelihood(X, Y, zs=zs, return_parts=True), model.compute_log_likelihood(X2, Y2, zs=zs2, return_parts=True)]
    assert want[0] != want[1]
    for _ in range(2):
        tickets = [model.enqueue_log_likelihood(X, Y, zs=zs), model.enqueue_log_likelihood(X2, Y2, zs=zs2)]
        got = [model.collect_log_likelihood(t, return_parts=True) for t in tickets]
        print("%s in flight %r\n   synchronous %r  bit-identical %s" % (name, got, want, got == want))
        for g, w in zip(got, want):
            for a, b in zip(g, w):
                assert abs(a - b) <= RTOL * max(abs(b), 1.0), (name, got, want)
    assert model.compute_log_likelihood(X, Y, zs=zs, return_parts=True) == want[0]
    model.close()


# ---- 10. a dilated last conv layer does not carry the head's rows ------------------------------------------------------------------------
def test_a_dilated_last_conv_layer_keeps_the_heads_rows_off_its_launch(ctx):
    """tests/test_gpu_head_ride.py's options on a conv layer feeding a 5 x 5 x 10 patch head: the undilated model's head rows ride the conv
    layer's launch (24 x 24 x 1 -> f5 -> 20 x 20 x 10 -> head f5); with the same head behind a dilated layer (28 x 28 x 1 -> f5 d2 -> 20 x 20 x 10)
    none does -- the sample is complete only behind the batch-to-space pass -- and the model matches torch.  ``two_dilated`` under the same
    options: no row rides either."""
    pytest.importorskip("torch")
    opts = dict(fused_shape=0, fused_persist=1, fused_wgs=3, head_ride=1000)
    k = dict(Ms=32, S=2, c=1.0, a=0.1)
    N = 3
    plain = ss.stack_spec(hwc=(24, 24, 1), convs=[(5, 1, 10, 0, 1)], head=(5, 1, 0), **k)
    spec = ss.stack_spec(hwc=(28, 28, 1), convs=[(5, 1, 10, 0, 2)], head=(5, 1, 0), **k)
    with ctx.options(**opts):
        X0, Y0 = syn.make_batch((24, 24, 1), N, seed=7)
        m0 = build_from_spec(plain, X0, Y0)
        n0 = tgp._rode(ctx)[1]
        e0 = m0.compute_log_likelihood(X0, Y0, zs=ss.make_noise(plain, N))
        rode = tgp._rode(ctx)
        print("undilated layer: %d rows rode, ELBO %.9f" % (rode[0], e0))
        assert rode[0] > 0 and rode[1] == n0 + 1, rode                    # the premise: this head rides an undilated layer
        m0.close()
        X, Y = syn.make_batch((28, 28, 1), N, seed=7)
        zs = ss.make_noise(spec, N)
        model = build_from_spec(spec, X, Y)
        got = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
        assert tgp._rode(ctx) == (0, n0 + 1), tgp._rode(ctx)              # no launch of the dilated model carried a row
        s2, X2, Y2, z2 = _case("two_dilated")
        m2 = build_from_spec(s2, X2, Y2)
        got2 = m2.compute_log_likelihood(X2, Y2, zs=z2, return_parts=True)
        assert tgp._rode(ctx) == (0, n0 + 1), tgp._rode(ctx)
        m2.close()
    want = tr.reference(spec, X, Y, zs)["parts"]
    for what, g, w in zip(("elbo", "data", "kl"), got, want):
        print("dilated layer under the ride's options %-4s device %.9f torch %.9f rel %.3e" % (what, g, w, abs(g - w) / max(abs(w), 1.0)))
        assert abs(g - w) <= RTOL * max(abs(w), 1.0), (what, g, w)
    for g, w in zip(got2, _torch("two_dilated")["parts"]):
        assert abs(g - w) <= RTOL * max(abs(w), 1.0), (got2, w)
    model.close()


# ---- 11. re-selection --------------------------------------------------------------------------------------------------------------------
def test_reselect_inducing_cuts_dilated_windows(ctx):
    """``reselect_inducing`` on ``dil2``: every new Z row of every layer is a patch of what that layer receives, as the host ``extract_patches``
    of its view cuts it -- for layer 0 a dilated window of the image, and not an undilated one."""
    spec, _, _, _ = _case("dil2")
    hwc = dr.STACKS["dil2"]["hwc"]
    X, Y = syn.make_batch(hwc, 30, seed=11)
    model = build_from_spec(copy.deepcopy(spec), X, Y)
    seed = 4
    idx = model._reselect_rng(seed, 0).choice(X.shape[0], size=20, replace=False)
    X_rows = model.X[idx]
    Fs, _, _ = model.propagate(X_rows, S=1, seed=seed)                  # the propagation reselect_inducing makes, at the parameters it has now
    report = model.reselect_inducing(images=20, seed=seed, candidates=20)
    assert [r["layer"] for r in report] == [0, 1, 2]
    views = [l.view for l in model.layers[:-1]] + [model.layers[-1].kern.view]
    for li, v in enumerate(views):
        src = X_rows if li == 0 else Fs[li - 1][0]
        img = np.asarray(src, np.float64).reshape(src.shape[0], v.input_size[0], v.input_size[1], v.feature_maps)
        windows = {row.tobytes() for row in v.extract_patches(img).reshape(-1, v.patch_length)}
        Z = np.ascontiguousarray(model.layers[li].feature.Z, np.float64)
        hits = [z.tobytes() in windows for z in Z]
        print("layer %d (dilation %d): %d of %d new inducing patches are windows of its input" % (li, v.dilation, sum(hits), len(hits)))
        assert all(hits), (li, hits)
    from deepcgp_amd.views import FullView
    v0 = views[0]
    assert v0.dilation == 2
    plain = FullView(v0.input_size, v0.filter_size, v0.feature_maps, 1)
    img = X_rows.reshape(-1, hwc[0], hwc[1], hwc[2])
    undilated = {row.tobytes() for row in plain.extract_patches(img).reshape(-1, plain.patch_length)}
    assert not all(z.tobytes() in undilated for z in np.ascontiguousarray(model.layers[0].feature.Z, np.float64))
    assert np.isfinite(model.compute_log_likelihood(X[:3], Y[:3]))
    model.close()


# ---- 12. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_with_a_message_before_anything_is_launched(ctx):
    """d < 1, a head, a strided layer, a window that does not fit, neighbours that do not take the dilated layer's true sizes -- also after a
    forward has succeeded and the padding of the layer above was changed --, a gradient step already taken, enqueued steps outstanding, a sharded
    model: DCGP_ERR_ARG and a message naming the layer.  A refused forward has launched nothing (the kernel timers of the ctx stay empty), and
    the model works afterwards."""
    L = dev.lib()

    def refused(rc, word):
        assert rc == dev.ERR_ARG, rc
        with pytest.raises(dev.DcgpError, match=word) as e:
            ctx._check(rc)
        print(e.value)

    def launches_nothing(h, n_values, word):
        ctx.timing_reset()
        ctx.timing_enable(1)
        try:
            refused(tgp._forward_rc(ctx, h, n_values), word)
            assert not ctx.timing(), ctx.timing()
        finally:
            ctx.timing_enable(0)
            ctx.timing_reset()
    # 10 x 10 x 1, f3 d2: the layer is added with its true size and gives 6 x 6 x 2, which the head takes
    conv, head = (10, 10, 1, 3, 1, 5, 2), (6, 6, 2, 3, 1, 5, 10, False)
    h = tgp._raw_model(ctx, [conv], head)
    refused(L.dcgp_model_set_dilation(h, 2, 2), "no layer 2")
    refused(L.dcgp_model_set_dilation(h, -1, 2), "no layer -1")
    refused(L.dcgp_model_set_dilation(h, 0, 0), "layer 0: the dilation must be >= 1")
    refused(L.dcgp_model_set_dilation(h, 0, -3), "layer 0: the dilation must be >= 1")
    refused(L.dcgp_model_set_dilation(h, 1, 2), "layer 1 is the head")
    refused(L.dcgp_model_set_dilation(h, 0, 5), "layer 0: a window of 3 taps 5 apart spans 11 pixels, its padded input is 10 x 10")
    ctx._check(L.dcgp_model_set_dilation(h, 0, 2))
    assert tgp._forward_rc(ctx, h, 100) == dev.DCGP_OK                          # the geometry that fits: X is [N, 10 * 10 * 1]
    ctx._check(L.dcgp_model_set_dilation(h, 0, 3))                              # f3 d3 gives 4 x 4, the head takes 6 x 6
    launches_nothing(h, 100, "dilation: layer 1 takes 6 x 6 x 2 with a padding of 0, layer 0 .dilation 3. produces 4 x 4 x 2")
    ctx._check(L.dcgp_model_set_dilation(h, 0, 2))
    ctx.timing_reset()
    ctx.timing_enable(1)
    try:
        assert tgp._forward_rc(ctx, h, 100) == dev.DCGP_OK
        assert ctx.timing(), "the timers see the launches of a step that runs"
    finally:
        ctx.timing_enable(0)
        ctx.timing_reset()
    # a sharded model, either order
    refused(L.dcgp_model_set_shard(h, 0, 4), "dilated layer")
    ctx._check(L.dcgp_model_set_dilation(h, 0, 1))
    ctx._check(L.dcgp_model_set_shard(h, 0, 4))
    refused(L.dcgp_model_set_dilation(h, 0, 2), "layer 0: a sharded model")
    ctx._check(L.dcgp_model_set_shard(h, 0, 0))
    ctx._check(L.dcgp_model_set_dilation(h, 0, 2))
    # enqueued steps outstanding
    dX, dY = ctx.to_device(np.zeros((2, 100))), ctx.to_device(np.zeros(2, np.int32), np.int32)
    ticket = C.c_uint64(0)
    ctx._check(L.dcgp_elbo_forward_enqueue(h, dX.ptr, dY.ptr, 2, 1.0, None, 0, 0, C.byref(ticket)))
    refused(L.dcgp_model_set_dilation(h, 0, 1), "enqueued steps")
    out, info = (C.c_double * 3)(), C.c_int(0)
    ctx._check(L.dcgp_elbo_forward_collect(h, ticket, out, C.byref(info)))
    assert tgp._forward_rc(ctx, h, 100) == dev.DCGP_OK                          # the model still works
    L.dcgp_model_destroy(h)
    # the padding of the layer above is changed AFTER a forward has succeeded: 10 x 10 f3 d2 gives 6 x 6, the head was added as 8 x 8 with a border of 1
    h = tgp._raw_model(ctx, [conv], (8, 8, 2, 3, 1, 5, 10, False))
    ctx._check(L.dcgp_model_set_dilation(h, 0, 2))
    ctx._check(L.dcgp_model_set_input_padding(h, 1, 1))
    assert tgp._forward_rc(ctx, h, 100) == dev.DCGP_OK
    ctx._check(L.dcgp_model_set_input_padding(h, 1, 0))                         # accepted: the head alone is consistent ...
    launches_nothing(h, 100, "dilation: layer 1 takes 8 x 8 x 2 with a padding of 0, layer 0 .dilation 2. produces 6 x 6 x 2")   # ... the chain is not
    ctx._check(L.dcgp_model_set_input_padding(h, 1, 1))
    assert tgp._forward_rc(ctx, h, 100) == dev.DCGP_OK
    L.dcgp_model_destroy(h)
    h = tgp._raw_model(ctx, [(5, 5, 1, 3, 2, 5, 2)], (2, 2, 2, 2, 1, 5, 10, False))     # a strided layer
    refused(L.dcgp_model_set_dilation(h, 0, 2), "layer 0 has stride 2")
    assert tgp._forward_rc(ctx, h, 25) == dev.DCGP_OK
    L.dcgp_model_destroy(h)
    h = tgp._raw_model(ctx, [conv], (1, 1, 72, 1, 1, 5, 10, True))              # a dense head on the dilated layer's 6 x 6 x 2 features
    ctx._check(L.dcgp_model_set_dilation(h, 0, 2))
    assert tgp._forward_rc(ctx, h, 100) == dev.DCGP_OK
    ctx._check(L.dcgp_model_set_dilation(h, 0, 3))                              # 4 x 4 x 2 = 32 features, the head takes 72
    launches_nothing(h, 100, "dilation: layer 1 takes 1 x 1 x 72")
    L.dcgp_model_destroy(h)
    # the Python surface: ValueError before a device model exists; the dilation is fixed once a gradient was taken
    from deepcgp_amd.views import FullView
    with pytest.raises(ValueError, match="stride 1"):
        FullView((10, 10), 3, 1, 2, dilation=2)
    with pytest.raises(ValueError, match="does not fit"):
        FullView((4, 4), 3, 1, 1, dilation=2)
    spec, X, Y, zs = _case("dil2")
    model = build_from_spec(spec, X, Y)
    model.compute_gradients(X, Y, zs=zs)
    refused(L.dcgp_model_set_dilation(model._model, 0, 1), "layer 0 has taken a gradient step")
    assert np.isfinite(model.compute_log_likelihood(X, Y))
    model.close()

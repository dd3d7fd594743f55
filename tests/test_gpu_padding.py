"""Zero padding on the device (``FullView(padding=p)``, ``--paddings``, dcgp_model_set_input_padding; csrc/pad.hip) against the padded CPU oracle and
torch autograd of the padded forward (tests/padding_ref.py; the two agree to 1e-9 without a GPU, tests/test_host_padding.py).

A padded layer is a VALID layer on a physically padded copy of its input, so every bound is the one the unpadded tests use for the same quantity:
RTOL of tests/test_gpu_model.py (ELBO, data term, KL, class probabilities, and two routes of one model), RTOL of tests/test_gpu_ops.py (layer
outputs), TOL_GROUP / TOL_E of tests/test_gpu_grad_m256.py (of tests/test_gpu_grad_large_m.py where a layer has M > 256), the input gradient's
1e-7 * max(1, |want|max) of tests/test_gpu_input_grad.py, the evaluation bounds of tests/test_gpu_evaluate.py / test_gpu_uncertainty.py /
test_gpu_patch_map.py, and the bit-identity of tests/test_gpu_train_run.py.  Every figure is printed before it is asserted (run with -s).
The stacks are padding_ref.STACKS; N = 3, S = 2."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.models import build_from_spec
import live_specs as ls
import padding_ref as pr
import stack_specs as ss
import test_gpu_grad_large_m as large_m
import test_gpu_grad_m256 as m256
from test_gpu_evaluate import RTOL as RTOL_EVAL, oracle_log_density
from test_gpu_model import RTOL
from test_gpu_ops import RTOL as RTOL_OPS
import torch_ref as tr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]   # a hung launch ends the run instead of holding the device

INPUT_GRAD_TOL = 1e-7      # tests/test_gpu_input_grad.py: |dX - autograd|max <= 1e-7 * max(1, |autograd|max) (written inline there)
STACKS = list(pr.STACKS)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def grad_bounds(spec):
    mod = large_m if any(l["M"] > 256 for l in spec["convs"] + [spec["head"]]) else m256
    return mod.TOL_GROUP, mod.TOL_E


@functools.lru_cache(maxsize=None)
def _case(name):
    """(spec, X, Y, zs) of a stack, once per process; never written to."""
    return pr.make_stack(name)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The padded oracle's figures of a stack, computed once: ELBO parts, every layer's sample / mean / variance, class probabilities."""
    spec, X, Y, zs = _case(name)
    ref = pr.oracle_model(spec, X, Y)
    Fs, Fm, Fv = ref.propagate(X, S=spec["S"], zs=zs)
    p, _ = ref.predict_y(X, spec["S"], zs=zs)
    return dict(parts=(ref.compute_log_likelihood(X, Y, zs=zs), ref.data_term(X, Y, zs=zs), ref.KL()), Fs=Fs, Fm=Fm, Fv=Fv, p=p)


@functools.lru_cache(maxsize=None)
def _torch(name):
    pytest.importorskip("torch")
    spec, X, Y, zs = _case(name)
    return tr.reference(spec, X, Y, zs)


# ---- 1. oracle parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedup", [False, True], ids=["tiled", "dedup"])
@pytest.mark.parametrize("name", STACKS)
def test_padded_stacks_match_the_padded_oracle(ctx, name, dedup):
    """ELBO, data term, KL, predict_y and every layer's mean, variance and sample."""
    spec, X, Y, zs = _case(name)
    o = _oracle(name)
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    got = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    for what, g, w in zip(("elbo", "data", "kl"), got, o["parts"]):
        print("%s%s %-4s device %.9f oracle %.9f rel %.3e" % (name, "-dedup" if dedup else "", what, g, w, abs(g - w) / max(abs(w), 1.0)))
    Fs, Fm, Fv = model.propagate(X, S=spec["S"], zs=zs)
    p, _ = model.predict_y(X, spec["S"], zs=zs)
    for i in range(len(Fm)):
        print("%s layer %d mean %.3e var %.3e sample %.3e" % (name, i, rel(Fm[i], o["Fm"][i]), rel(Fv[i], o["Fv"][i]), rel(Fs[i], o["Fs"][i])))
    print("%s predict_y %.3e" % (name, rel(p, o["p"])))
    e, data, kl = o["parts"]
    assert abs(got[0] - e) <= RTOL * abs(e) and abs(got[1] - data) <= RTOL * abs(data) and abs(got[2] - kl) <= RTOL * max(abs(kl), 1.0), (got, o["parts"])
    assert [m.shape[-1] for m in Fm] == [o for _, o in ss.output_dims(spec)]
    for i in range(len(Fm)):
        assert rel(Fm[i], o["Fm"][i]) < RTOL_OPS and rel(Fv[i], o["Fv"][i]) < RTOL_OPS and rel(Fs[i], o["Fs"][i]) < RTOL_OPS, (name, i)
    assert rel(p, o["p"]) < RTOL
    assert model.compute_log_likelihood(X, Y, zs=zs, return_parts=True) == got          # the other bank (and its padded buffer): the same bits
    model.close()


# ---- 2. / 3. the identities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["res3_first_only", "ch_264_72"])
def test_padding_at_layer_0_is_the_unpadded_model_on_padded_images(ctx, name):
    """A model padded only at layer 0 against the VALID model of the same parameters fed np.pad(X): ELBO parts and layer outputs within RTOL.
    On the MI355X both stacks came out bit-identical, tiled and de-duplicated: ELBO, data term, KL and every layer's mean and variance (the
    padded copy is an ordinary image to every kernel behind it); the assertion stays at RTOL, which is what the layers promise."""
    if name == "res3_first_only":
        k = dict(pr.STACKS["res3"], convs=[(3, 1, 2, 1, 1), (3, 2, 2, 0, 1)], head=(3, 1, 0))
        N = k.pop("N")
        spec = ss.stack_spec(**k)
        X, Y = syn.make_batch(k["hwc"], N, seed=7)
        zs = ss.make_noise(spec, N, seed=7)
    else:
        spec, X, Y, zs = _case(name)
    assert [l.get("pad", 0) for l in spec["convs"] + [spec["head"]]][1:] == [0] * len(spec["convs"])
    c0 = spec["convs"][0]
    Xp = pr.pad_images(X, (c0["H"], c0["W"], c0["C"]), c0["pad"])
    padded, valid = build_from_spec(spec, X, Y), build_from_spec(pr.physical(spec), Xp, Y)
    for dedup in (False, True):
        padded.dedup_layer0 = valid.dedup_layer0 = dedup
        a = padded.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
        b = valid.compute_log_likelihood(Xp, Y, zs=zs, return_parts=True)
        print("%s dedup=%d padded %r valid %r bit-identical %s" % (name, dedup, a, b, a == b))
        for g, w in zip(a, b):
            assert abs(g - w) <= RTOL * max(abs(w), 1.0), (name, dedup, a, b)
    _, Fa, Va = padded.propagate(X, S=spec["S"], zs=zs)
    _, Fb, Vb = valid.propagate(Xp, S=spec["S"], zs=zs)
    print("%s layer outputs bit-identical %s" % (name, all(np.array_equal(x, y) for x, y in zip(Fa + Va, Fb + Vb))))
    for x, y in zip(Fa + Va, Fb + Vb):
        assert rel(x, y) < RTOL
    padded.close(), valid.close()


def test_all_zero_paddings_is_the_model_without_the_flag(ctx):
    """``--paddings 0,0,0`` and no flag: the same model on the same path, the same bits (ELBO parts and a gradient step)."""
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder
    rng = np.random.default_rng(0)
    X = rng.standard_normal((40, 14, 14, 1))
    Y = rng.integers(0, 10, (40, 1))
    args = ['--name', 't', '-M', '6,7,8', '--feature-maps', '3,2', '--filter-sizes', '3,3,3', '--strides', '2,1,1', '--num-samples', '2', '--batch-size', '8']
    models = []
    for extra in ([], ['--paddings', '0,0,0']):
        np.random.seed(0)
        models.append(ModelBuilder(default_parser().parse_args(args + extra), X, Y).build())
    a, b = models
    for la, lb in zip(a.layers, b.layers):
        assert np.array_equal(la.feature.Z, lb.feature.Z)
    Xb, Yb = X[:8].reshape(8, -1), Y[:8].reshape(-1)
    zs = [np.random.default_rng(3 + i).standard_normal((2, 8, l.num_outputs)) for i, l in enumerate(a.layers)]
    ea, eb = (m.compute_log_likelihood(Xb, Yb, zs=zs, return_parts=True) for m in (a, b))
    print("no flag %r  --paddings 0,0,0 %r" % (ea, eb))
    assert ea == eb and all(np.isfinite(ea))
    (_, ga), (_, gb) = (m.compute_gradients(Xb, Yb, zs=zs) for m in (a, b))
    for da, db in zip(ga, gb):
        for k in da:
            assert np.array_equal(da[k], db[k]), k
    a.close(), b.close()


def test_model_builder_with_paddings_from_flags(ctx):
    """``--paddings 1,1,0`` through ModelBuilder (inducing patches clustered from the zero-padded images): the ELBO at explicit noise against the
    padded oracle built from the same parameters, and the reference's training loop for three steps: finite."""
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder, train
    from oracle_build import spec_from_model
    rng = np.random.default_rng(0)
    np.random.seed(0)
    X = rng.standard_normal((40, 10, 10, 1))
    Y = rng.integers(0, 10, (40, 1))
    flags = default_parser().parse_args(['--name', 't', '-M', '6,7,8', '--feature-maps', '3,2', '--filter-sizes', '3,3,3', '--strides', '1,2,1',
                                         '--paddings', '1,1,0', '--num-samples', '2', '--batch-size', '8'])
    model = ModelBuilder(flags, X, Y).build()
    views = [l.view for l in model.layers[:-1]] + [model.layers[-1].kern.view]
    assert [(v.input_size[0], v.padding, v.out_image_height) for v in views] == [(10, 1, 10), (10, 1, 5), (5, 0, 3)]
    for l in model.layers:          # (with the builder's q_mu = 0 every class has the same mean and the ELBO does not see the images)
        l.q_mu = 0.3 * rng.standard_normal(l.q_mu.shape)
    model.sync_parameters()
    spec = spec_from_model(model)
    for e, v in zip(spec["convs"] + [spec["head"]], views):
        e["pad"] = v.padding
    Xb, Yb = X[:8].reshape(8, -1), Y[:8].reshape(-1)
    zs = ss.make_noise(spec, 8, seed=3)
    e = model.compute_log_likelihood(Xb, Yb, zs=zs)
    ref = pr.oracle_model(spec, Xb, Yb).compute_log_likelihood(Xb, Yb, zs=zs)
    print("--paddings 1,1,0: ELBO %.9f oracle %.9f rel %.3e" % (e, ref, abs(e - ref) / abs(ref)))
    assert abs(e - ref) <= RTOL * abs(ref), (e, ref)
    hist = train(model, 3)
    assert len(hist) == 3 and np.all(np.isfinite(hist)), hist
    model.close()


# ---- 4. gradients -----------------------------------------------------------------------------------------------------------------------
GRAD = [(n, False) for n in STACKS] + [("res3", True), ("ch_264_72", True)]


@pytest.mark.parametrize("name,dedup", GRAD, ids=["%s%s" % (n, "-dedup" if d else "") for n, d in GRAD])
def test_gradient_matches_torch_autograd_of_the_padded_forward(ctx, name, dedup):
    """Every group of every layer, group-wise and entry-wise over the floor (tests/live_specs.py: errors); the ELBO parts against torch."""
    spec, X, Y, zs = _case(name)
    t = _torch(name)
    (e_t, data_t, kl_t), want = t["parts"], t["want"]
    ls.assert_live(name, want)
    tol_group, tol_e = grad_bounds(spec)
    tag = name + ("-dedup" if dedup else "")
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    e, grads = model.compute_gradients(X, Y, zs=zs)
    e2, grads2 = model.compute_gradients(X, Y, zs=zs)
    rows = []
    for li, groups in enumerate(want):
        assert set(groups) == set(grads[li]), (tag, li)
        for gname, w in groups.items():
            got = np.asarray(grads[li][gname], np.float64)
            assert got.shape == np.shape(w), (tag, li, gname)
            rows.append((li, gname) + ls.errors(gname, got, w))
            print("%s L%d %-14s group %.3e  entry %.3e  |want|max %.3e" % ((tag,) + rows[-1] + (np.abs(w).max(),)))
    print("%s elbo rel %.3e  WORST group %.3e entry %.3e" % (tag, abs(e - e_t) / abs(e), max(r[2] for r in rows), max(r[3] for r in rows)))
    assert abs(e - e_t) <= RTOL * abs(e), (tag, e, e_t)
    for li, gname, err_g, err_e in rows:
        assert err_g <= tol_group, (tag, li, gname, "group-wise", err_g)
        assert err_e <= tol_e, (tag, li, gname, "entry-wise", err_e)
    assert e == e2
    for a, b in zip(grads, grads2):
        for k in a:
            assert np.array_equal(a[k], b[k]), (tag, k, "repeat")
    model.close()


# ---- 5. input gradient ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedup", [False, True], ids=["tiled", "dedup"])
@pytest.mark.parametrize("objective", ["density", "elbo"])
@pytest.mark.parametrize("name", ["res3", "wide_pad"])
def test_input_gradient_is_in_the_unpadded_geometry(ctx, name, objective, dedup):
    """dX [N, H W C] of the caller's images (the crop and the replica sum of a tiled batch are one pass) against autograd through the pad."""
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
    H, W, Cc = pr.STACKS[name]["hwc"]
    sal = model.saliency(X, Y, objective=objective, zs=zs)
    assert sal.shape == (X.shape[0], H, W, Cc) and np.array_equal(sal.reshape(got.shape), got)
    model.close()


# ---- 6. two steps in flight -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["res3", "ch_264_72"])
def test_two_steps_in_flight_on_a_model_padded_at_layer_0(ctx, name):
    """Two enqueued steps on different images (the padded copy of X is per bank) against their synchronous values.  The pipelined plan may
    take another route than the synchronous one, so the bound is RTOL, the project's bound between two routes of one model."""
    spec, X, Y, zs = _case(name)
    X2, Y2 = syn.make_batch(pr.STACKS[name]["hwc"], X.shape[0], seed=19)
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


# ---- 7. a padded head does not ride -----------------------------------------------------------------------------------------------------
def _rode(ctx):
    out = (C.c_longlong * 2)()
    assert dev.lib().dcgp_debug_head_ride(ctx.handle, out) == 0
    return out[0], out[1]


def test_a_padded_head_keeps_its_rows_off_the_layer_launch(ctx):
    """tests/test_gpu_head_ride.py's shape (28 x 28 x 1, conv f5 s2 R10, head f5, M = 32, N = 3, S = 2) under its options: the unpadded model's
    head rows ride the conv layer's launch; with the head padded by 1 none does (the ride reads the unpadded sample), and the model matches the
    padded oracle."""
    opts = dict(fused_shape=0, fused_persist=1, fused_wgs=3, head_ride=1000)
    k = dict(hwc=(28, 28, 1), Ms=32, S=2, c=1.0, a=0.1)
    N = 3
    X, Y = syn.make_batch(k["hwc"], N, seed=7)
    plain = ss.stack_spec(convs=[(5, 2, 10, 0, 1)], head=(5, 1, 0), **k)
    spec = ss.stack_spec(convs=[(5, 2, 10, 0, 1)], head=(5, 1, 1), **k)
    with ctx.options(**opts):
        m0 = build_from_spec(plain, X, Y)
        n0 = _rode(ctx)[1]
        e0 = m0.compute_log_likelihood(X, Y, zs=ss.make_noise(plain, N))
        rode = _rode(ctx)
        print("unpadded head: %d rows rode, ELBO %.9f" % (rode[0], e0))
        assert rode == (N * 2, n0 + 1), rode                              # the premise: this shape rides
        m0.close()
        zs = ss.make_noise(spec, N)
        model = build_from_spec(spec, X, Y)
        got = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
        assert _rode(ctx) == (0, n0 + 1), _rode(ctx)                      # no launch of the padded model carried a row
    ref = pr.oracle_model(spec, X, Y)
    want = (ref.compute_log_likelihood(X, Y, zs=zs), ref.data_term(X, Y, zs=zs), ref.KL())
    for what, g, w in zip(("elbo", "data", "kl"), got, want):
        print("padded head %-4s device %.9f oracle %.9f rel %.3e" % (what, g, w, abs(g - w) / max(abs(w), 1.0)))
        assert abs(g - w) <= RTOL * max(abs(w), 1.0), (what, g, w)
    assert model.layers[-1].kern.patch_count == 100
    model.close()


# ---- 8. evaluation ----------------------------------------------------------------------------------------------------------------------
def test_evaluation_calls_on_a_padded_stack(ctx):
    """7 test images in batches of 3 (a partial last batch): ``evaluate`` against the padded oracle at explicit noise (RTOL of
    tests/test_gpu_evaluate.py) and against the per-batch calls it replaces (that module's bit-identity / 1e-13); ``evaluate_uncertainty``
    returns what ``evaluate`` returns, bit for bit (tests/test_gpu_uncertainty.py); ``predict_patch_contributions`` sums to ``predict_f``
    (1e-9) and matches the restatement on the oracle's padded hidden samples (1e-8), and ``as_maps`` gives the padded head's 5 x 5 maps
    (tests/test_gpu_patch_map.py)."""
    from patch_map_ref import head_patch_mean
    N, S, bs, seed = 7, 2, 3, 11
    spec, _, _, _ = _case("res3")
    hwc = pr.STACKS["res3"]["hwc"]
    X, Y = syn.make_batch(hwc, N, seed=23)
    zs = ss.make_noise(spec, N, seed=23)
    ref = pr.oracle_model(spec, X, Y)
    model = build_from_spec(spec, X, Y)
    want, om = oracle_log_density(ref, X, Y, S, zs)
    r = model.evaluate(X, Y, S=S, batch_size=bs, zs=zs, per_image=True)
    print("evaluate: log density %.3e  p_mean %.3e" % (rel(r["log_density"], want), rel(r["p_mean"], om.mean(axis=0))))
    assert rel(r["log_density"], want) < RTOL_EVAL and rel(r["p_mean"], om.mean(axis=0)) < RTOL_EVAL
    assert r["accuracy"] == np.mean(om.mean(axis=0).argmax(axis=1) == Y)
    r = model.evaluate(X, Y, S=S, batch_size=bs, seed=seed, per_image=True)
    for i, lo in enumerate(range(0, N, bs)):
        sl = slice(lo, lo + bs)
        assert np.array_equal(r["p_mean"][sl], model.predict_proba(X[sl], S, seed=seed + i))
        ld = model.predict_density(X[sl], Y[sl], S, seed=seed + i)[:, 0]
        assert np.max(np.abs(r["log_density"][sl] - ld)) <= 1e-13 * np.max(np.abs(ld))
    u = model.evaluate_uncertainty(X, Y, S=S, batch_size=bs, seed=seed, per_image=True)
    for key in ("accuracy", "mean_log_density", "n"):
        assert u[key] == r[key], key
    assert np.array_equal(u["log_density"], r["log_density"]) and np.array_equal(u["p_mean"], r["p_mean"])
    assert u["predictive_entropy"].shape == (N,) and np.all(np.isfinite(u["mutual_information"]))
    c, fm = model.predict_patch_contributions(X, S, zs=zs)
    h = spec["head"]
    assert c.shape == (S, N, 25, h["R"]) and np.array_equal(fm, model.predict_f(X, S, zs=zs)[0])
    assert np.max(np.abs(c.sum(2) - fm)) / max(np.max(np.abs(fm)), 1e-30) <= 1e-9
    Fs, _, _ = ref.propagate(X, S=S, zs=zs)
    hp = pr.physical(spec)["head"]
    wantc = np.stack([head_patch_mean(hp, pr.pad_images(Fs[-2][s_], (h["H"], h["W"], h["C"]), h["pad"]), syn.JITTER) for s_ in range(S)])
    print("patch contributions vs oracle %.3e" % rel(c, wantc))
    assert rel(c, wantc) <= 1e-8
    maps = model.layers[-1].kern.view.as_maps(c)
    assert maps.shape == (S, N, 5, 5, h["R"]) and np.array_equal(maps[:, :, 1, 2], c[:, :, 7])
    model.close()


def test_operator_level_calls_pad_on_the_host(ctx):
    """The layer and kernel objects on their own (no device model): a padded view on X against the VALID view of the padded size on np.pad(X) --
    the same device call on the same values, so equal to the bit -- for ``ConvLayer.conditional_ND`` (the one-call route with the identity
    mean's centre pixel, the composed route of a Matern base kernel, full_cov), ``ConvKernel.Kzx / Kdiag / K / patch_mean`` and the head's
    ``conditional_ND`` / ``patch_contributions``; and the padded conv layer against the padded oracle's (RTOL of tests/test_gpu_ops.py)."""
    from deepcgp_amd.models import build_layers_from_spec
    spec, X, Y, zs = _case("res3")
    phys = pr.physical(spec)
    c0, h = spec["convs"][0], spec["head"]
    Xp = pr.pad_images(X, (c0["H"], c0["W"], c0["C"]), c0["pad"])
    for base in ("rbf", "matern32"):
        a, b = copy.deepcopy(spec), copy.deepcopy(phys)
        a["convs"][0]["base"] = b["convs"][0]["base"] = base
        conv, vconv = build_layers_from_spec(a)[0], build_layers_from_spec(b)[0]
        assert conv.identity_mean and conv.view.padding == 1 and vconv.view.padding == 0 and conv.num_outputs == vconv.num_outputs == 200
        for full_cov in (False, True):
            got, want = conv.conditional_ND(X, full_cov=full_cov), vconv.conditional_ND(Xp, full_cov=full_cov)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (base, full_cov)
        assert np.array_equal(conv.view.extract_patches(X.reshape(-1, 10, 10, 1)), vconv.view.extract_patches(Xp.reshape(-1, 12, 12, 1)))
        if base == "rbf":
            om, ov = pr.oracle_model(spec, X, Y).layers[0].conditional_ND(X)
            m, v = conv.conditional_ND(X)
            print("padded conv layer vs the padded oracle: mean %.3e var %.3e" % (rel(m, om), rel(v, ov)))
            assert rel(m, om) < RTOL_OPS and rel(v, ov) < RTOL_OPS
    head, vhead = build_layers_from_spec(spec)[-1], build_layers_from_spec(phys)[-1]
    F = np.random.default_rng(3).standard_normal((4, h["H"] * h["W"] * h["C"]))
    Fp = pr.pad_images(F, (h["H"], h["W"], h["C"]), h["pad"])
    k, vk, Z = head.kern, vhead.kern, head.feature.Z
    beta = np.random.default_rng(4).standard_normal((h["M"], 3))
    assert k.patch_count == vk.patch_count == 25
    assert np.array_equal(k.Kzx(Z, F), vk.Kzx(Z, Fp)) and np.array_equal(k.Kdiag(F), vk.Kdiag(Fp))
    assert np.array_equal(k.K(F), vk.K(Fp)) and np.array_equal(k.K(F, F[:2]), vk.K(Fp, Fp[:2]))
    assert np.array_equal(k.patch_mean(Z, F, beta), vk.patch_mean(Z, Fp, beta))
    for got, want in zip(head.conditional_ND(F), vhead.conditional_ND(Fp)):
        assert np.array_equal(got, want)
    for got, want in zip(head.conditional_ND(F, full_cov=True), vhead.conditional_ND(Fp, full_cov=True)):
        assert np.array_equal(got, want)
    assert np.array_equal(head.patch_contributions(F), vhead.patch_contributions(Fp))


# ---- 9. train_run -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedup", [True, False], ids=["dedup", "tiled"])
def test_train_run_on_a_padded_model_equals_the_loop_bit_for_bit(ctx, dedup):
    """An UNPADDED dataset attached to a padded model (rows of 100 values; the device pads each gathered batch): five Adam steps through
    ``train_run`` against five ``train_step`` calls, ELBOs and every parameter to the bit (tests/test_gpu_train_run.py)."""
    spec, _, _, _ = _case("res3")
    pool, batch, steps = 11, 4, 5
    X, _ = syn.make_batch(pr.STACKS["res3"]["hwc"], pool, seed=7)
    Y = np.random.default_rng(99).integers(0, 10, pool).astype(np.int32)
    idx = np.stack([np.random.default_rng(5 + i).choice(pool, batch, replace=False) for i in range(steps)])
    lrs = np.array([0.01, 0.01, 0.01, 0.001, 0.001])
    models = []
    for _ in range(2):
        m = build_from_spec(copy.deepcopy(spec), X.copy(), Y.copy())
        m.dedup_layer0 = dedup
        models.append(m)
    a, b = models
    assert a._row_length() == 100
    ha = np.array([a.train_step(a.X[idx[i]], a.Y[idx[i]], lrs[i], seed=11 + i) for i in range(steps)])
    b.attach_dataset()
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
    a.close(), b.close()


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------------------
def _raw_model(ctx, layers, head):
    """A device model through the C entry points alone: layers [(H, W, C, f, s, M, R)], head (H, W, C, f, s, M, R, ard)."""
    L = dev.lib()
    h = C.c_void_p()
    ctx._check(L.dcgp_model_create(ctx.handle, 2, 1e-3, C.byref(h)))
    rng = np.random.default_rng(0)
    for (H, W, Cc, f, s, M, R) in layers:
        Z, q_mu, q_sqrt = rng.standard_normal((M, f * f * Cc)), rng.standard_normal((M, R)), np.tile(np.eye(M)[None], [R, 1, 1])
        ctx._check(L.dcgp_model_add_conv_layer(h, H, W, Cc, f, s, M, R, 0, 0, 1.0, 2.0, Z.ctypes.data, None, q_mu.ctypes.data, q_sqrt.ctypes.data))
    H, W, Cc, f, s, M, R, ard = head
    Z, w = rng.standard_normal((M, f * f * Cc)), np.ones(((H - f) // s + 1) * ((W - f) // s + 1))
    q_mu, q_sqrt = rng.standard_normal((M, R)), np.tile(np.eye(M)[None], [R, 1, 1])
    ctx._check(L.dcgp_model_set_head(h, H, W, Cc, f, s, M, R, 0, 0, 1.0, 2.0, Z.ctypes.data, w.ctypes.data, q_mu.ctypes.data, q_sqrt.ctypes.data))
    if ard:
        lsc = np.full(f * f * Cc, 2.0)
        ctx._check(L.dcgp_model_set_param(h, len(layers), b"ard_lengthscales", lsc.ctypes.data, lsc.size))
    return h


def _forward_rc(ctx, h, n_values, N=2):
    L = dev.lib()
    dX, dY = ctx.to_device(np.zeros((N, n_values))), ctx.to_device(np.zeros(N, np.int32), np.int32)
    out, info = (C.c_double * 3)(), C.c_int(0)
    return L.dcgp_elbo_forward(h, dX.ptr, dY.ptr, N, 1.0, None, 0, 0, out, C.byref(info))


def test_refusals_come_with_a_message_before_anything_is_launched(ctx):
    """A geometry mismatch between layers, padding on a dense head, a negative pad, a bad layer index: DCGP_ERR_ARG and a message.  A refused
    forward has launched nothing: the kernel timers of the ctx stay empty."""
    L = dev.lib()

    def refused(rc, word):
        assert rc == dev.ERR_ARG, rc
        with pytest.raises(dev.DcgpError, match=word) as e:
            ctx._check(rc)
        print(e.value)
    conv, head = (10, 10, 1, 3, 1, 5, 2), (10, 10, 2, 3, 1, 5, 10, False)       # 8 x 8 x 2 + a border of 1 = 10 x 10 x 2
    h = _raw_model(ctx, [conv], head)
    refused(L.dcgp_model_set_input_padding(h, 2, 1), "no layer 2")
    refused(L.dcgp_model_set_input_padding(h, -1, 1), "no layer -1")
    refused(L.dcgp_model_set_input_padding(h, 1, -1), "must be >= 0")
    ctx._check(L.dcgp_model_set_input_padding(h, 1, 1))
    assert _forward_rc(ctx, h, 100) == dev.DCGP_OK                              # the geometry that fits
    ctx._check(L.dcgp_model_set_input_padding(h, 1, 2))                         # 8 + 4 != 10
    ctx.timing_reset()
    ctx.timing_enable(1)
    try:
        refused(_forward_rc(ctx, h, 100), "layer 1 takes 10 x 10 x 2, layer 0 produces 8 x 8 x 2")
        assert not ctx.timing(), ctx.timing()
        ctx._check(L.dcgp_model_set_input_padding(h, 1, 1))
        assert _forward_rc(ctx, h, 100) == dev.DCGP_OK
        assert ctx.timing(), "the timers see the launches of a step that runs"
    finally:
        ctx.timing_enable(0)
        ctx.timing_reset()
    refused(L.dcgp_model_set_input_padding(h, 0, 5), "smaller than its border")   # layer 0 was added as 10 x 10: no image inside a border of 5
    assert _forward_rc(ctx, h, 100) == dev.DCGP_OK                              # (a refused setting changes nothing)
    L.dcgp_model_destroy(h)
    h = _raw_model(ctx, [(10, 10, 1, 3, 1, 5, 2)], (10, 10, 3, 3, 1, 5, 10, False))   # channels: layer 0 makes 2 maps, the head takes 3
    ctx._check(L.dcgp_model_set_input_padding(h, 1, 1))
    refused(_forward_rc(ctx, h, 100), "layer 1 takes")
    L.dcgp_model_destroy(h)
    h = _raw_model(ctx, [(10, 10, 1, 3, 1, 5, 2)], (1, 1, 128, 1, 1, 5, 10, True))    # the dense head on the 8 x 8 x 2 features: 1 x 1 holds no border
    assert _forward_rc(ctx, h, 100) == dev.DCGP_OK
    refused(L.dcgp_model_set_input_padding(h, 1, 1), "smaller than its border")
    L.dcgp_model_destroy(h)
    h = _raw_model(ctx, [(10, 10, 1, 3, 1, 5, 2)], (3, 3, 2, 3, 1, 5, 10, True))      # a single-patch head with per-dimension lengthscales, large enough
    ctx._check(L.dcgp_model_set_input_padding(h, 1, 1))
    refused(_forward_rc(ctx, h, 100), "dense head")
    L.dcgp_model_destroy(h)
    # the Python surface: ValueError naming the flag, before a device model exists
    spec, X, Y, _ = _case("wide_pad")
    bad = copy.deepcopy(spec)
    bad["head"].update(kernel="rbf", pad=1)
    with pytest.raises(ValueError, match="--paddings"):
        build_from_spec(bad, X, Y)

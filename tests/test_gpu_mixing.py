"""Mixed conv layers on the device (``ConvLayer(..., mixing=W)``, dcgp_model_set_mixing; csrc/mix.hip) against tests/mixing_ref.py: the NumPy
mirror of the three kernels (operator entries, ``==`` on small-integer operands) and torch autograd of the sample-then-mix forward with W a
leaf (ELBO parts, the layers' marginals, every gradient group, the input gradient).  tests/test_host_mixing.py shows without a GPU that every
case here is live.

A mixing is three more sums per column, so every bound is the one the tests without it use for the same quantity, imported: RTOL of
tests/test_gpu_model.py (ELBO, data term, KL), RTOL of tests/test_gpu_ops.py (layer outputs), TOL_GROUP / TOL_E of tests/test_gpu_grad_m256.py
(of tests/test_gpu_grad_large_m.py for ``m264``), the input gradient's 1e-7 * max(1, |want|max), RTOL of tests/test_gpu_evaluate.py, the norm's
bound of tests/test_gpu_grad_clip.py and the bit-identity of tests/test_gpu_train_run.py.  Every figure is printed before it is asserted (-s)."""
import copy
import functools

import numpy as np
import pytest

from deepcgp_amd import augment
from deepcgp_amd import device as dev
from deepcgp_amd import synthetic as syn
from deepcgp_amd.layers import mixing_matrix
from deepcgp_amd.models import build_from_spec
import compose_ref
import live_specs as ls
import mixing_ref as R
import stack_specs as ss
import test_gpu_grad_clip as clip
import test_gpu_grad_large_m as large_m
import test_gpu_grad_m256 as m256
from test_gpu_evaluate import RTOL as RTOL_EVAL
from test_gpu_model import RTOL
from test_gpu_ops import RTOL as RTOL_OPS
import torch_ref as tr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]   # a hung launch ends the run instead of holding the device

INPUT_GRAD_TOL = 1e-7      # tests/test_gpu_input_grad.py: |dX - autograd|max <= 1e-7 * max(1, |autograd|max)
CASES = [(name, None) for name in R.CASES] + [(name, base) for name, bases in R.BASES.items() for base in bases]
DEDUP = [False, True]


def _id(case):
    return case[0] + ("" if case[1] is None else "-" + case[1])


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def grad_bounds(spec):
    mod = large_m if any(l["M"] > 256 for l in spec["convs"] + [spec["head"]]) else m256
    return mod.TOL_GROUP, mod.TOL_E


@functools.lru_cache(maxsize=None)
def _case(name, base=None):
    """(spec, X, Y, zs), once per process; never written to."""
    return R.make_case(name, base=base)


@functools.lru_cache(maxsize=None)
def _ref(name, base=None):
    """ONE torch forward per case: ELBO parts, every gradient group, the layers' samples and marginals, the head's marginals, J and dX."""
    import torch
    spec, X, Y, zs = _case(name, base)
    out = tr.forward(spec, X, Y, zs, x_leaf=True)
    want, _ = tr.gradients(out)
    (dX,) = torch.autograd.grad(out["data"].sum(), out["X"])
    S, N = spec["S"], X.shape[0]
    n = lambda ts: [t.detach().numpy().reshape(S, N, -1) for t in ts]      # noqa: E731
    return dict(parts=(out["elbo"].item(), out["data"].sum().item(), out["kl"].item()), want=want, Fs=n(out["F"]), Fm=n(out["Fmeans"]),
                Fv=n(out["Fvars"]), head=(out["mean"].detach().numpy(), out["var"].detach().numpy()), J=out["data"].detach().numpy(), dX=dX.numpy())


# ---- 1. the operator entries against the NumPy mirror ------------------------------------------------------------------------------------------
def _ints(rng, shape, lo=-4, hi=5):
    return rng.integers(lo, hi, shape).astype(np.float64)


def _mix_forward(ctx, W, u, gm, gv, col0, Kc, rep, lat_stride, out_stride, n_out, outputs=(True, True, True)):
    """dcgp_mix_forward on NaN-filled outputs of n_out doubles (an unwritten element shows): (sample, mean, var) flat, None where not asked for."""
    G, Rm = W.shape
    dW, ins = ctx.to_device(W), [ctx.to_device(a) for a in (u, gm, gv)]
    outs = [ctx.to_device(np.full(n_out, np.nan)) if on else None for on in outputs]
    ctx._check(dev.lib().dcgp_mix_forward(ctx.handle, dW.ptr, G, Rm, *[a.ptr if on else None for a, on in zip(ins, outputs)], col0, Kc, rep,
                                          lat_stride, out_stride, *[o.ptr if o else None for o in outs]))
    return [o.numpy() if o else None for o in outs]


@pytest.mark.parametrize("K,G,Rm", [(216, 3, 5), (525, 4, 2), (525, 1, 3), (216, 3, 3), (1, 2, 2), (2100, 3, 10), (70, 20, 17)])
def test_operator_entries_equal_the_mirror(ctx, K, G, Rm):
    """Small-integer operands: every product and sum is exact, the device result must EQUAL the mirror.  rep = 1 and 3 (the replica layout of a
    de-duplicated first layer), a chunked call (col0 > 0: the columns before it stay untouched), null mean / var, and gW twice: the same bits."""
    rng = np.random.default_rng(K + 7 * G + Rm)
    W = _ints(rng, (G, Rm), -3, 4)
    for rep in (1, 3):
        u, gm, gv = _ints(rng, (rep, K, G)), _ints(rng, (rep, K, G)), _ints(rng, (rep, K, G), 0, 6)
        want = [np.stack([w for w in ws]) for ws in zip(*[R.mirror_forward(W, u[s], gm[s], gv[s]) for s in range(rep)])]
        got = _mix_forward(ctx, W, u, gm, gv, 0, K, rep, K * G, K * Rm, rep * K * Rm)
        for name, g, w in zip(("sample", "mean", "var"), got, want):
            assert np.array_equal(g.reshape(rep, K, Rm), w), (name, rep)
        col0 = K // 3                                            # a chunk: columns col0 .. K - 1 of every replica
        got = _mix_forward(ctx, W, u, gm, gv, col0, K - col0, rep, K * G, K * Rm, rep * K * Rm, outputs=(True, False, False))
        assert got[1] is None and got[2] is None
        g = got[0].reshape(rep, K, Rm)
        assert np.array_equal(g[:, col0:], want[0][:, col0:]) and np.isnan(g[:, :col0]).all()
        got = _mix_forward(ctx, W, u, gm, gv, 0, K, rep, K * G, K * Rm, rep * K * Rm, outputs=(False, True, True))
        assert got[0] is None and np.array_equal(got[1].reshape(rep, K, Rm), want[1]) and np.array_equal(got[2].reshape(rep, K, Rm), want[2])
    u, gF = _ints(rng, (K, G)), _ints(rng, (K, Rm))
    dW, du, dg = ctx.to_device(W), ctx.to_device(u), ctx.to_device(gF)
    res = []
    for _ in range(2):
        gu, gW = ctx.to_device(np.full((K, G), np.nan)), ctx.to_device(np.full((G, Rm), np.nan))
        ctx._check(dev.lib().dcgp_mix_backward(ctx.handle, dW.ptr, G, Rm, du.ptr, dg.ptr, K, gu.ptr, gW.ptr))
        res.append((gu.numpy(), gW.numpy()))
    assert np.array_equal(res[0][0], R.mirror_backward_latent(W, gF))
    assert np.array_equal(res[0][1], R.mirror_backward_w(u, gF))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def test_gw_has_a_fixed_order_on_real_operands(ctx):
    """Operands that do round: two runs give the same bits, and they are the mirror's (its partial sums in the kernels' order) to 4 ulp of the
    sum of magnitudes (the device's FMAs round once where the mirror rounds twice)."""
    rng = np.random.default_rng(3)
    K, G, Rm = 525, 3, 5
    W, u, gF = rng.standard_normal((G, Rm)), rng.standard_normal((K, G)), rng.standard_normal((K, Rm))
    dW, du, dg = ctx.to_device(W), ctx.to_device(u), ctx.to_device(gF)
    res = []
    for _ in range(2):
        gW = ctx.to_device(np.full((G, Rm), np.nan))
        ctx._check(dev.lib().dcgp_mix_backward(ctx.handle, dW.ptr, G, Rm, du.ptr, dg.ptr, K, None, gW.ptr))
        res.append(gW.numpy())
    want = R.mirror_backward_w(u, gF)
    err = np.abs(res[0] - want).max()
    bound = K * 2.0 ** -52 * (np.abs(u).T @ np.abs(gF)).max()
    print("gW: |device - mirror| %.3e  bound %.3e" % (err, bound))
    assert np.array_equal(res[0], res[1]) and err <= bound


def test_operator_refusals(ctx):
    L = dev.lib()
    a = ctx.to_device(np.zeros(64 * 65))
    for G, Rm, word in ((0, 2, "G = 0"), (65, 2, "G = 65"), (2, 65, "R = 65"), (2, 0, "R = 0")):
        rc = L.dcgp_mix_forward(ctx.handle, a.ptr, G, Rm, a.ptr, a.ptr, a.ptr, 0, 1, 1, 0, 0, a.ptr, a.ptr, a.ptr)
        assert rc == dev.ERR_ARG
        with pytest.raises(dev.DcgpError, match=word):
            ctx._check(rc)


# ---- 2. W = I and a permutation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedup", DEDUP, ids=["tiled", "dedup"])
@pytest.mark.parametrize("name", ["a_3_3", "b_3_3", "pad_lin"])
def test_identity_and_permutation_are_the_unmixed_layer_bit_for_bit(ctx, name, dedup):
    spec, X, Y, zs = _case(name)
    G = spec["convs"][0]["R"]
    if name == "pad_lin":      # a trained LinearConv2dMean on top: G = R = 5 for the comparison
        spec, X, Y, zs = R.make_case(name, G=5)
        G = 5
    plain = copy.deepcopy(spec)
    del plain["convs"][0]["mix_W"]
    S = spec["S"]
    res = {}
    perm = np.roll(np.arange(G), 1)
    for tag, s in (("plain", plain), ("eye", R.with_mixing(spec, [np.eye(G)])), ("perm", R.with_mixing(spec, [np.eye(G)[:, perm]]))):
        if tag == "perm" and s["convs"][0].get("mean_filter") is not None:      # the filter's columns follow the maps
            s["convs"][0]["mean_filter"] = np.asarray(s["convs"][0]["mean_filter"])[..., perm]
        m = build_from_spec(s, X, Y)
        m.dedup_layer0 = dedup
        res[tag] = (m.predict_all_layers(X, S, zs=zs), m.compute_log_likelihood(X, Y, zs=zs, return_parts=True))
        m.close()
    P = res["plain"][0][0][0].shape[2] // G
    for k, what in enumerate(("Fs", "Fmeans", "Fvars")):
        a, b, c = (res[t][0][k][0] for t in ("plain", "eye", "perm"))
        assert np.array_equal(a, b), (name, what, "identity")
        assert np.array_equal(a.reshape(S, -1, P, G)[..., perm], c.reshape(S, -1, P, G)), (name, what, "permutation")
    for g, w in zip(res["eye"][1], res["plain"][1]):      # (launch placement differs: the head no longer rides)
        print("%s dedup=%d: mixed by I %.12g unmixed %.12g" % (name, dedup, g, w))
        assert abs(g - w) <= RTOL * max(abs(w), 1.0)


# ---- 3. ELBO, data term, KL and the layers' marginals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedup", DEDUP, ids=["tiled", "dedup"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_stacks_match_the_torch_forward(ctx, case, dedup):
    spec, X, Y, zs = _case(*case)
    o = _ref(*case)
    tag = _id(case) + ("-dedup" if dedup else "")
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    got = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    for what, g, w in zip(("elbo", "data", "kl"), got, o["parts"]):
        print("%s %-4s device %.9f reference %.9f rel %.3e" % (tag, what, g, w, abs(g - w) / max(abs(w), 1.0)))
    Fs, Fm, Fv = model.predict_all_layers(X, spec["S"], zs=zs)
    rows = []
    for i in range(len(Fm) - 1):
        assert Fs[i].shape == o["Fs"][i].shape == (spec["S"], X.shape[0], model.layers[i].num_outputs)
        rows += [("layer %d sample" % i, rel(Fs[i], o["Fs"][i])), ("layer %d mean" % i, rel(Fm[i], o["Fm"][i])), ("layer %d var" % i, rel(Fv[i], o["Fv"][i]))]
    rows += [("head mean", rel(Fm[-1], o["head"][0])), ("head var", rel(Fv[-1], o["head"][1]))]
    for what, err in rows:
        print("%s %-16s %.3e" % (tag, what, err))
    e, data, kl = o["parts"]
    assert abs(got[0] - e) <= RTOL * abs(e) and abs(got[1] - data) <= RTOL * abs(data) and abs(got[2] - kl) <= RTOL * max(abs(kl), 1.0), (got, o["parts"])
    for what, err in rows:
        assert err < RTOL_OPS, (tag, what, err)
    assert model.compute_log_likelihood(X, Y, zs=zs, return_parts=True) == got
    # the layer-level calls: conditional_ND's marginals and the sample through the operator entry
    li = [i for i, c in enumerate(spec["convs"]) if c.get("mix_W") is not None][0]
    if li == 0:
        l0 = model.layers[0]
        mean, var = l0.conditional_ND(X)
        smp, _, _ = l0.sample_from_conditional(np.tile(X[None], [spec["S"], 1, 1]), z=zs[0])
        print("%s layer-level mean %.3e var %.3e sample %.3e" % (tag, rel(mean, o["Fm"][0][0]), rel(var, o["Fv"][0][0]), rel(smp, o["Fs"][0])))
        assert rel(mean, o["Fm"][0][0]) < RTOL_OPS and rel(var, o["Fv"][0][0]) < RTOL_OPS and rel(smp, o["Fs"][0]) < RTOL_OPS
    model.close()


# ---- 4. gradients ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dedup", DEDUP, ids=["tiled", "dedup"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gradient_of_every_group_including_the_mixing(ctx, case, dedup):
    spec, X, Y, zs = _case(*case)
    o = _ref(*case)
    want = o["want"]
    tol_group, tol_e = grad_bounds(spec)
    tag = _id(case) + ("-dedup" if dedup else "")
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    e, grads = model.compute_gradients(X, Y, zs=zs)
    e2, grads2 = model.compute_gradients(X, Y, zs=zs)
    rows = []
    for li, groups in enumerate(want):
        assert set(groups) == set(grads[li]), (tag, li, sorted(groups), sorted(grads[li]))
        for gname, w in groups.items():
            got = np.asarray(grads[li][gname], np.float64)
            assert got.shape == np.shape(w), (tag, li, gname, got.shape, np.shape(w))
            rows.append((li, gname) + ls.errors(gname, got, w))
            print("%s L%d %-16s group %.3e  entry %.3e  |want|max %.3e" % ((tag,) + rows[-1] + (np.abs(w).max(),)))
    print("%s elbo rel %.3e  WORST group %.3e entry %.3e" % (tag, abs(e - o["parts"][0]) / abs(e), max(r[2] for r in rows), max(r[3] for r in rows)))
    assert any("mixing" in g for g in grads[:-1])
    assert abs(e - o["parts"][0]) <= RTOL * abs(e), (tag, e, o["parts"][0])
    for li, gname, err_g, err_e in rows:
        assert err_g <= tol_group, (tag, li, gname, "group-wise", err_g)
        assert err_e <= tol_e, (tag, li, gname, "entry-wise", err_e)
    assert e == e2
    for a, b in zip(grads, grads2):
        for k in a:
            assert np.array_equal(a[k], b[k]), (tag, k, "repeat")
    model.close()


@pytest.mark.parametrize("dedup", DEDUP, ids=["tiled", "dedup"])
@pytest.mark.parametrize("name", ["a_3_5", "b_4_2", "deep", "pad_lin"])
def test_input_gradient_both_objectives(ctx, name, dedup):
    spec, X, Y, zs = _case(name)
    o = _ref(name)
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    J, got = model.input_gradient(X, Y, objective="elbo", zs=zs)
    err = np.abs(got - o["dX"]).max()
    print("%s dedup=%d elbo: |dX - autograd| %.3e  |want|max %.3e  J rel %.3e" % (name, dedup, err, np.abs(o["dX"]).max(), rel(J, o["J"])))
    assert got.shape == X.shape and rel(J, o["J"]) <= RTOL and err <= INPUT_GRAD_TOL * max(1.0, np.abs(o["dX"]).max())
    Jw, want = tr.input_gradient(spec, X, Y, zs, tr.robustmax_density(Y))
    J, got = model.input_gradient(X, Y, objective="density", zs=zs)
    err = np.abs(got - want).max()
    print("%s dedup=%d density: |dX - autograd| %.3e  |want|max %.3e  J rel %.3e" % (name, dedup, err, np.abs(want).max(), rel(J, Jw)))
    assert rel(J, Jw) <= RTOL and err <= INPUT_GRAD_TOL * max(1.0, np.abs(want).max())
    s = model.saliency(X, Y, objective="elbo", zs=zs)
    assert np.all(np.isfinite(s)) and s.shape[0] == X.shape[0]
    model.close()


# ---- 5. training -------------------------------------------------------------------------------------------------------------------------------
def _values(model):
    model.pull_parameters()
    return [(p.pathname, np.array(p.value)) for p in model.parameters]


def _train_models(name, dedup, n=2, pool=11):
    spec, _, _, _ = _case(name)
    X, _ = syn.make_batch(R.CASES[name]["hwc"], pool, seed=7)
    Y = np.random.default_rng(99).integers(0, 10, pool).astype(np.int32)
    models = []
    for _ in range(n):
        m = build_from_spec(copy.deepcopy(spec), X.copy(), Y.copy())
        m.dedup_layer0 = dedup
        models.append(m)
    return spec, X, Y, models


@pytest.mark.parametrize("name,dedup", [("pad_lin", True), ("deep", False)])
def test_train_run_equals_the_loop_bit_for_bit(ctx, name, dedup):
    """Six Adam steps with augmentation and a finite clip norm: ``train_run`` against six ``train_step`` calls on mirror-augmented batches --
    ELBOs, norms and every parameter, W among them, to the bit; W has moved."""
    from test_gpu_augment import _mirror_batch
    batch, steps, seed0 = 4, 6, 11
    aug = augment.Augmentation(1, True)
    spec, X, Y, (a, b) = _train_models(name, dedup)
    hwc = R.CASES[name]["hwc"]
    idx = np.stack([np.random.default_rng(5 + i).choice(len(X), batch, replace=False) for i in range(steps)])
    lrs = np.array([0.01, 0.01, 0.01, 0.001, 0.001, 0.001])
    li = [i for i, c in enumerate(spec["convs"]) if c.get("mix_W") is not None][0]
    key = "DGP/layers/%d/mixing/W" % li
    start = dict(_values(a))
    probe = build_from_spec(copy.deepcopy(spec), X.copy(), Y.copy())      # the first step's norm, to put the clip at half of it
    probe.dedup_layer0 = dedup
    probe.set_grad_clip(np.inf)
    probe.train_step(_mirror_batch(probe.X[idx[0]], hwc, seed0, aug), probe.Y[idx[0]], lrs[0], seed=seed0)
    max_norm = 0.5 * probe.last_grad_norms[0]
    probe.close()
    ha, na = [], []
    a.set_grad_clip(max_norm), b.set_grad_clip(max_norm)
    for i in range(steps):
        ha.append(a.train_step(_mirror_batch(a.X[idx[i]], hwc, seed0 + i, aug), a.Y[idx[i]], lrs[i], seed=seed0 + i))
        na.extend(a.last_grad_norms)
    b.attach_dataset()
    b.set_augmentation(aug)
    hb = b.train_run(idx, lrs, seed=seed0)
    print("loop %s\n run %s\nnorms %s (clip at %.6g)" % (np.array(ha), hb, na, max_norm))
    assert np.all(np.isfinite(ha)) and np.array_equal(np.array(ha), hb) and np.array_equal(np.array(na), b.last_grad_norms)
    assert na[0] > max_norm                                   # the clip is active
    va, vb = _values(a), _values(b)
    assert [n for n, _ in va] == [n for n, _ in vb] and key in dict(va)
    for (pname, x), (_, y) in zip(va, vb):
        assert np.array_equal(x, y), pname
    moved = np.abs(dict(va)[key] - start[key]).max()
    print("%s moved by %.3e" % (key, moved))
    assert moved > 1e-4
    b.detach_dataset()
    a.close(), b.close()


@pytest.mark.parametrize("name", ["a_3_5", "pad_lin"])
def test_reported_norm_includes_the_mixing(ctx, name):
    """last_grad_norms[0] against the norm formed on the host from compute_gradients' gradients (tests/test_gpu_grad_clip.py's _g_u, plus the
    unconstrained groups ``mixing`` and ``mean_filter``), within that test's bound; without W's share the host norm misses it."""
    spec, X, Y, zs = _case(name)
    model = build_from_spec(copy.deepcopy(spec), X, Y)
    model.set_grad_clip(np.inf)
    _, g = model.compute_gradients(X, Y, zs=zs)
    model.adam_step(0.01)
    got = model.last_grad_norms
    gu, n = clip._g_u(model, g)
    without = clip._norm(gu)
    for li, gl in enumerate(g):
        for k in ("mixing", "mean_filter"):
            if k in gl:
                gu["layers/%d/%s" % (li, k)] = gl[k]
                n += gl[k].size
    want, bound = clip._norm(gu), 8 * n * 2.0 ** -53
    print("%s: device %.17g numpy %.17g rel %.3e bound %.3e; without the new groups %.17g" % (name, got[0], want, abs(got[0] - want) / want, bound, without))
    assert got.shape == (1,) and abs(got[0] - want) <= bound * want and abs(got[0] - without) > bound * want
    model.close()


def test_a_frozen_mixing_stays_put_and_everything_else_moves(ctx):
    spec, X, Y, (a,) = _train_models("pad_lin", True, n=1)
    a.set_trainable(0, "mixing", False)
    assert a.layers[0].mixing_trainable is False
    start = dict(_values(a))
    zs = ss.make_noise(spec, 4, seed=3)
    for _ in range(3):
        a.train_step(X[:4], Y[:4], 0.01, zs=zs)
    now = dict(_values(a))
    key = "DGP/layers/0/mixing/W"
    assert np.array_equal(now[key], start[key])
    for k in start:
        if k != key and "likelihood" not in k:
            assert not np.array_equal(now[k], start[k]), k
    _, grads = a.compute_gradients(X[:4], Y[:4], zs=zs)
    assert not grads[0]["mixing"].any()                        # frozen: the gradient is not formed
    a.set_trainable(0, "mixing", True)
    a.train_step(X[:4], Y[:4], 0.01, zs=zs)
    assert not np.array_equal(dict(_values(a))[key], start[key])
    with pytest.raises(ValueError, match="not mixed"):
        a.set_trainable(1, "mixing", True)
    a.close()
    frozen = copy.deepcopy(spec)
    frozen["convs"][0]["mix_trainable"] = False              # the spec's flag reaches the device
    b = build_from_spec(frozen, X, Y)
    b.train_step(X[:4], Y[:4], 0.01, zs=zs)
    assert np.array_equal(dict(_values(b))[key], start[key])
    b.close()


def test_sgd_and_natgrad_steps(ctx):
    """One step of each against the host replay on the torch gradients.  SGD (tests/test_gpu_matern.py's bounds: the step moves W by >= 1e-5
    relative, the result is the replay's to 1e-9): W is unconstrained, W + lr gW; the other groups are the groups of the same step with W frozen,
    to the bit.  NatGrad: (q_mu, q_sqrt) of every layer against tests/natgrad_ref.py at 1e-8 (tests/test_gpu_matern.py), W untouched -- it
    belongs to the Adam part, whose first step then moves it by lr * sign(gW)."""
    from natgrad_ref import natgrad_reference
    spec, X, Y, zs = _case("a_3_5")
    want = _ref("a_3_5")["want"]
    lr = 1e-7
    a, b = build_from_spec(copy.deepcopy(spec), X, Y), build_from_spec(copy.deepcopy(spec), X, Y)
    b.set_trainable(0, "mixing", False)
    a.compute_gradients(X, Y, zs=zs, fetch=False)
    b.compute_gradients(X, Y, zs=zs, fetch=False)
    a.sgd_step(lr), b.sgd_step(lr)
    va, vb = dict(_values(a)), dict(_values(b))
    key = "DGP/layers/0/mixing/W"
    W0 = np.asarray(spec["convs"][0]["mix_W"])
    expect = W0 + lr * want[0]["mixing"]
    print("SGD: W rel %.3e (moved %.3e)" % (rel(va[key], expect), rel(expect, W0)))
    assert rel(expect, W0) >= 1e-5 and rel(va[key], expect) < 1e-9
    for k in va:
        if k != key:
            assert np.array_equal(va[k], vb[k]), k
    a.close(), b.close()
    gamma = 1e-5
    n = build_from_spec(copy.deepcopy(spec), X, Y)
    n.compute_gradients(X, Y, zs=zs, fetch=False)
    n.natgrad_step(gamma)
    v1 = dict(_values(n))
    assert np.array_equal(v1[key], W0)
    for li, (l, m) in enumerate(zip(spec["convs"] + [spec["head"]], n.layers)):
        mu1, L1 = natgrad_reference(np.asarray(l["q_mu"]), np.asarray(l["q_sqrt"]), want[li]["q_mu"], want[li]["q_sqrt"], gamma)
        print("natgrad L%d rel q_mu %.3e q_sqrt %.3e" % (li, rel(m.q_mu, mu1), rel(m.q_sqrt, L1)))
        assert rel(m.q_mu, mu1) < 1e-8 and rel(m.q_sqrt, L1) < 1e-8, (li, rel(m.q_mu, mu1), rel(m.q_sqrt, L1))
    for li in range(len(n.layers)):
        n.set_trainable(li, "q_mu", False), n.set_trainable(li, "q_sqrt", False)
    n.adam_step(0.01, 1)
    v2 = dict(_values(n))
    step = v2[key] - W0
    print("NatGrad + Adam: |W step| in [%.6g, %.6g]" % (np.abs(step).min(), np.abs(step).max()))
    assert np.allclose(step, 0.01 * np.sign(want[0]["mixing"]), rtol=1e-6, atol=0)
    assert np.array_equal(v2["DGP/layers/0/q_mu"], v1["DGP/layers/0/q_mu"])
    n.close()


# ---- 6. state ------------------------------------------------------------------------------------------------------------------------------------
def test_optimizer_state_round_trip_with_the_new_keys(ctx):
    spec, X, Y, (a, b) = _train_models("pad_lin", True)
    zs = ss.make_noise(spec, 4, seed=3)
    for _ in range(2):
        a.train_step(X[:4], Y[:4], 0.01, zs=zs)
    st = a.optimizer_state()
    assert st["t"] == 2 and st["layers/0/mixing/m"].shape == (3, 5) and st["layers/0/mixing/v"].any() and "layers/1/mixing/m" not in st
    for p, (_, v) in zip(b.parameters, _values(a)):
        p.assign(v)
    b.sync_parameters()
    b.set_optimizer_state(st)
    ea, eb = a.train_step(X[:4], Y[:4], 0.01, zs=zs), b.train_step(X[:4], Y[:4], 0.01, zs=zs)
    assert ea == eb
    for (k, x), (_, y) in zip(_values(a), _values(b)):
        assert np.array_equal(x, y), k
    bad = dict(st)
    del bad["layers/0/mixing/v"]
    with pytest.raises(ValueError, match="layers/0/mixing/v"):
        b.set_optimizer_state(bad)
    a.close(), b.close()


def test_checkpoint_round_trip_through_load_model(ctx, tmp_path):
    """ModelBuilder with --latent-gps, three Adam steps, save_model_parameters, ModelBuilder with --load-model: the same ELBO bit for bit at a
    fixed seed, and the key is in the file.  (--white: the reference's checkpoint holds no frozen prior patches Z0.)"""
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder, save_model_parameters, train
    rng = np.random.default_rng(0)
    X = rng.standard_normal((40, 10, 10, 1))
    Y = rng.integers(0, 10, (40, 1))
    args = ['--name', 't', '-M', '6,7,8', '--feature-maps', '4,2', '--filter-sizes', '3,3,3', '--strides', '1,1,1', '--paddings', '1,1,0',
            '--num-samples', '2', '--batch-size', '8', '--white', '--latent-gps', '2,3', '--identity-mean']
    np.random.seed(0)
    model = ModelBuilder(default_parser().parse_args(args), X, Y).build()
    assert [l.gp_count for l in model.layers[:-1]] == [2, 3] and [l.feature_maps_out for l in model.layers[:-1]] == [4, 2]
    assert all(l.centre_mean and not l.identity_mean for l in model.layers[:-1])
    hist = train(model, 3, lr=0.01)
    assert len(hist) == 3 and np.all(np.isfinite(hist))
    W = [np.array(l.mixing) for l in model.layers[:-1]]
    assert all(not np.array_equal(w, mixing_matrix("random", *w.shape, seed=li)) for li, w in enumerate(W))      # trained
    path = str(tmp_path / "ckpt.npy")
    saved = save_model_parameters(model, path, global_step=3)
    assert np.array_equal(saved["DGP/layers/1/mixing/W"], W[1])
    Xb, Yb = X[:8].reshape(8, -1), Y[:8].reshape(-1)
    e = model.compute_log_likelihood(Xb, Yb, seed=5)
    np.random.seed(1)
    builder = ModelBuilder(default_parser().parse_args(args + ['--load-model', 'ckpt']), X, Y, model_path=path)
    again = builder.build()
    assert builder.global_step == 3
    for l, w in zip(again.layers[:-1], W):
        assert np.array_equal(l.mixing, w)
    e2 = again.compute_log_likelihood(Xb, Yb, seed=5)
    print("ELBO %.12f, after the round trip %.12f" % (e, e2))
    assert e == e2
    model.close(), again.close()


# ---- 7. evaluation ---------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_predict_y_and_the_full_cov_refusal(ctx):
    import torch
    N, S, bs = 7, 2, 3
    spec, _, _, _ = _case("pad_lin")
    X, Y = syn.make_batch(R.CASES["pad_lin"]["hwc"], N, seed=23)
    spec = dict(copy.deepcopy(spec), S=S)
    zs = ss.make_noise(spec, N, seed=23)
    with torch.no_grad():
        out = tr.forward(spec, X, Y, zs)
    m, v = out["mean"].numpy(), out["var"].numpy()
    om, _, want = compose_ref.predictions(("robustmax", 10), m, v, Y)
    model = build_from_spec(spec, X, Y)
    r = model.evaluate(X, Y, S=S, batch_size=bs, zs=zs, per_image=True)
    p, _ = model.predict_y(X, S, zs=zs)
    print("evaluate: log density %.3e  p_mean %.3e  predict_y %.3e" % (rel(r["log_density"], want[:, 0]), rel(r["p_mean"], om.mean(axis=0)), rel(p, om)))
    assert rel(r["log_density"], want[:, 0]) < RTOL_EVAL and rel(r["p_mean"], om.mean(axis=0)) < RTOL_EVAL and rel(p, om) < RTOL_EVAL
    assert r["accuracy"] == np.mean(om.mean(axis=0).argmax(axis=1) == Y.reshape(-1))
    u = model.evaluate_uncertainty(X, Y, S=S, batch_size=bs, zs=zs, per_image=True)
    assert np.array_equal(u["log_density"], r["log_density"]) and np.array_equal(u["p_mean"], r["p_mean"])
    # views (tests/test_gpu_tta.py's recipe): the mirror makes X' [V N, ...] view-major, the torch forward runs on X' with the noise of row v N + i,
    # member s V + v is sample s on view v; the device takes the noise as [S, V, N, D]
    from test_gpu_tta import _lse_mean, _members, _views_of
    t = model.evaluate(X, Y, S=S, batch_size=bs, zs=zs, per_image=True, views=np.zeros((1, 3), np.int32))
    assert np.array_equal(t["log_density"], r["log_density"])                   # the identity view alone is the plain evaluation
    views = np.array([[0, 0, 0], [1, 0, 0], [0, -1, 1]], np.int32)
    V = len(views)
    zf = ss.make_noise(spec, V * N, seed=31)
    Xv = _views_of(X, R.CASES["pad_lin"]["hwc"], views)
    with torch.no_grad():
        ov = tr.forward(spec, Xv, np.tile(Y.reshape(-1), V), zf)
    pv, _, _ = compose_ref.predictions(("robustmax", 10), ov["mean"].numpy(), ov["var"].numpy(), np.tile(Y.reshape(-1), V))
    mem = _members(pv, V)
    pbar, logdens = mem.mean(axis=0), _lse_mean(np.log(mem[:, np.arange(N), Y.reshape(-1)]))
    t = model.evaluate(X, Y, S=S, batch_size=bs, zs=[z.reshape(S, V, N, -1) for z in zf], views=views, per_image=True)
    print("evaluate(views): log density %.3e  p_mean %.3e" % (rel(t["log_density"], logdens), rel(t["p_mean"], pbar)))
    assert rel(t["log_density"], logdens) < RTOL_EVAL and rel(t["p_mean"], pbar) < RTOL_EVAL
    assert not np.array_equal(t["p_mean"], r["p_mean"])
    c, fm = model.predict_patch_contributions(X, S, zs=zs)
    assert rel(fm, m) < RTOL and np.all(np.isfinite(c))
    for call in (lambda: model.predict_f_full_cov(X, S), lambda: model.predict_all_layers_full_cov(X, S)):
        with pytest.raises(NotImplementedError, match="mixed layer"):
            call()
    with pytest.raises(ValueError, match="zs\\[0\\] has"):      # the mixed layer's noise is P * G a row, not P * R
        model.compute_log_likelihood(X, Y, zs=[np.zeros((S, N, model.layers[0].num_outputs)), zs[1]])
    model.close()


# ---- 8. refusals; a model built from the flags ----------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    L = dev.lib()
    spec, X, Y, zs = _case("a_3_5")

    def refused(rc, word):
        assert rc == dev.ERR_ARG, rc
        with pytest.raises(dev.DcgpError, match=word):
            ctx._check(rc)
    plain = copy.deepcopy(spec)
    W = np.ascontiguousarray(plain["convs"][0].pop("mix_W"))
    plain["head"] = R.make_case("a_3_5", Rout=3)[0]["head"]      # an unmixed model: the head takes the layer's 3 maps
    m = build_from_spec(plain, X, Y)
    m._build()
    buf = np.empty_like(W)
    refused(L.dcgp_model_set_mixing(m._model, 1, W.ctypes.data, 3, 5), "head")
    refused(L.dcgp_model_set_mixing(m._model, 4, W.ctypes.data, 3, 5), "no layer")
    refused(L.dcgp_model_set_mixing(m._model, 0, W.ctypes.data, 4, 5), "G = 4")
    refused(L.dcgp_model_set_mixing(m._model, 0, W.ctypes.data, 3, 5), "R = 5")       # the head takes C = 3
    refused(L.dcgp_model_set_mixing(m._model, 0, W.ctypes.data, 3, 65), "R = 65")
    refused(L.dcgp_model_set_param(m._model, 0, b"mixing", W.ctypes.data, W.size), "not mixed")
    refused(L.dcgp_model_get_param(m._model, 0, b"mixing", buf.ctypes.data, buf.size), "not mixed")
    refused(L.dcgp_model_set_trainable(m._model, 0, b"mixing", 1), "not mixed")
    e0 = m.compute_log_likelihood(X, Y, zs=zs)
    I3 = np.ascontiguousarray(2.0 * np.eye(3))
    ctx._check(L.dcgp_model_set_mixing(m._model, 0, I3.ctypes.data, 3, 3))            # before the first gradient step: allowed
    e1 = m.compute_log_likelihood(X, Y, zs=zs)
    ctx._check(L.dcgp_model_set_mixing(m._model, 0, None, 0, 0))                      # ... and off again
    assert m.compute_log_likelihood(X, Y, zs=zs) == e0 != e1
    m.compute_gradients(X, Y, zs=zs, fetch=False)
    refused(L.dcgp_model_set_mixing(m._model, 0, I3.ctypes.data, 3, 3), "before the first")
    m.close()


def test_a_model_built_from_the_flags_trains(ctx):
    """ModelBuilder with --latent-gps on synthetic images: 20 Adam steps on one fixed batch and fixed noise; the ELBO is finite throughout and
    higher at the end than at the start."""
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder
    hwc = (12, 12, 1)
    X, Y = syn.make_batch(hwc, 48, seed=4)
    args = ['--name', 't', '-M', '8,8,8', '--feature-maps', '5,4', '--filter-sizes', '3,3,3', '--strides', '1,2,1', '--paddings', '1,0,0',
            '--num-samples', '2', '--batch-size', '16', '--latent-gps', '2,3']
    np.random.seed(0)
    model = ModelBuilder(default_parser().parse_args(args), X.reshape((48,) + hwc), Y.reshape(48, 1)).build()
    assert [l.mixing.shape for l in model.layers[:-1]] == [(2, 5), (3, 4)]
    Xb, Yb = X[:16], Y[:16]
    hist = [model.train_step(Xb, Yb, 0.01, seed=3) for _ in range(20)]
    hist.append(model.compute_log_likelihood(Xb, Yb, seed=3))
    print("ELBO %s" % np.array(hist))
    assert np.all(np.isfinite(hist)) and hist[-1] > hist[0]
    model.close()

"""Worker of tests/test_gpu_memcheck.py (not collected by pytest): ``python tests/memcheck_scenarios.py <name>`` builds one scenario in a fresh
process, runs it, and prints one line

    RESULT <sha256 of the concatenated result bytes> <n_bad> <all_finite 0/1>

with the guard report on stderr.  The test runs every scenario twice -- a clean environment, then DCGP_POISON_WS=1 DCGP_GUARD_WS=4096 (csrc/ctx.hip:
every fresh device allocation filled with NaNs and followed by a guard of 0xFF bytes) -- and demands the same hash, finite results and whole guards.
Nothing is compared with a reference here: the clean run of the same code is the reference, and that code's correctness is what the rest of the
suite pins.  Results are hashed whole (every gradient array, every prediction, every parameter after a step), never reduced to sums.

Scenarios (``names()``): ``compose:<case id>`` for a cover of tests/compose_cases.py in which every level of every factor occurs, ``ard``, ``mixed``,
``evaluate``, ``train_run`` and ``operators``.  Inputs come from the helpers of tests/, noise is explicit wherever a call takes noise, and the
sizes are the cases' own.  ``check_guards()`` runs before every ``model.close()`` and once at the end.

Not built: ``pad_images`` on its own -- csrc/pad.hip has no entry point in include/dcgp.h; it runs inside the padded stacks of the compose cover
(ch_264_72, ch_res), the ``mixed`` scenario (pad_lin) and the augmentation of ``train_run``."""
import copy
import ctypes as C
import hashlib
import os
import sys
import time

import numpy as np

T0 = time.perf_counter()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import compose_cases as cc      # noqa: E402


# ---- the compose cover ---------------------------------------------------------------------------------------------------------------------
def compose_cover():
    """Ids of a subset of compose_cases.CASES in which every level of every factor of compose_cases.FACTORS occurs: greedy, the case that adds the
    most levels not yet seen, the earliest of the table on a tie.  Deterministic (tests/test_host_memcheck.py asserts the cover without a GPU)."""
    todo = {(f, level) for f in cc.NAMES for level in cc.FACTORS[f]}
    picked = []
    while todo:
        gains = [len(todo & set(case.items())) for case in cc.CASES]
        best = max(gains)
        assert best > 0, sorted(todo)
        case = cc.CASES[gains.index(best)]
        picked.append(cc.case_id(case))
        todo -= set(case.items())
    return picked


def names():
    return ["compose:" + cid for cid in compose_cover()] + ["ard", "mixed", "evaluate", "train_run", "operators"]


# ---- results and guards ------------------------------------------------------------------------------------------------------------------
class Results:
    """The scenario's results, hashed in the order they arrive; whether all of them were finite; the guard violations seen so far."""

    def __init__(self):
        self.h = hashlib.sha256()
        self.finite = True
        self.n_bad = 0
        self.count = 0

    def add(self, what, value):
        if isinstance(value, dict):
            for k in sorted(value, key=str):
                self.add("%s/%s" % (what, k), value[k])
            return
        if isinstance(value, (list, tuple)):
            for i, v in enumerate(value):
                self.add("%s/%d" % (what, i), v)
            return
        if value is None:
            return
        a = np.ascontiguousarray(value)
        if a.dtype.kind not in "fiub":
            raise TypeError("%s: cannot hash %r" % (what, a.dtype))
        if a.dtype.kind == "f" and not np.all(np.isfinite(a)):
            self.finite = False
            print("NOT FINITE: %s (%d of %d entries)" % (what, int(np.sum(~np.isfinite(a))), a.size), file=sys.stderr)
        self.h.update(("%s %s %r|" % (what, a.dtype.str, a.shape)).encode())
        self.h.update(a.tobytes())
        self.count += 1

    def add_uncertainty(self, what, r):
        """evaluate_uncertainty's result: the reliability table is NaN by definition where a bin is empty -- the counts and the filled bins are hashed."""
        r = dict(r)
        table = r.pop("reliability")
        filled = table["count"] > 0
        assert np.all(np.isnan(table["confidence"][~filled])) and np.all(np.isnan(table["accuracy"][~filled]))
        self.add(what, r)
        self.add(what + "/reliability", {"count": table["count"], "confidence": table["confidence"][filled], "accuracy": table["accuracy"][filled]})

    def check(self, ctx, where):
        print("%.2f s: %s, %d results so far" % (time.perf_counter() - T0, where, self.count), file=sys.stderr)
        n, report = ctx.check_guards()
        if n:
            print("GUARD %s: %d violation(s): %s" % (where, n, report), file=sys.stderr)
        self.n_bad += n

    def close(self, model, where):
        self.check(model._ctx, "before close of " + where)
        model.close()


def values(model):
    model.pull_parameters()
    return {p.pathname: np.array(p.value) for p in model.parameters}


def model_calls(res, tag, model, X, Y, zs, S):
    """What every model scenario runs: ELBO; compute_gradients under both dedup settings; an Adam, an SGD and a NatGrad step; predict_y."""
    res.add(tag + "/elbo", model.compute_log_likelihood(X, Y, zs=zs, return_parts=True))
    for dedup in (False, True):
        model.dedup_layer0 = dedup
        e, g = model.compute_gradients(X, Y, zs=zs)
        res.add("%s/grad dedup=%d/elbo" % (tag, dedup), e)
        res.add("%s/grad dedup=%d" % (tag, dedup), g)
    model.adam_step(0.01, 1)
    res.add(tag + "/after adam", values(model))
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.sgd_step(1e-4)
    res.add(tag + "/after sgd", values(model))
    model.compute_gradients(X, Y, zs=zs, fetch=False)
    model.natgrad_step(1e-5)
    res.add(tag + "/after natgrad", values(model))
    res.add(tag + "/predict_y", model.predict_y(X, S, zs=zs))


# ---- model scenarios ---------------------------------------------------------------------------------------------------------------------
def run_compose(res, cid):
    import compose_ref as cr
    from deepcgp_amd.models import build_from_spec
    spec, X, Y, zs, lik = cc.make_case(cc.BY_ID[cid])
    model = build_from_spec(copy.deepcopy(spec), X.copy(), Y.copy(), likelihood=cr.make_likelihood(lik))
    model_calls(res, cid, model, X, Y, zs, spec["S"])
    res.close(model, cid)


def run_ard(res):
    import ard_ref as ar
    from deepcgp_amd.models import build_from_spec
    spec, X, Y, zs = ar.ard_case("small3_M20")
    model = build_from_spec(spec, X, Y)
    model_calls(res, "ard", model, X, Y, zs, spec["S"])
    res.close(model, "ard")


def run_mixed(res):
    import mixing_ref as mr
    from deepcgp_amd.models import build_from_spec
    spec, X, Y, zs = mr.make_case("pad_lin")       # 3 latent GPs into 5 maps (G < R), a padded layer with a trained mean filter
    assert spec["convs"][0]["mix_W"].shape == (3, 5)
    model = build_from_spec(spec, X, Y)
    model_calls(res, "mixed", model, X, Y, zs, spec["S"])
    res.close(model, "mixed")


VIEWS = np.array([(0, 0, 0), (-2, 3, 1), (1, 0, 0)], np.int32)      # the identity, a flip with a negative shift, a plain shift (tests/test_gpu_tta.py)


def run_evaluate(res):
    import live_specs as ls
    from deepcgp_amd.models import build_from_spec
    spec, X, Y, zs = ls.make_case("small3_M20")
    S, N, V = spec["S"], X.shape[0], len(VIEWS)
    model = build_from_spec(spec, X, Y)
    rng = np.random.default_rng(5)
    zv = [rng.standard_normal((S, V, N, z.shape[-1])) for z in zs]         # [S, V, N, D]: what a call with views takes
    res.add("evaluate", model.evaluate(X, Y, S=S, batch_size=2, zs=zs, per_image=True))
    res.add("predict_density", model.predict_density(X, Y, S, zs=zs))
    res.add_uncertainty("evaluate_uncertainty", model.evaluate_uncertainty(X, Y, S=S, batch_size=2, zs=zs, bins=5, per_image=True))
    res.add("evaluate views", model.evaluate(X, Y, S=S, batch_size=2, zs=zv, views=VIEWS, per_image=True))
    res.add("predict_density views", model.predict_density(X, Y, S, zs=zv, views=VIEWS))
    res.add_uncertainty("evaluate_uncertainty views", model.evaluate_uncertainty(X, Y, S=S, batch_size=2, zs=zv, views=VIEWS, bins=5, per_image=True))
    res.add("predict_f_full_cov", model.predict_f_full_cov(X, S, zs=zs))
    kern = model.layers[-1].kern
    A, B = (np.random.default_rng(s).standard_normal((n, X.shape[1] if len(model.layers) == 1 else kern.view.input_size[0] * kern.view.input_size[1]
                                                      * kern.view.feature_maps)) * 0.7 for s, n in ((1, 7), (2, 5)))
    res.add("ConvKernel.K(X)", kern.K(A))
    res.add("ConvKernel.K(X, X2)", kern.K(A, B))
    res.add("patch evidence", model.predict_patch_contributions(X, S, zs=zs))
    for dedup in (False, True):
        model.dedup_layer0 = dedup
        for objective in ("density", "elbo"):
            res.add("input_gradient %s dedup=%d" % (objective, dedup), model.input_gradient(X, Y, objective=objective, zs=zs))
    res.close(model, "evaluate")


def run_train_run(res):
    """tests/test_gpu_train_run.py's smallest geometry (g973_M5), augmentation and clipping on, two steps per device call: two calls, the state
    saved, a fresh model resumed from it exactly, one more call; then the sharded Adam step of tests/test_gpu_model.py at 3 ranks."""
    import live_specs as ls
    from deepcgp_amd import synthetic as syn
    from deepcgp_amd.augment import Augmentation
    from deepcgp_amd.models import build_from_spec
    pool, batch, every = 23, 5, 2
    k = dict(hwc=(9, 7, 3), convs=[(4, 2, 3)], head=(2, 1), M=5, c=1.0, a=0.1)
    spec = ls.live_spec(S=2, **k)
    X, _ = syn.make_batch(k["hwc"], pool, seed=7)
    Y = np.random.default_rng(99).integers(0, 10, pool).astype(np.int32)
    rng = np.random.default_rng(5)
    idx = np.stack([rng.choice(pool, batch, replace=False) for _ in range(6)]).astype(np.int64)
    idx[0] = [0, 22, 5, 11, 17]
    lrs = np.array([0.01, 0.01, 0.01, 0.001, 0.001, 0.001])

    def fresh():
        m = build_from_spec(copy.deepcopy(spec), X.copy(), Y.copy())
        m.dedup_layer0 = True
        m.set_augmentation(Augmentation(2, True))
        m.set_grad_clip(5.0)
        m.attach_dataset()
        return m
    a = fresh()
    for period in range(2):
        lo = period * every
        res.add("run period %d" % period, a.train_run(idx[lo:lo + every], lrs[lo:lo + every], seed=11 + lo))
        res.add("grad norms period %d" % period, a.last_grad_norms)
    saved, state = values(a), a.optimizer_state()
    res.add("saved", saved)
    res.add("saved optimiser state", state)
    a.detach_dataset()
    res.close(a, "train_run, first model")
    b = fresh()
    params = dict(saved)
    for p in b.parameters:
        p.assign(params[p.pathname])
    b.sync_parameters()
    b.set_optimizer_state(state)
    res.add("resumed period", b.train_run(idx[4:6], lrs[4:6], seed=11 + 4))
    res.add("resumed values", values(b))
    res.add("resumed optimiser state", b.optimizer_state())
    b.detach_dataset()
    res.close(b, "train_run, resumed model")
    # the sharded Adam step, three ranks' shards played in one process
    hwc, N = (12, 12, 1), 3
    sspec = syn.make_spec(hwc, [(3, 1, 2)], (3, 1), 11, S=2, num_data=200, seed=4, conv_q_sqrt_scale=0.3, variance=2.0, ls=1.5)
    Xs, Ys = syn.make_batch(hwc, N, seed=4)
    m = build_from_spec(sspec, Xs, Ys)
    m.set_trainable(0, "q_mu", False)
    for t in (1, 2):
        m.compute_gradients(Xs, Ys, zs=syn.make_noise(sspec, N, seed=50 + t), fetch=False)
        m.debug_sharded_adam(3, 0.05, t)
    res.add("sharded adam", values(m))
    res.add("sharded adam elbo", m.compute_log_likelihood(Xs, Ys, zs=syn.make_noise(sspec, N, seed=60)))
    res.close(m, "sharded adam")


# ---- the operator entry points -------------------------------------------------------------------------------------------------------------
def _rbf(A, B, variance, ls):
    d = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * A @ B.T
    return variance * np.exp(-0.5 * np.maximum(d, 0.0) / ls ** 2)


def _gp_inputs(rng, M, R, L, scale=0.5):
    Z = rng.standard_normal((M, L))
    q_mu = rng.standard_normal((M, R))
    q_sqrt = np.tril(rng.standard_normal((R, M, M))) * scale + np.eye(M)[None]
    return Z, q_mu, q_sqrt


def ragged_gemm_cases():
    """The entries of tests/gemm_cases.py with an output edge that is no multiple of the case's tile (the symmetric long contraction's own kernel
    works on 32-row fragments)."""
    import gemm_cases as gc
    out = []
    for c in gc.CASES:
        tile = c["expect"].get("tile", 32)
        if c["M"] % tile or c["N"] % tile:
            out.append(c)
    return out


def _gemm(res, ctx, c, rng):
    """tests/test_gpu_gemm.py::_call with C cut to exactly the extent the call addresses: the last element of the last output is the buffer's last."""
    import gemm_cases as gc
    from deepcgp_amd import device as dev
    L = dev.lib()
    d = gc.build(c, rng)
    n_c = (c["batch"] - 1) * c["c_bs"] + (c["M"] - 1) * c["c_rs"] + c["N"]
    dA = ctx.to_device(d["A_buf"])
    dB = dA if c["sym"] else ctx.to_device(d["B_buf"])
    dC = ctx.to_device(d["C_buf"][:n_c])
    vec = {k: ctx.to_device(d[k + "_buf"]) if d[k + "_buf"] is not None else None for k in ("ks", "cs", "sv", "sx")}

    def ptr(k):
        return vec[k].ptr if vec[k] is not None else None
    pa, pb = dA.ptr + 8 * c["a_off"], dB.ptr + 8 * c["b_off"]
    with ctx.options(gemm_tile=c["gemm_tile"], no_syrk=c["no_syrk"]):
        head = (ctx.handle, pa, c["a_rs"], c["a_cs"], c["a_bs"], pb, c["b_rs"], c["b_cs"], c["b_bs"], dC.ptr, c["c_rs"], c["c_bs"], c["M"], c["N"], c["K"],
                c["batch"], c["alpha"], int(c["accumulate"]))
        if c["entry"] == "strided":
            ctx._check(L.dcgp_gemm_strided(*head, ptr("cs"), c["cs_s"], c["cs_bs"], ptr("ks"), c["ks_s"], c["ks_bs"], c["flags"]))
        else:
            ctx._check(L.dcgp_gemm_strided_ex(*head, ptr("sv"), c["sv_bs"], ptr("sx"), c["sx_rs"], c["sx_bs"], c["flags"]))
    res.add("gemm " + c["name"], dC.numpy())


def run_operators(res):
    from deepcgp_amd import device as dev
    from deepcgp_amd import kernels as K
    from deepcgp_amd.conditionals import conditional
    from deepcgp_amd.kernels import RBF, AdditivePatchKernel, ConvKernel, InducingPoints, PatchInducingFeatures
    from deepcgp_amd.layers import ConvLayer, MultiOutputConvKernel, SVGP_Layer, _potrf
    from deepcgp_amd.likelihoods import MultiClass
    from deepcgp_amd.views import FullView
    ctx = dev.get_context()
    L = dev.lib()
    # conditional: P x M x N Kmn, white and not, with and without q_sqrt, and full_cov
    for P, M, N, R in ((3, 4, 5, 2), (2, 37, 130, 10), (2, 130, 33, 3), (2, 384, 40, 3)):
        rng = np.random.default_rng(7 * M + P)
        Ld = 9
        Z, q_mu, q_sqrt = _gp_inputs(rng, M, R, Ld)
        Kmm = _rbf(Z, Z, 5.0, 3.0) + 1e-6 * np.eye(M)
        Xp = rng.standard_normal((P, N, Ld))
        Kmn = np.stack([_rbf(Z, Xp[p], 5.0, 3.0) for p in range(P)])
        Knn = np.full((P, N), 5.0) + rng.random((P, N)) * 0.1
        Knn_full = np.stack([_rbf(Xp[p], Xp[p], 5.0, 3.0) for p in range(P)])
        for white in (False, True):
            tag = "conditional %s white=%d" % ((P, M, N, R), white)
            res.add(tag, conditional(Kmn, Kmm, Knn, q_mu, q_sqrt=q_sqrt, white=white))
            res.add(tag + " no q_sqrt", conditional(Kmn, Kmm, Knn, q_mu, q_sqrt=None, white=white))
            res.add(tag + " full_cov", conditional(Kmn, Kmm, Knn_full, q_mu, full_cov=True, q_sqrt=q_sqrt, white=white))
    res.check(ctx, "conditional")
    # conv_layer: the one-launch layer kernel and the sweep + GEMM route
    for H, W, Cc, f, s, M, R, N in ((9, 7, 3, 4, 2, 5, 3, 4), (28, 28, 1, 5, 2, 70, 10, 3)):
        rng = np.random.default_rng(1000 * M + R)
        X = rng.standard_normal((N, H * W * Cc))
        v = FullView((H, W), f, Cc, s)
        Z, q_mu, q_sqrt = _gp_inputs(rng, M, R, v.patch_length, scale=0.05)
        Z *= 1.5
        for white in (False, True):
            layer = ConvLayer(RBF(v.patch_length, 5.0, 5.0), None, PatchInducingFeatures(Z), v, white=white, gp_count=R, q_mu=q_mu, q_sqrt=q_sqrt)
            z = rng.standard_normal((N, layer.num_outputs))
            tag = "conv_layer M=%d white=%d " % (M, white)
            res.add(tag + "fused", layer._forward(X, z))
            with ctx.options(no_fused_layer=1):
                res.add(tag + "unfused", layer._forward(X, z))
            res.add(tag + "KL", layer.KL())
            if M == 70 and not white:
                for shape in range(8):
                    with ctx.options(fused_shape=shape):
                        res.add(tag + "shape %d" % shape, layer._forward(X, z))
                with ctx.options(fused_shape=0, fused_split=3, fused_parts=0):
                    res.add(tag + "split 3", layer._forward(X, z))
                with ctx.options(fused_shape=0, fused_parts=3):
                    res.add(tag + "parts 3", layer._forward(X, z))
    res.check(ctx, "conv_layer")
    # kuf in both layouts, scalar and ARD lengthscales (tests/test_gpu_ard.py: GEOMS)
    for H, W, Cc, f, s, M in ((12, 12, 1, 3, 1, 6), (13, 13, 2, 4, 3, 33), (14, 14, 10, 5, 1, 72), (28, 28, 1, 5, 2, 200), (28, 28, 1, 5, 2, 264),
                              (9, 9, 11, 5, 2, 20)):
        rng = np.random.default_rng(H + M)
        N = 3
        X = rng.standard_normal((N, H, W, Cc))
        v = FullView((H, W), f, Cc, s)
        Lp, P = v.patch_length, v.patch_count
        Z = rng.standard_normal((M, Lp))
        lsc = 0.9 * np.sqrt(Lp) * (0.8 + 0.4 * rng.random(Lp))
        for name, k in (("ard", RBF(Lp, 1.7, lsc, ARD=True)), ("scalar", RBF(Lp, 1.7, 0.9 * np.sqrt(Lp)))):
            tag = "kuf %s %s " % ((H, W, Cc, f, s, M), name)
            res.add(tag + "Kuu", k._gram(Z, 1e-3))
            res.add(tag + "[P, M, N]", MultiOutputConvKernel(k, H * W * Cc, P).Kuf(Z, (X, v)))
            dX, dZ, out = ctx.to_device(X), ctx.to_device(Z), ctx.empty((M, N * P))
            k._kuf(ctx, dX, N, H, W, Cc, f, s, dZ, M, out, 1)
            res.add(tag + "[M, N P]", out.numpy())
    res.check(ctx, "kuf")
    # the head's kernels: the unit sweep (Kzx, Kdiag), Kzz, the additive kernel, the head's conditional
    for H, W, Cc, f, s, M, N in ((7, 7, 1, 2, 1, 5, 3), (13, 11, 10, 5, 1, 33, 4)):
        rng = np.random.default_rng(11 * M + H)
        X = rng.standard_normal((N, H * W * Cc))
        X[0, : H * W * Cc // 2] += 6.0
        v = FullView((H, W, Cc), f, Cc, s)
        w = rng.standard_normal(v.patch_count)
        Z, q_mu, q_sqrt = _gp_inputs(rng, M, 3, v.patch_length, 0.3)
        for var, ls_ in ((5.0, 5.0), (0.7, 1.3)):
            tag = "head %s var=%g " % ((H, W, Cc, f, s, M, N), var)
            k = ConvKernel(RBF(v.patch_length, var, ls_), v, w)
            res.add(tag + "Kzx", k.Kzx(Z, X))
            res.add(tag + "Kdiag", k.Kdiag(X))
            res.add(tag + "Kzz", k.Kzz(Z))
            a = AdditivePatchKernel(RBF(v.patch_length, var, ls_), v, w)
            res.add(tag + "additive Kzx", a.Kzx(Z, X))
            res.add(tag + "additive Kdiag", a.Kdiag(X))
        for white in (False, True):
            layer = SVGP_Layer(ConvKernel(RBF(v.patch_length, 5.0, 5.0), v, np.abs(w) + 0.5), 3, PatchInducingFeatures(Z), None, white, q_mu, q_sqrt)
            res.add("head %s conditional white=%d" % ((H, W, Cc, f, s, M, N), white), layer.conditional_ND(X))
            res.add("head %s KL white=%d" % ((H, W, Cc, f, s, M, N), white), layer.KL())
    res.check(ctx, "head kernels")
    # the dense RBF-ARD head
    D, M, N, R = 20, 7, 5, 10
    rng = np.random.default_rng(D + M)
    X, Z = rng.standard_normal((N, D)), rng.standard_normal((M, D))
    lsd = 3.0 * (0.8 + 0.4 * rng.random(D))
    _, q_mu, q_sqrt = _gp_inputs(rng, M, R, D, 0.2)
    k = RBF(D, 2.5, lsd, ARD=True)
    res.add("dense head K(Z)", k.K(Z))
    res.add("dense head K(Z, X)", k.K(Z, X))
    for white in (False, True):
        layer = SVGP_Layer(k, R, InducingPoints(Z), None, white=white, q_mu=q_mu, q_sqrt=q_sqrt)
        res.add("dense head conditional white=%d" % white, layer.conditional_ND(X))
        res.add("dense head KL white=%d" % white, layer.KL())
    res.check(ctx, "dense head")
    # kmeans, robustmax, extract_patches
    rng = np.random.default_rng(0)
    pts = np.concatenate([rng.standard_normal((333, 9)) + c for c in (0.0, 3.0, -2.5)])

    class FixedRows:
        rows = np.random.default_rng(5).choice(pts.shape[0], size=17, replace=False)

        def choice(self, n_, size, replace):
            return self.rows
    res.add("kmeans", K.kmeans(pts, 17, rng=FixedRows()))
    n = 7
    rng = np.random.default_rng(n)
    mu, var = rng.standard_normal((n, 10)) * 2.0, rng.random((n, 10)) * 3.0
    var[0, :3] = 0.0
    y = rng.integers(0, 10, n)
    lik = MultiClass(10)
    res.add("robustmax varexp", lik.variational_expectations(mu, var, y))
    res.add("robustmax predict", lik.predict_mean_and_var(mu, var))
    for H, W, Cc, f, s in ((9, 7, 3, 4, 2), (8, 8, 1, 3, 1)):
        Xi = np.random.default_rng(0).standard_normal((3, H, W, Cc))
        v = FullView((H, W), f, Cc, s)
        res.add("extract_patches %s" % ((H, W, Cc, f, s),), v.extract_patches(Xi))
        res.add("extract_patches_PNL %s" % ((H, W, Cc, f, s),), v.extract_patches_PNL(Xi))
    res.check(ctx, "kmeans, robustmax, extract_patches")
    # the strided GEMM wherever an output edge is no multiple of the tile
    rng = np.random.default_rng(3)
    for c in ragged_gemm_cases():
        _gemm(res, ctx, c, rng)
    res.check(ctx, "gemm")
    # the factorisation chain alone: Gram matrix, factor, inverse of the factor
    for M in (4, 37, 41, 200, 256, 264, 1000):
        rng = np.random.default_rng(M)
        Z = rng.standard_normal((M, 25)) * 2.0
        Kuu = RBF(25, 5.0, 5.0)._gram(Z, 1e-6)
        Lc = _potrf(Kuu)
        dL, dX = ctx.to_device(Lc), ctx.empty((M, M))
        ctx._check(L.dcgp_trtri_lower(ctx.handle, dL.ptr, M, dX.ptr))
        res.add("chain M=%d" % M, (Kuu, Lc, dX.numpy()))
    res.check(ctx, "factorisation chain")
    # the chain as a model step runs it, right-hand sides riding (tests/chain_cases.py): a full entry, a prior's sums-only entry and one that carries nothing at
    # Mp = 48; six riding matrices at Mp = 256, two row tiles per workgroup -- the group's Yw, the diagonal blocks' hand-over buffer and the sums
    import chain_cases as chain
    for batch, M in (("b", 48), ("d6", 256)):
        inp = chain.build(batch, M)
        for alone in (True, False):
            out = chain.run(ctx, inp, alone=alone, defer=not alone)
            tag = "chain %s alone=%d" % (chain.case_id(batch, M), alone)
            res.add(tag, {k: out[k] for k in ("info", "L", "Linv", "LinvT", "G", "alpha")})
            res.add(tag + "/sums", [s[chain.written_slots(e, inp["Mp"])] if s is not None else None for s, e in zip(out["sums"], inp["ents"])])
    res.check(ctx, "riding factorisation chain")
    # the per-output likelihoods' tails on a head wider than the ELBO tail's 1024 doubles of LDS (tests/test_gpu_pointwise.py: K = 1030, two chunks per row)
    import compose_ref as cr
    import test_gpu_pointwise as pw
    from deepcgp_amd.models import build_from_spec
    for lik in pw.LIKS:
        spec, X, Ylab, Y, zs = pw.make_case(1030, lik)
        model = build_from_spec(copy.deepcopy(spec), X.copy(), Y.copy(), likelihood=cr.make_likelihood(lik))
        tag = "wide head %s" % lik[0]
        res.add(tag + "/elbo", model.compute_log_likelihood(X, Y, zs=zs, return_parts=True))
        res.add(tag + "/grad", model.compute_gradients(X, Y, zs=zs)[1])
        res.add(tag + "/evaluate", model.evaluate(X, Y, S=spec["S"], batch_size=2, zs=zs, per_image=True))
        res.close(model, tag)


def main(name):
    from deepcgp_amd import device as dev
    res = Results()
    if name.startswith("compose:"):
        run_compose(res, name.split(":", 1)[1])
    else:
        {"ard": run_ard, "mixed": run_mixed, "evaluate": run_evaluate, "train_run": run_train_run, "operators": run_operators}[name](res)
    import gc
    gc.collect()                      # device arrays no longer referenced are freed, and their guards checked, before the last look
    res.check(dev.get_context(), "the end")
    assert res.count > 0
    # (which modes this process ran under, as the library and the environment have them: the test holds the two runs to it)
    print("MODES guard %d poison %d" % (dev.get_context().guard_bytes(), int("DCGP_POISON_WS" in os.environ)))
    print("RESULT %s %d %d" % (res.h.hexdigest(), res.n_bad, int(res.finite)))


if __name__ == "__main__":
    main(sys.argv[1])

#!/usr/bin/env python
"""usage (GPU box): python tools/inducing_init_time.py [--rounds 5] [--adam-steps 200] [--skip-quality] [--out profiles/inducing_init_time.json]

What greedy conditional-variance selection of the inducing patches (csrc/greedy.hip, --inducing-init greedy) costs and what it buys, beside
the k-means it can stand in for (csrc/kmeans.hip).

Timing, per shape (n candidates of d elements, k selected): ``first_layer`` n = 25600, d = 25, k = 256 (5 x 5 x 1 patches of cfg2's synthetic
images); ``second_layer`` n = 38400, d = 250, k = 384 and ``dense_head`` n = 38400, d = 490, k = 384 (standard normal rows: what these layers
see depends on the layers below).  RBF, variance 5, lengthscale sqrt(d) on the normal rows and 5 on the patches; floor 0, so that all k
launches do their work.  One warm-up, then ``--rounds`` rounds that visit dcgp_greedy_variance and dcgp_kmeans in turn on the same
device-resident candidates (host clock around the synchronous entry: transposition, allocations and frees included); medians and spreads
((max - min) / median).  Beside them, by the library's event timers: the pivot launches alone (``pivots_ms``), the same on d = 4 rows (a
full-rank Gram matrix, so no stall) where the column evaluation is four loads and the projection's k (k - 1) / 2 n reads and 3 k n accesses of
residual and factor remain (``projection_GBps``),
and k EMPTY dependent launches of the same grid (dcgp_debug_empty_launches): ``boundary_share`` = their time / the pivot launches'.

Quality, for both initialisations, on cfg2's model (28 x 28 x 1 synthetic images of deepcgp_amd.synthetic, conv f5 s2 into head f5, M = 256,
variance = lengthscale = 5), the candidates being the 100 M patches both recipes draw: cond(K_uu + JITTER I), the smallest pivot of its
Cholesky factor, the candidates' Nystrom trace tr(K_ff - K_fu inv(K_uu + JITTER I) K_uf) (host NumPy), n_greedy at the default floor, and
the ELBO of one fixed batch after 0 and after ``--adam-steps`` Adam steps (lr 1e-3, same minibatches, same seeds).

No figure is fixed in advance.  Prints one JSON line."""
import argparse
import copy
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"first_layer": (25600, 25, 256), "second_layer": (38400, 250, 384), "dense_head": (38400, 490, 384)}
VARIANCE = 5.0


def summary(ts):
    ts = np.array(ts)
    return {"legs_ms": [float(t) for t in ts], "ms": float(np.median(ts)), "spread": float((ts.max() - ts.min()) / np.median(ts))}


def images(n):
    from deepcgp_amd import synthetic as syn
    return syn._blur_images(np.random.default_rng(1235), n, 28, 28, 1)


def greedy_call(ctx, dP, n, d, k, ls, floor=0.0):
    from deepcgp_amd import device as dev
    rows, trace, resid, ng = ctx.empty((k,), np.int32), ctx.empty((k,)), ctx.empty((n,)), C.c_int(0)
    ctx.sync()
    t0 = time.perf_counter()
    ctx._check(dev.lib().dcgp_greedy_variance(ctx.handle, dP.ptr, n, d, k, 0, VARIANCE, ls, 0.0, None, floor, rows.ptr, trace.ptr, resid.ptr, None,
                                              C.byref(ng)))
    return 1e3 * (time.perf_counter() - t0), ng.value, trace.numpy()


def kmeans_call(ctx, dP, n, d, k, tol, rows):
    from deepcgp_amd import device as dev
    dC, iters = ctx.empty((k, d)), C.c_int(0)
    ctx.sync()
    t0 = time.perf_counter()
    ctx._check(dev.lib().dcgp_kmeans(ctx.handle, dP.ptr, n, d, k, rows.ctypes.data, 300, tol, dC.ptr, C.byref(iters)))
    return 1e3 * (time.perf_counter() - t0), iters.value


def pivots_ms(ctx, dP, n, d, k, ls):
    ctx.timing_enable(1)
    ctx.timing_reset()
    _, ng, _ = greedy_call(ctx, dP, n, d, k, ls)
    t = ctx.timing().get("greedy_pivots", (0, 0.0))
    ctx.timing_enable(0)
    return float(t[1]), ng


def timing(ctx, rounds):
    from deepcgp_amd import device as dev
    from deepcgp_amd.models import draw_patches
    out = {}
    for name, (n, d, k) in SHAPES.items():
        rng = np.random.default_rng(n + d)
        if name == "first_layer":
            P, ls = draw_patches(images(256), n, 5, rng=np.random.RandomState(0)), 5.0
        else:
            P, ls = rng.standard_normal((n, d)), float(np.sqrt(d))
        dP = ctx.to_device(P)
        tol = 1e-4 * float(np.mean(np.var(P, axis=0)))
        start = np.ascontiguousarray(rng.choice(n, size=k, replace=False), np.int32)
        g, km, ng, iters = [], [], 0, 0
        for r in range(rounds + 1):              # round 0: warm-up
            tg, ng, trace = greedy_call(ctx, dP, n, d, k, ls)
            tk, iters = kmeans_call(ctx, dP, n, d, k, tol, start)
            if r:
                g.append(tg)
                km.append(tk)
        piv, _ = pivots_ms(ctx, dP, n, d, k, ls)
        # the projection nearly alone: d = 4 standard normal rows at lengthscale 0.3 -- a Gram matrix of full rank (no stall: checked), four loads a column
        d4 = ctx.to_device(np.random.default_rng(4).standard_normal((n, 4)))
        proj, ng4 = pivots_ms(ctx, d4, n, 4, k, 0.3)
        assert ng4 == k, ("the projection-only run stalled", ng4, k)
        nwg = (n + 255) // 256
        empty = C.c_double(0.0)
        ctx._check(dev.lib().dcgp_debug_empty_launches(ctx.handle, k, nwg, C.byref(empty)))      # warm
        ctx._check(dev.lib().dcgp_debug_empty_launches(ctx.handle, k, nwg, C.byref(empty)))
        proj_bytes = 8.0 * n * (k * (k - 1) / 2.0 + 3.0 * k)
        out[name] = {"n": n, "d": d, "k": k, "greedy": summary(g), "kmeans": dict(summary(km), iterations=iters), "n_greedy": ng,
                     "trace_first_last": [float(trace[0]), float(trace[-1])],
                     "greedy_over_kmeans": float(np.median(g) / np.median(km)), "pivots_ms": piv, "pivots_d4_ms": proj,
                     "projection_GBps": proj_bytes / proj * 1e-6, "column_read_GBps": 8.0 * n * d * k / max(piv - proj, 1e-9) * 1e-6,
                     "empty_launches_ms": empty.value, "boundary_us_each": 1e3 * empty.value / k, "boundary_share": empty.value / piv,
                     "workgroups": nwg}
    return out


def rbf(A, B, variance, ls):
    d2 = np.maximum(np.sum(A * A, 1)[:, None] + np.sum(B * B, 1)[None, :] - 2.0 * A @ B.T, 0.0)
    return variance * np.exp(-0.5 * d2 / ls ** 2)


def z_quality(Z, cand, variance, ls):
    from deepcgp_amd.kernels import JITTER
    Kuu = rbf(Z, Z, variance, ls) + JITTER * np.eye(len(Z))
    Lc = np.linalg.cholesky(Kuu)
    A = np.linalg.solve(Lc, rbf(Z, cand, variance, ls))
    return {"cond": float(np.linalg.cond(Kuu)), "smallest_pivot": float(np.min(np.diag(Lc))),
            "nystrom_trace": float(len(cand) * variance - np.sum(A * A)), "trace_of_prior": float(len(cand) * variance),
            "distinct_rows": int(len({z.tobytes() for z in np.round(Z, 12)}))}


def quality(adam_steps):
    from deepcgp_amd import synthetic as syn
    from deepcgp_amd.kernels import JITTER, RBF, _cluster_patches, greedy_variance
    from deepcgp_amd.models import build_from_spec, draw_patches
    spec0, _, _ = syn.make_config("cfg2_mnist_CH_M256")
    c0, h0 = spec0["convs"][0], spec0["head"]
    M = c0["M"]
    imgs = images(512)
    feats = syn._identity_conv(imgs, c0["f"], c0["R"], c0["s"])
    labels = np.random.default_rng(7).integers(0, 10, size=512).astype(np.int32)
    out = {"M": M, "candidates": 100 * M, "adam_steps": adam_steps, "lr": 1e-3}
    for init in ("kmeans", "greedy"):
        res, Zs = {}, []
        for li, (src, lay) in enumerate(((imgs, c0), (feats, h0))):
            np.random.seed(100 + li)             # both recipes draw the same candidates
            cand = draw_patches(src, 100 * M, lay["f"])
            np.random.seed(100 + li)
            if init == "kmeans":
                Z = _cluster_patches(src, M, lay["f"])
                extra = {}
            else:
                Z, info = greedy_variance(cand, M, RBF(cand.shape[1], lay["variance"], lay["ls"]), return_info=True)
                extra = {"n_greedy": info["n_greedy"], "floor": JITTER, "trace_after_n_greedy": float(info["trace"][max(info["n_greedy"] - 1, 0)])}
            res["layer%d" % li] = dict(z_quality(Z, cand, lay["variance"], lay["ls"]), **extra)
            Zs.append(Z)
        spec = copy.deepcopy(spec0)
        for lay, Z, scale in ((spec["convs"][0], Zs[0], 1e-5), (spec["head"], Zs[1], 1.0)):
            lay["Z"] = Z
            if "Z0" in lay:
                lay["Z0"] = Z.copy()
            Lu = np.linalg.cholesky(rbf(Z, Z, lay["variance"], lay["ls"]) + JITTER * np.eye(M))
            lay["q_sqrt"] = np.tile(Lu[None], [lay["q_sqrt"].shape[0], 1, 1]) * scale
        spec["num_data"] = 512
        flat = imgs.reshape(512, -1)
        m = build_from_spec(spec, flat[:32], labels[:32])
        res["elbo_step0"] = float(m.compute_log_likelihood(flat[:32], labels[:32], seed=1))
        order = np.random.default_rng(9)
        for t in range(adam_steps):
            idx = order.choice(512, 32, replace=False)
            m.train_step(flat[idx], labels[idx], 1e-3, seed=1000 + t)
        res["elbo_after"] = float(m.compute_log_likelihood(flat[:32], labels[:32], seed=1))
        m.close()
        out[init] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--adam-steps", type=int, default=200)
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from deepcgp_amd import device as dev
    ctx = dev.get_context()
    out = {"rounds": a.rounds, "variance": VARIANCE}
    if not a.skip_timing:
        out["timing"] = timing(ctx, a.rounds)
    if not a.skip_quality:
        out["quality"] = quality(a.adam_steps)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""usage (GPU box): python tools/ard_time.py [--steps 100] [--rounds 5] [--iters 100] [--parent-tree DIR] [--sweeps-only] [--out profiles/ard_time.json]

What per-dimension (ARD) lengthscales on the conv layers cost on the device (csrc/rbf.hip: the patch sweep's ARD instance; csrc/grad.hip:
conv_backward on the scaled copies), on the model of tools/mixing_time.py: cfg2 C+H (28 x 28 x 1, conv f5 s2, head f5), batch 32, S = 10,
dedup_layer0 on, at M = 256 and at M = 384.  Three legs take the same steps:
  a_scalar_fused     scalar RBF on the route the library chooses (M = 256: the one-launch layer kernel; M = 384: sweep + GEMM)
  b_scalar_unfused   scalar RBF with the ctx option no_fused_layer: the sweep + GEMM route an ARD layer takes at every M
  c_ard              every conv layer RBF(L, ARD=True), the lengthscales spread 0.8 - 1.2 around the scalar
One warm-up leg of each, then ``--rounds`` rounds that visit the three in turn (alternating, one process), for the forward ELBO step and for the
training step; a leg is a host clock around ``--steps`` synchronous calls on device-resident batches.  Each leg reports the median of its
rounds and its spread ((max - min) / median).  ``c_minus_b_us`` is the ARD instance's own cost (the scaling sweep in place of the unit sweep,
and in a training step the scaled copies, dXs on the first layer and the chain rule through the scaling); ``b_minus_a_us`` is the price of the
route, which an ARD instance of the one-launch kernel would recover.

``--parent-tree DIR`` (a built checkout of the parent commit): leg (a) is also timed with the parent's library and Python, in a fresh child
process before and after this process's rounds (``parent_a``: both visits).

Then the sweep alone through the operator entries (event timers of the library, ``--iters`` calls): dcgp_kuf_patches_rbf_ard against
dcgp_kuf_patches_rbf (whose RBF sweep is the unit sweep of csrc/head_units.hip) on the 46080-column first layer and on a 5 x 5 x 10 layer,
with their share of the fp64 MFMA rate measured in the same run (dcgp_debug_mfma_f64_rate) on 2 Mp Kc Lp flops.

No figure is fixed in advance.  Prints one JSON line."""
import argparse
import copy
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, S, LR = 32, 10, 1e-4
LEGS = ("a_scalar_fused", "b_scalar_unfused", "c_ard")
CONFIGS = {"M256": 256, "M384": 384}      # cfg2_mnist_CH_M256 with this M
# (H, W, C, f, s, N, M): 320 x 144 = 46080 columns of 25-element patches; 320 x 64 = 20480 columns of 250-element patches
SWEEPS = {"first_layer_46080": (28, 28, 1, 5, 2, 320, 256), "patches_5x5x10": (12, 12, 10, 5, 1, 320, 256)}

CHILD = r"""
import json, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from deepcgp_amd import synthetic as syn
from deepcgp_amd.models import build_from_spec
steps, rounds, out = int(sys.argv[2]), int(sys.argv[3]), {}
for key, M in json.loads(sys.argv[4]).items():
    spec, X, Y = syn.make_config("cfg2_mnist_CH_M256", S=%d, M=M)
    m = build_from_spec(spec, X, Y)
    m.dedup_layer0 = True
    m._build()
    dX, dY = m._ctx.to_device(X), m._ctx.to_device(Y, np.int32)
    res = {}
    for what in ("forward", "train"):
        legs = []
        for k in range(rounds + 1):
            m._ctx.sync()
            t0 = time.perf_counter()
            for i in range(steps):
                m.train_step(dX, dY, %g, seed=1000 * k + i) if what == "train" else m.compute_log_likelihood(dX, dY, seed=1000 * k + i)
            if k:
                legs.append(1e3 * (time.perf_counter() - t0) / steps)
        res[what] = legs
    out[key] = res
    m.close()
print("CHILD " + json.dumps(out))
""" % (S, LR)


def parent_visit(tree, steps, rounds):
    """Leg (a) with the parent's library and Python, in a fresh child process (its own device context)."""
    tree = os.path.abspath(tree)
    env = dict(os.environ, PYTHONPATH=tree)
    env.pop("DCGP_LIB", None)
    r = subprocess.run([sys.executable, "-c", CHILD, tree, str(steps), str(rounds), json.dumps(CONFIGS)], cwd=tree, env=env, capture_output=True,
                       text=True, timeout=900)
    for line in r.stdout.splitlines():
        if line.startswith("CHILD "):
            return json.loads(line[6:])
    raise RuntimeError("parent leg failed: %s" % r.stderr[-2000:])


def ard_spec(spec, seed=11):
    spec = copy.deepcopy(spec)
    rng = np.random.default_rng(seed)
    for c in spec["convs"]:
        c["ls"] = float(c["ls"]) * (0.8 + 0.4 * rng.random(c["f"] * c["f"] * c["C"]))
    return spec


def summary(ts):
    ts = np.array(ts)
    return {"legs_ms": [float(t) for t in ts], "ms": float(np.median(ts)), "spread": float((ts.max() - ts.min()) / np.median(ts))}


def sweeps_alone(ctx, iters):
    from deepcgp_amd import device as dev
    from deepcgp_amd.kernels import RBF
    peak = C.c_double(0.0)
    ctx._check(dev.lib().dcgp_debug_mfma_f64_rate(ctx.handle, C.byref(peak)))
    out = {"mfma_f64_tflops_measured": peak.value}
    rng = np.random.default_rng(0)
    for name, (H, W, Cc, f, s, N, M) in SWEEPS.items():
        L, P = f * f * Cc, ((H - f) // s + 1) * ((W - f) // s + 1)
        Mp, Lp = (M + 15) // 16 * 16, (L + 3) // 4 * 4
        dX, dZ, o = ctx.to_device(rng.standard_normal((N, H, W, Cc))), ctx.to_device(rng.standard_normal((M, L))), ctx.empty((M, N * P))
        ls0 = 0.9 * np.sqrt(L)
        res = {"columns": N * P, "L": L, "M": M, "flops": 2.0 * Mp * N * P * Lp, "store_bytes": 8.0 * M * N * P}
        for leg, k in (("scalar", RBF(L, 1.7, ls0)), ("ard", RBF(L, 1.7, ls0 * (0.8 + 0.4 * rng.random(L)), ARD=True))):
            for it in range(3):
                k._kuf(ctx, dX, N, H, W, Cc, f, s, dZ, M, o, 1)
            ctx.timing_enable(1)
            ctx.timing_reset()
            for it in range(iters):
                k._kuf(ctx, dX, N, H, W, Cc, f, s, dZ, M, o, 1)
            t = {n: v for n, v in ctx.timing().items() if v[0] > 0 and n.startswith("kuf")}
            ctx.timing_enable(0)
            us = 1e3 * sum(v[1] for v in t.values()) / iters
            res[leg] = {"timers": {n: list(v) for n, v in t.items()}, "us": us, "tflops": res["flops"] / us * 1e-6,
                        "share_of_measured_mfma_rate": res["flops"] / us * 1e-6 / peak.value, "store_GBps": res["store_bytes"] / us * 1e-3}
        res["ard_over_scalar"] = res["ard"]["us"] / res["scalar"]["us"]
        out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--sweeps-only", action="store_true", help="the sweep kernels alone, no model legs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"batch": BATCH, "S": S, "dedup_layer0": True, "steps_per_leg": a.steps, "rounds": a.rounds, "configs": CONFIGS}
    if a.parent_tree and not a.sweeps_only:      # (before this process opens the device)
        out["parent_a"] = {"before": parent_visit(a.parent_tree, a.steps, a.rounds)}
    from deepcgp_amd import synthetic as syn
    from deepcgp_amd.models import build_from_spec
    ctx = None
    for key, M in ({} if a.sweeps_only else CONFIGS).items():
        spec, X, Y = syn.make_config("cfg2_mnist_CH_M256", S=S, M=M)
        models = {}
        for leg in LEGS:
            m = build_from_spec(ard_spec(spec) if leg == "c_ard" else copy.deepcopy(spec), X, Y)
            m.dedup_layer0 = True
            m._build()
            models[leg] = m
        ctx = models[LEGS[0]]._ctx
        dX, dY = ctx.to_device(X), ctx.to_device(Y, np.int32)

        def run(leg, train, seed0):
            m, last = models[leg], None
            ctx.set_option("no_fused_layer", 1 if leg == "b_scalar_unfused" else 0)
            ctx.sync()
            t0 = time.perf_counter()
            for i in range(a.steps):       # (every call ends in a device synchronisation)
                last = m.train_step(dX, dY, LR, seed=seed0 + i) if train else m.compute_log_likelihood(dX, dY, seed=seed0 + i)
            ctx.set_option("no_fused_layer", 0)
            return 1e3 * (time.perf_counter() - t0) / a.steps, last

        res_cfg = {}
        for what, train in (("forward", False), ("train", True)):
            legs, last = {leg: [] for leg in LEGS}, {}
            for k in range(a.rounds + 1):              # round 0: warm-up
                for leg in LEGS:
                    t, last[leg] = run(leg, train, 1000 * k)
                    if k:
                        legs[leg].append(t)
            res = {leg: dict(summary(legs[leg]), last_elbo=float(last[leg])) for leg in LEGS}
            A, B, Cc = (res[leg]["ms"] for leg in LEGS)
            res["c_minus_b_us"], res["b_minus_a_us"], res["c_over_a"] = float(1e3 * (Cc - B)), float(1e3 * (B - A)), float(Cc / A)
            res_cfg[what] = res
        out[key] = res_cfg
        for m in models.values():
            m.close()
    if ctx is None:
        from deepcgp_amd import device as dev
        ctx = dev.get_context()
    out["sweep_alone"] = sweeps_alone(ctx, a.iters)
    if a.parent_tree and not a.sweeps_only:
        out["parent_a"]["after"] = parent_visit(a.parent_tree, a.steps, a.rounds)
        for key in CONFIGS:
            for what in ("forward", "train"):
                ts = out["parent_a"]["before"][key][what] + out["parent_a"]["after"][key][what]
                out[key][what]["parent_a"] = summary(ts)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

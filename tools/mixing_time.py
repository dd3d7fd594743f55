#!/usr/bin/env python
"""usage (GPU box): python tools/mixing_time.py [--steps 200] [--rounds 5] [--iters 200] [--out profiles/mixing_time.json]

What a mixed conv layer costs and saves on the device (csrc/mix.hip), on the model of tools/conv_mean_time.py: cfg2_mnist_CH_M256 (28 x 28 x 1,
conv f5 s2, head f5, M = 256), batch 32, S = 10, dedup_layer0 on, ten maps.  Three models take the same steps:
  a_unmixed_R10   the conv layer holds 10 GPs and emits them
  b_mixed_3_10    3 latent GPs mixed into 10 maps (``mixing_matrix("random", 3, 10)``, trainable)
  c_unmixed_R3    3 GPs, 3 maps (the head reads 3 channels): the layer of (b) without its mixing
One warm-up leg of each, then ``--rounds`` rounds that visit the three in turn (alternating, one process), for the forward ELBO step and for the
training step; a leg is a host clock around ``--steps`` synchronous calls on device-resident batches.  Each variant reports the median of its legs
and its spread ((max - min) / median); ``a_over_b`` is what the mixing saves, ``b_minus_c_us`` what it costs itself (a head on 10 channels
instead of 3 included).  The layer kernel's work per launch is K M^2 (1 + R) + 2 M R K plus the sweep: at G = 3, R = 10 the two triangular
products drop to (1 + 3) / (1 + 10) = 0.36 of their flops (derived; the measured ratio of whole steps is set beside it).

Then the three kernels alone (dcgp_debug_mix_time: ``--iters`` launches between two events), each beside a copy kernel that moves the bytes the
kernel has to move, on the columns of that layer (32 x 10 x 144) and on a de-duplicated first layer's worth of a small batch (4608).

No figure is fixed in advance.  Prints one JSON line."""
import argparse
import copy
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepcgp_amd import device as dev                          # noqa: E402
from deepcgp_amd import synthetic as syn                       # noqa: E402
from deepcgp_amd.layers import mixing_matrix                   # noqa: E402
from deepcgp_amd.models import build_from_spec                 # noqa: E402

BATCH, S, LR, G = 32, 10, 1e-4, 3
VARIANTS = ("a_unmixed_R10", "b_mixed_3_10", "c_unmixed_R3")
KERNEL_COLUMNS = {"layer_tiled": BATCH * S * 144, "small": 4608}


def specs():
    base, X, Y = syn.make_config("cfg2_mnist_CH_M256", S=S)
    out = {VARIANTS[0]: base}
    for name in VARIANTS[1:]:
        spec = copy.deepcopy(base)
        c, h = spec["convs"][0], spec["head"]
        R = c["R"]
        c.update(R=G, q_mu=np.ascontiguousarray(np.asarray(c["q_mu"])[:, :G]), q_sqrt=np.ascontiguousarray(np.asarray(c["q_sqrt"])[:G]))
        if name == "b_mixed_3_10":
            c.update(mix_W=mixing_matrix("random", G, R, seed=0), mix_trainable=True)
        else:      # the head on the layer's 3 maps
            Z = np.asarray(h["Z"]).reshape(h["M"], h["f"], h["f"], h["C"])[..., :G]
            h.update(C=G, Z=np.ascontiguousarray(Z.reshape(h["M"], -1)))
        out[name] = spec
    return out, X, Y


def kernels_alone(ctx, iters):
    out = {}
    for name, Kc in KERNEL_COLUMNS.items():
        us = (C.c_double * 8)()
        ctx._check(dev.lib().dcgp_debug_mix_time(ctx.handle, G, 10, Kc, iters, us))
        out[name] = {"columns": Kc, "G": G, "R": 10,
                     "mix_forward_us": us[0], "forward_copy_same_bytes_us": us[1], "forward_bytes": 8 * 3 * (G + 10) * Kc,
                     "mix_backward_latent_us": us[2], "latent_copy_same_bytes_us": us[3], "latent_bytes": 8 * (G + 10) * Kc,
                     "mix_backward_w_us": us[4], "w_copy_same_bytes_us": us[5], "w_bytes": 8 * (G + 10) * Kc}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sp, X, Y = specs()
    models, feeds = {}, {}
    for name in VARIANTS:
        m = build_from_spec(sp[name], X, Y)
        m.dedup_layer0 = True
        m._build()
        models[name] = m
        feeds[name] = (m._ctx.to_device(X), m._ctx.to_device(Y, np.int32))
    ctx = models[VARIANTS[0]]._ctx

    def leg(name, train, seed0):
        m, (dX, dY) = models[name], feeds[name]
        last = None
        ctx.sync()
        t0 = time.perf_counter()
        for i in range(a.steps):       # (every call ends in a device synchronisation)
            last = m.train_step(dX, dY, LR, seed=seed0 + i) if train else m.compute_log_likelihood(dX, dY, seed=seed0 + i)
        return 1e3 * (time.perf_counter() - t0) / a.steps, last

    out = {"shape": "cfg2_mnist_CH_M256", "batch": BATCH, "S": S, "dedup_layer0": True, "steps_per_leg": a.steps, "rounds": a.rounds,
           "derived_triangular_flop_ratio": (1 + G) / (1 + 10)}
    for what, train in (("forward", False), ("train", True)):
        legs = {name: [] for name in VARIANTS}
        last = {}
        for k in range(a.rounds + 1):              # round 0: warm-up
            for name in VARIANTS:
                t, last[name] = leg(name, train, 1000 * k)
                if k:
                    legs[name].append(t)
        res = {}
        for name in VARIANTS:
            ts = np.array(legs[name])
            res[name] = {"legs_ms": legs[name], "ms": float(np.median(ts)), "spread": float((ts.max() - ts.min()) / np.median(ts)),
                         "last_elbo": float(last[name])}
        A, B, Cc = (res[n]["ms"] for n in VARIANTS)
        res["a_over_b"] = float(A / B)
        res["b_over_a"] = float(B / A)
        res["b_minus_c_us"] = float(1e3 * (B - Cc))
        out[what] = res
    out["kernels_alone"] = kernels_alone(ctx, a.iters)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for m in models.values():
        m.close()


if __name__ == "__main__":
    main()

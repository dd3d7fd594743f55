#!/usr/bin/env python
"""usage (GPU box): python tools/conv_mean_time.py [--steps 200] [--rounds 5] [--iters 200] [--out profiles/conv_mean_time.json]

What a linear convolutional mean function costs on the device (csrc/conv_mean.hip), at the headline shape: cfg2_mnist_CH_M256 (28 x 28 x 1,
conv f5 s2 R10, head f5, M = 256), batch 32, S = 10, dedup_layer0 on.  Four models with the SAME geometry and parameters take the same steps:
  none             no mean function
  conv2d           Conv2dMean, added inside the layer's own launch (the head's rows may ride that launch)
  centre0_frozen   LinearConv2dMean("centre0"), frozen: the layer launch, then conv_mean_add (no head rows ride)
  channels_train   LinearConv2dMean("channels"), trainable: conv_mean_add, and conv_mean_backward_filter in the training step
One warm-up leg of each, then ``--rounds`` rounds that visit the four in turn (alternating, one process), for the forward ELBO step and for the
training step; a leg is a host clock around ``--steps`` synchronous calls on device-resident batches.  Each variant reports the median of its
legs and its spread ((max - min) / median).  The conv layer is layer 0 and has no input gradient in a training step; conv_mean_backward_dx runs
in ``input_gradient`` and in deeper layers.

Then the three kernels alone (dcgp_debug_conv_mean_time: ``--iters`` launches between two events), each beside a copy kernel that moves the
bytes the kernel has to move, for the two layer shapes a deep MNIST stack has: the first layer above (de-duplicated: 32 images, 10 replicas of
the output) and a 14 x 14 x 10 layer with f5 s1 R10 on the tiled batch (320 images, L = 250).

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
from deepcgp_amd.mean_functions import conv_mean_filter        # noqa: E402
from deepcgp_amd.models import build_from_spec                 # noqa: E402

BATCH, S, LR = 32, 10, 1e-4
VARIANTS = ("none", "conv2d", "centre0_frozen", "channels_train")
# (H, W, C, f, stride, R, rows, rep)
KERNEL_SHAPES = {"layer0_dedup": (28, 28, 1, 5, 2, 10, BATCH, S), "deep_14x14x10": (14, 14, 10, 5, 1, 10, BATCH * S, 1)}


def specs():
    base, X, Y = syn.make_config("cfg2_mnist_CH_M256", S=S)
    out = {}
    for name in VARIANTS:
        spec = copy.deepcopy(base)
        c = spec["convs"][0]
        if name == "conv2d":
            c["mean_function"] = "conv2d"
        elif name != "none":
            kind = "centre0" if name == "centre0_frozen" else "channels"
            c["mean_filter"], c["mean_trainable"] = conv_mean_filter(kind, c["f"], c["C"], c["R"]), name == "channels_train"
        out[name] = spec
    return out, X, Y


def kernels_alone(ctx, iters):
    out = {}
    for name, (H, W, Cc, f, s, R, rows, rep) in KERNEL_SHAPES.items():
        us = (C.c_double * 8)()
        ctx._check(dev.lib().dcgp_debug_conv_mean_time(ctx.handle, H, W, Cc, f, s, R, rows, rep, iters, us))
        P, L = ((H - f) // s + 1) * ((W - f) // s + 1), f * f * Cc
        Kc = rows * P
        out[name] = {
            "shape": dict(H=H, W=W, C=Cc, f=f, stride=s, R=R, rows=rows, rep=rep, columns=Kc, L=L),
            "conv_mean_add_us": us[0], "copy_same_bytes_us": us[1], "add_bytes": 16 * rep * Kc * R, "add_flops": 2 * Kc * L * R,
            "conv_mean_backward_dx_us": us[2], "dx_copy_same_bytes_us": us[3], "dx_bytes": 8 * (Kc * R + 2 * rows * H * W * Cc),
            "conv_mean_backward_filter_us": us[4], "filter_copy_same_bytes_us": us[5], "filter_bytes": 8 * Kc * (L + R), "filter_flops": 2 * Kc * L * R,
        }
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
    ctx = models["none"]._ctx

    def leg(name, train, seed0):
        m, (dX, dY) = models[name], feeds[name]
        last = None
        ctx.sync()
        t0 = time.perf_counter()
        for i in range(a.steps):       # (every call ends in a device synchronisation)
            last = m.train_step(dX, dY, LR, seed=seed0 + i) if train else m.compute_log_likelihood(dX, dY, seed=seed0 + i)
        return 1e3 * (time.perf_counter() - t0) / a.steps, last

    out = {"shape": "cfg2_mnist_CH_M256", "batch": BATCH, "S": S, "dedup_layer0": True, "steps_per_leg": a.steps, "rounds": a.rounds}
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
        for name in VARIANTS[1:]:
            res[name]["over_none_us"] = float(1e3 * (res[name]["ms"] - res["none"]["ms"]))
        res["centre0_frozen"]["over_conv2d_us"] = float(1e3 * (res["centre0_frozen"]["ms"] - res["conv2d"]["ms"]))
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

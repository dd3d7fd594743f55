#!/usr/bin/env python
"""usage (GPU box): python tools/dilation_time.py [--steps 300] [--pairs 5] [--iters 200] [--out profiles/dilation_time.json]

What dilation on the device costs.  A dilated layer is an ordinary layer on the d^2 phase sub-images of its input (csrc/dilate.hip), so the cost
is the relayout: space-to-batch of the input (and of explicit noise), batch-to-space of the outputs; in a training step also space-to-batch of
the gradient arriving from above.

(1) A cfg2-like model at batch 32, S = 10, dedup_layer0 on, whose first layer is f5 s1 d2 on 28 x 28 (20 x 20 = 400 patches a row).  Two models
with the same parameters take the same steps, leg by leg:
  (a) dilated:  fed the 28 x 28 images -- the device splits them and merges the layer's outputs;
  (b) physical: the same layer undilated on 14 x 14, fed the N * 4 host-split images (100 patches each: the same patch columns).  Its head sees
      N * 4 * S rows of 10 x 10 x R (36 patches) instead of N * S rows of 20 x 20 x R (256 patches), so the two models differ behind layer 0 as
      well: (a) - (b) is the relayout PLUS the heavier head;
  (c) undilated: the same layer and parameters undilated on 24 x 24 crops of the images: 20 x 20 = 400 patches a row as in (a), the same patch
      columns in the layer kernel, and the very same head.  (a) - (c) is the relayout (and 14 x 14 strips in place of 24 x 24 ones).
One warm-up leg of each, then ``--pairs`` alternating (a, b, c) rounds in this one process, for the forward ELBO step and for the training step; a
leg is a host clock around ``--steps`` synchronous calls.  Both read their batch from device arrays: no upload is timed.

(2) Each relayout kernel alone on that layer's buffers (dcgp_debug_dilate_time: ``--iters`` launches between two events), beside the same
relayout walking its source instead of its destination and beside a copy kernel of the same traffic: the input batch (32 x 28 x 28 x 1) and the
output batch (320 x 20 x 20 x R).

(3) The same for a 17 x 17 d3 layer, where phantoms exist (d^2 P' / P = 1.19).

Prints one JSON line: the rounds in ms per step, their medians, the spread of each side's own repeats ((max - min) / median), and the kernels'
microseconds per launch."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepcgp_amd import device as dev                       # noqa: E402
from deepcgp_amd import synthetic as syn                    # noqa: E402
from deepcgp_amd.models import build_from_spec              # noqa: E402

HWC, F, R, D, HEAD, M, BATCH, S, LR = (28, 28, 1), 5, 10, 2, (5, 1), 256, 32, 10, 1e-4


def specs():
    """(dilated: 28 x 28 f5 d2 -> 20 x 20 x R -> head; physical: the same layer on 14 x 14 -> 10 x 10 x R -> a head of its own)."""
    H, W, Cc = HWC
    Hs, Ws = -(-H // D), -(-W // D)
    physical = syn.make_spec((Hs, Ws, Cc), [(F, 1, R)], HEAD, M, S=S, num_data=60000, seed=1235, conv_q_sqrt_scale=0.1)
    Ho, Wo = H - D * (F - 1), W - D * (F - 1)
    dilated = syn.make_spec((Ho, Wo, R), [], HEAD, M, S=S, num_data=60000, seed=1236)
    conv = dict(physical["convs"][0])
    conv.update(H=H, W=W, dil=D)
    dilated["convs"] = [conv]
    undilated = {k: v for k, v in dilated.items()}
    conv = dict(conv)
    conv.pop("dil")
    conv.update(H=Ho + F - 1, W=Wo + F - 1)
    undilated["convs"] = [conv]
    return dilated, physical, undilated


def split(X, H, W, Cc, d):
    x = X.reshape(-1, H, W, Cc)
    Hs, Ws = -(-H // d), -(-W // d)
    out = np.zeros((x.shape[0], d, d, Hs, Ws, Cc))
    for a in range(d):
        for b in range(d):
            t = x[:, a::d, b::d]
            out[:, a, b, :t.shape[1], :t.shape[2]] = t
    return np.ascontiguousarray(out.reshape(x.shape[0] * d * d, -1))


def kernels(ctx, rows, H, W, Cc, d, iters):
    us = (C.c_double * 8)()
    ctx._check(dev.lib().dcgp_debug_dilate_time(ctx.handle, rows, H, W, Cc, d, iters, us))
    names = ("s2b_us", "s2b_from_image_side_us", "copy_phase_batch_us", "b2s_us", "b2s_from_phase_side_us", "copy_image_batch_us")
    out = {k: float(v) for k, v in zip(names, us)}
    out.update(rows=rows, H=H, W=W, C=Cc, d=d, image_bytes=8 * rows * H * W * Cc, phase_bytes=8 * rows * d * d * -(-H // d) * -(-W // d) * Cc)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dilation_time.json"))
    a = ap.parse_args()
    dilated, physical, undilated = specs()
    H, W, Cc = HWC
    X, Y = syn.make_batch(HWC, BATCH, seed=1235)
    Xs = split(X, H, W, Cc, D)
    Ys = np.repeat(np.asarray(Y).reshape(-1), D * D).astype(np.int32)
    Hc = H - (D - 1) * (F - 1)      # 24: the undilated window gives the dilated layer's 20 x 20
    Xc = np.ascontiguousarray(X.reshape(BATCH, H, W, Cc)[:, :Hc, :Hc]).reshape(BATCH, -1)
    models = {"dilated": build_from_spec(dilated, X, Y), "physical": build_from_spec(physical, Xs, Ys), "undilated": build_from_spec(undilated, Xc, Y)}
    data = {"dilated": (X, Y), "physical": (Xs, Ys), "undilated": (Xc, Y)}
    feeds = {}
    for name, m in models.items():
        m.dedup_layer0 = True
        m._build()
        feeds[name] = (m._ctx.to_device(data[name][0]), m._ctx.to_device(data[name][1], np.int32))

    def leg(name, train, seed0):
        m, (dX, dY) = models[name], feeds[name]
        m._ctx.sync()
        t0 = time.perf_counter()
        for i in range(a.steps):       # (every call ends in a device synchronisation)
            if train:
                m.train_step(dX, dY, LR, seed=seed0 + i)
            else:
                m.compute_log_likelihood(dX, dY, seed=seed0 + i)
        return 1e3 * (time.perf_counter() - t0) / a.steps

    out = {"shape": "28 x 28 x 1 -> conv f5 s1 d2 R10 M256 (400 patches a row) -> head f5 M256", "batch": BATCH, "S": S, "dedup_layer0": True,
           "dilation": D, "steps_per_leg": a.steps}
    for what, train in (("forward", False), ("train", True)):
        pairs = []
        for k in range(a.pairs + 1):               # leg 0 of each: warm-up
            ts = [leg(name, train, 1000 * k) for name in ("dilated", "physical", "undilated")]
            if k:
                pairs.append(ts)
        pa = np.array(pairs)
        med = np.median(pa, axis=0)
        spread = (pa.max(axis=0) - pa.min(axis=0)) / med
        out[what] = {"rounds_ms": pairs, "dilated_ms": float(med[0]), "physical_ms": float(med[1]), "undilated_ms": float(med[2]),
                     "dilated_minus_physical_us": float(1e3 * (med[0] - med[1])), "dilated_minus_undilated_us": float(1e3 * (med[0] - med[2])),
                     "dilated_spread": float(spread[0]), "physical_spread": float(spread[1]), "undilated_spread": float(spread[2])}
    ctx = models["dilated"]._ctx
    Ho, Wo = H - D * (F - 1), W - D * (F - 1)
    out["kernels_28x28_d2"] = {"input": kernels(ctx, BATCH, H, W, Cc, D, a.iters), "output": kernels(ctx, BATCH * S, Ho, Wo, R, D, a.iters)}
    out["kernels_17x17_d3"] = {"input": kernels(ctx, BATCH, 17, 17, 1, 3, a.iters), "output": kernels(ctx, BATCH * S, 11, 11, R, 3, a.iters),
                               "phantom_ratio": 9 * 4 * 4 / (11 * 11)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for m in models.values():
        m.close()


if __name__ == "__main__":
    main()

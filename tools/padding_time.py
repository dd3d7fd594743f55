#!/usr/bin/env python
"""usage (GPU box): python tools/padding_time.py [--steps 300] [--pairs 5] [--out profiles/padding_time.json]

What zero padding on the device costs, at the headline shape (cfg2_mnist_CH_M256's layers, batch 32, S = 10, dedup_layer0 on).  Two models
with the SAME layer geometry and parameters take the same steps, leg by leg:
  (a) padded: the conv layer padded by 2 (28 x 28 images, a 32 x 32 window), fed the 28 x 28 images -- the device pads them (csrc/pad.hip);
  (b) valid:  the conv layer added as a VALID 32 x 32 layer, fed images the host padded beforehand.
Every other kernel of the two is identical, so the difference is the pad launch (and, in a training step, nothing else: layer 0 has no input
gradient).  Both read their batch from device arrays: no upload is timed.  One warm-up leg of each, then ``--pairs`` alternating (a, b) pairs
in this one process, for the forward ELBO step and for the training step; a leg is a host clock around ``--steps`` synchronous calls.
Then (c), alone: the same stack with EVERY layer padded (conv by 2, head by 2: 14 x 14 x 10 -> 18 x 18 x 10), whose training step also crops
the head's input gradient.

Expectation, stated beside the measurement (not a bar): a padded layer moves rows x (H + 2p)(W + 2p) C doubles per pass (one write, at most
one read of the same size) -- at this shape 0.26 MB for layer 0 and 8.3 MB for the head, microseconds at HBM rates -- so the cost should be
the launch itself, about 2 us per padded layer per pass behind a streaming kernel.

Prints one JSON line: the pairs in ms per step, their medians, the spread of each side's own repeats ((max - min) / median), the difference
of the medians, the bytes the expectation counts, and whether (a) and (b) returned the same ELBO to the bit."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepcgp_amd import synthetic as syn                    # noqa: E402
from deepcgp_amd.models import build_from_spec              # noqa: E402

HWC, CONV, HEAD, M, BATCH, S, LR, PAD = (28, 28, 1), (5, 2, 10), (5, 1), 256, 32, 10, 1e-4, 2


def specs():
    """(padded at layer 0, the same layers VALID on 32 x 32, every layer padded)."""
    H, W, C = HWC
    valid = syn.make_spec((H + 2 * PAD, W + 2 * PAD, C), [CONV], HEAD, M, S=S, num_data=60000, seed=1235, conv_q_sqrt_scale=0.1)
    padded = copy.deepcopy(valid)
    padded["convs"][0].update(H=H, W=W, pad=PAD)
    h = valid["head"]
    full = syn.make_spec((H + 2 * PAD, W + 2 * PAD, C), [CONV], HEAD, M, S=S, num_data=60000, seed=1235, conv_q_sqrt_scale=0.1)
    full["convs"][0].update(H=H, W=W, pad=PAD)
    hp = syn.make_spec((h["H"] + 2 * PAD, h["W"] + 2 * PAD, h["C"]), [], HEAD, M, S=S, num_data=60000, seed=1236)["head"]
    hp.update(H=h["H"], W=h["W"], pad=PAD)
    full["head"] = hp
    return padded, valid, full


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    padded, valid, full = specs()
    H, W, C = HWC
    X, Y = syn.make_batch(HWC, BATCH, seed=1235)
    Xp = np.ascontiguousarray(np.pad(X.reshape(BATCH, H, W, C), ((0, 0), (PAD, PAD), (PAD, PAD), (0, 0)))).reshape(BATCH, -1)
    models = {"padded": build_from_spec(padded, X, Y), "valid": build_from_spec(valid, Xp, Y), "all_padded": build_from_spec(full, X, Y)}
    feeds = {}
    for name, m in models.items():
        m.dedup_layer0 = True
        m._build()
        feeds[name] = (m._ctx.to_device(Xp if name == "valid" else X), m._ctx.to_device(Y, np.int32))

    def leg(name, train, seed0):
        m, (dX, dY) = models[name], feeds[name]
        last = None
        m._ctx.sync()
        t0 = time.perf_counter()
        for i in range(a.steps):       # (every call ends in a device synchronisation)
            last = m.train_step(dX, dY, LR, seed=seed0 + i) if train else m.compute_log_likelihood(dX, dY, seed=seed0 + i)
        return 1e3 * (time.perf_counter() - t0) / a.steps, last

    out = {"shape": "cfg2_mnist_CH_M256 layers", "batch": BATCH, "S": S, "dedup_layer0": True, "pad": PAD, "steps_per_leg": a.steps}
    identical = True
    for what, train in (("forward", False), ("train", True)):
        pairs = []
        for k in range(a.pairs + 1):               # leg 0 of each: warm-up
            ta, ea = leg("padded", train, 1000 * k)
            tb, eb = leg("valid", train, 1000 * k)
            identical = identical and ea == eb
            if k:
                pairs.append([ta, tb])
        pa = np.array(pairs)
        med = np.median(pa, axis=0)
        out[what] = {"pairs_ms": pairs, "padded_ms": float(med[0]), "valid_ms": float(med[1]), "difference_us": float(1e3 * (med[0] - med[1])),
                     "padded_spread": float((pa[:, 0].max() - pa[:, 0].min()) / med[0]), "valid_spread": float((pa[:, 1].max() - pa[:, 1].min()) / med[1])}
    for what, train in (("forward", False), ("train", True)):
        ts = [leg("all_padded", train, 1000 * k)[0] for k in range(a.pairs + 1)][1:]
        out["all_padded_" + what] = {"legs_ms": ts, "ms": float(np.median(ts)), "spread": float((max(ts) - min(ts)) / np.median(ts))}
    h = valid["head"]
    out["expected_bytes_per_pass"] = {"layer0": 8 * BATCH * (H + 2 * PAD) * (W + 2 * PAD) * C,
                                      "head": 8 * BATCH * S * (h["H"] + 2 * PAD) * (h["W"] + 2 * PAD) * h["C"]}
    out["expected"] = "the pad / crop launches, about 2 us per padded layer per pass; the bytes are microseconds at HBM rates"
    out["last_elbo_identical"] = bool(identical)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for m in models.values():
        m.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""usage (GPU box): python tools/tta_time.py [--n 10000] [--S 5] [--batch 32] [--reps 5] [--shift 2] [--out profiles/tta_time.json]

What test-time augmentation costs on the device and what it cost before, at tools/eval_time.py's configuration: cfg2_mnist_CH_M256 (28 x 28 x 1
images, conv layer 5 x 5 / 2 with 10 maps, ConvKernel head 5 x 5 / 1, M = 256), 10 000 synthetic images, S = 5, batches of 32; the cross pattern
at shift 2 with the flip, V = 10 views.  Three legs on one model:
  (tta)   ``evaluate(views=V)``: one call, the views formed on the device per batch;
  (host)  what a user had to do before: per view ``augment.apply`` on the host and one ``evaluate(per_image=True)`` over the set, the V ``p_mean``
          tables averaged on the host.  Timing only: its noise and its log density differ from (tta)'s by construction;
  (plain) one ``evaluate`` without views, the floor of a single view.
One untimed (tta, host, plain) triple, then ``--reps`` timed triples in alternating order in this one process; each leg is a host clock around
work that ends in a device synchronisation.  Prints one JSON line (and writes it to --out): the triples in ms, the medians, each leg's spread
((max - min) / median), (tta) against (host) and against V x (plain), and the two accuracies."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepcgp_amd import augment, synthetic as syn, device as dev      # noqa: E402
from deepcgp_amd.models import build_from_spec                        # noqa: E402

CONFIG = "cfg2_mnist_CH_M256"


def spread(v):
    return float((np.max(v) - np.min(v)) / np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--S", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shift", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_time.json"))
    a = ap.parse_args()
    cfg = syn.CONFIGS[CONFIG]
    hwc = tuple(cfg["hwc"])
    spec = syn.make_spec(cfg["hwc"], cfg["convs"], cfg["head"], cfg["M"], S=a.S, num_data=cfg["num_data"], seed=1)
    X, Y = syn.make_batch(cfg["hwc"], a.n, seed=2)
    model = build_from_spec(spec, X[:cfg["batch"]], Y[:cfg["batch"]])
    ctx = dev.get_context()
    views = augment.views(a.shift, True, "cross")
    V = len(views)

    def clocked(fn):
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        return 1e3 * (time.perf_counter() - t0), out

    def tta():
        return model.evaluate(X, Y, S=a.S, batch_size=a.batch, seed=0, views=views)

    def host():
        X4 = X.reshape((a.n,) + hwc)
        acc = np.zeros((a.n, 10))
        for dy, dx, f in views:
            Xv = augment.apply(X4, int(dy), int(dx), int(f)).reshape(a.n, -1)
            acc += model.evaluate(Xv, Y, S=a.S, batch_size=a.batch, seed=0, per_image=True)["p_mean"]
        return {"accuracy": float(np.mean((acc / V).argmax(axis=1) == Y))}

    def plain():
        return model.evaluate(X, Y, S=a.S, batch_size=a.batch, seed=0)

    triples, outs = [], None
    for k in range(a.reps + 1):                      # triple 0: workspaces, the parameter-only chain
        (ta, ra), (tb, rb), (tc, rc) = clocked(tta), clocked(host), clocked(plain)
        outs = (ra, rb, rc)
        if k:
            triples.append([ta, tb, tc])
    t = np.array(triples)
    med = [float(np.median(t[:, j])) for j in range(3)]
    res = {"tool": "tta_time", "config": CONFIG, "n": a.n, "S": a.S, "batch": a.batch, "reps": a.reps, "pattern": "cross", "shift": a.shift,
           "hflip": True, "views": V, "triples_ms": [[round(x, 3) for x in row] for row in triples],
           "tta_ms": round(med[0], 3), "host_loop_ms": round(med[1], 3), "plain_ms": round(med[2], 3),
           "tta_spread": round(spread(t[:, 0]), 4), "host_loop_spread": round(spread(t[:, 1]), 4), "plain_spread": round(spread(t[:, 2]), 4),
           "host_loop_over_tta": round(med[1] / med[0], 3), "tta_over_V_plain": round(med[0] / (V * med[2]), 3),
           "tta_view_images_per_s": round(1e3 * V * a.n / med[0], 1),
           "accuracy_tta": outs[0]["accuracy"], "accuracy_host_loop": outs[1]["accuracy"], "accuracy_plain": outs[2]["accuracy"]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    model.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""usage (GPU box): python tools/train_run_time.py [--steps 2000] [--pairs 5] [--pool 60000] [--out profiles/train_run_time.json]

What a training run on the device (DGP_Base.train_run, dcgp_model_train_run_adam) gains over the per-step loop it replaced, at the headline
configuration: cfg2_mnist_CH_M256, batch 32, S = 10, dedup_layer0 on, a synthetic pool of 60 000 images.  Two models built from one spec take
the same steps, leg by leg:
  (a) loop: per step a host draw, the host gather X[idx], its upload and one ``train_step`` -- the Adam branch models.train had;
  (b) run:  the same index table through one ``train_run`` on the resident set (the upload is timed once, apart).
One warm-up leg of each, then ``--pairs`` alternating (a, b) pairs in this one process; each leg is a host clock around work that ends in a
device synchronisation.  Prints one JSON line: the pairs in steps / s, their medians, the spread of (a)'s own repeats ((max - min) / median),
the upload time, and whether the two models' ELBO histories were equal to the bit in every leg."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepcgp_amd import synthetic as syn                    # noqa: E402
from deepcgp_amd.models import build_from_spec, index_table  # noqa: E402

CONFIG, BATCH, S, LR = "cfg2_mnist_CH_M256", 32, 10, 1e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--pool", type=int, default=60000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = syn.CONFIGS[CONFIG]
    spec = syn.make_spec(cfg["hwc"], cfg["convs"], cfg["head"], cfg["M"], S=S, num_data=a.pool, seed=1235, conv_q_sqrt_scale=0.1)
    X, Y = syn.make_batch(cfg["hwc"], a.pool, seed=1235)
    loop_m, run_m = build_from_spec(spec, X, Y), build_from_spec(spec, X, Y)
    for m in (loop_m, run_m):
        m.dedup_layer0 = True
        m._build()
    t0 = time.perf_counter()
    run_m.attach_dataset()
    run_m._ctx.sync()
    upload_s = time.perf_counter() - t0
    pairs, identical, seed = [], True, 0

    def loop_leg(seed0):
        r = np.random.default_rng(seed0)
        hist = np.empty(a.steps)
        t0 = time.perf_counter()
        for i in range(a.steps):
            idx = r.choice(a.pool, size=BATCH, replace=False)
            hist[i] = loop_m.train_step(loop_m.X[idx], loop_m.Y[idx], LR, seed=seed0 + i)
        return hist, a.steps / (time.perf_counter() - t0)

    def run_leg(seed0):
        t0 = time.perf_counter()
        idx = index_table(np.random.default_rng(seed0), a.pool, BATCH, a.steps)      # the draws are part of the leg, as in (a)
        hist = run_m.train_run(idx, LR, seed=seed0)
        return hist, a.steps / (time.perf_counter() - t0)

    for k in range(a.pairs + 1):                  # leg 0 of each: warm-up
        seed = k * a.steps
        ha, ra = loop_leg(seed)
        hb, rb = run_leg(seed)
        identical = identical and bool(np.array_equal(ha, hb))
        if k:
            pairs.append([ra, rb])
    pa = np.array(pairs)
    out = {"config": CONFIG, "batch": BATCH, "S": S, "dedup_layer0": True, "pool": a.pool, "steps_per_leg": a.steps, "pairs_steps_per_s": pairs,
           "loop_steps_per_s": float(np.median(pa[:, 0])), "run_steps_per_s": float(np.median(pa[:, 1])),
           "loop_spread": float((pa[:, 0].max() - pa[:, 0].min()) / np.median(pa[:, 0])),
           "run_spread": float((pa[:, 1].max() - pa[:, 1].min()) / np.median(pa[:, 1])),
           "upload_s": upload_s, "histories_identical": identical}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    loop_m.close(), run_m.close()


if __name__ == "__main__":
    main()

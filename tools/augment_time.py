#!/usr/bin/env python
"""usage (GPU box): python tools/augment_time.py [--steps 2000] [--pairs 5] [--pool 60000] [--parent-tree DIR] [--out profiles/augment_time.json]

What augmenting on the device costs and what it saves, at tools/train_run_time.py's configuration: cfg2_mnist_CH_M256, batch 32, S = 10,
dedup_layer0 on, a synthetic pool of 60 000 images; max_shift 4 with the flip on.  Three models built from one spec take the same steps, leg
by leg:
  (aug)   ``train_run`` with the augmentation set: the augmenting gather writes each step's batch;
  (plain) ``train_run`` without one, on the same tree: the plain gather;
  (loop)  what a user had to do before: per step a host draw, the host gather X[idx], ``augment.apply`` on the host with the same draws, the
          upload and one ``train_step``.
One warm-up leg of each, then ``--pairs`` alternating (aug, plain, loop) triples in this one process; each leg is a host clock around work
that ends in a device synchronisation.  ``--parent-tree DIR`` (a built checkout of the parent commit): its plain ``train_run`` rate, by the
same leg in a child process that imports the package from DIR, run in this invocation before the triples.  Prints one JSON line: the triples
in steps / s, the medians, each side's spread ((max - min) / median), the difference of (aug) to (plain) as a share of (plain), and whether
the (aug) and (loop) ELBO histories were equal to the bit in every leg."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

CONFIG, BATCH, S, LR = "cfg2_mnist_CH_M256", 32, 10, 1e-4
SHIFT, FLIP = 4, True


def spread(v):
    return float((np.max(v) - np.min(v)) / np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--pool", type=int, default=60000)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--plain-only-from", default=None, help="(the child of --parent-tree) import the package from this tree, time the plain run alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tree = a.plain_only_from or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    from deepcgp_amd import synthetic as syn
    from deepcgp_amd.models import build_from_spec, index_table

    cfg = syn.CONFIGS[CONFIG]
    spec = syn.make_spec(cfg["hwc"], cfg["convs"], cfg["head"], cfg["M"], S=S, num_data=a.pool, seed=1235, conv_q_sqrt_scale=0.1)
    X, Y = syn.make_batch(cfg["hwc"], a.pool, seed=1235)
    hwc = tuple(cfg["hwc"])

    def model(resident):
        m = build_from_spec(spec, X, Y)
        m.dedup_layer0 = True
        m._build()
        if resident:
            m.attach_dataset()
        return m

    def run_leg(m, seed0):
        t0 = time.perf_counter()
        idx = index_table(np.random.default_rng(seed0), a.pool, BATCH, a.steps)      # the draws are part of the leg, as in the loop
        hist = m.train_run(idx, LR, seed=seed0)
        return hist, a.steps / (time.perf_counter() - t0)

    if a.plain_only_from:
        m = model(True)
        rates = [run_leg(m, k * a.steps)[1] for k in range(a.pairs + 1)][1:]
        print(json.dumps({"plain_steps_per_s": float(np.median(rates)), "plain_spread": spread(rates), "legs": rates}))
        m.close()
        return

    parent = None
    if a.parent_tree:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only-from", os.path.abspath(a.parent_tree), "--steps", str(a.steps),
                            "--pairs", str(a.pairs), "--pool", str(a.pool)], capture_output=True, text=True, check=True)
        parent = json.loads(r.stdout.strip().splitlines()[-1])

    from deepcgp_amd import augment
    aug = augment.Augmentation(SHIFT, FLIP)
    aug_m, plain_m, loop_m = model(True), model(True), model(False)
    aug_m.set_augmentation(aug)

    def loop_leg(seed0):
        r = np.random.default_rng(seed0)
        hist = np.empty(a.steps)
        t0 = time.perf_counter()
        for i in range(a.steps):
            idx = r.choice(a.pool, size=BATCH, replace=False)
            Xb = augment.apply(loop_m.X[idx].reshape((BATCH,) + hwc), *augment.draw(seed0 + i, BATCH, SHIFT, FLIP)).reshape(BATCH, -1)
            hist[i] = loop_m.train_step(Xb, loop_m.Y[idx], LR, seed=seed0 + i)
        return hist, a.steps / (time.perf_counter() - t0)

    triples, identical = [], True
    for k in range(a.pairs + 1):                  # leg 0 of each: warm-up
        seed = k * a.steps
        ha, ra = run_leg(aug_m, seed)
        _, rp = run_leg(plain_m, seed)
        hl, rl = loop_leg(seed)
        identical = identical and bool(np.array_equal(ha, hl))
        if k:
            triples.append([ra, rp, rl])
    t = np.array(triples)
    med = [float(np.median(t[:, j])) for j in range(3)]
    out = {"config": CONFIG, "batch": BATCH, "S": S, "dedup_layer0": True, "pool": a.pool, "steps_per_leg": a.steps, "max_shift": SHIFT, "hflip": FLIP,
           "triples_steps_per_s": triples, "aug_steps_per_s": med[0], "plain_steps_per_s": med[1], "host_augmented_loop_steps_per_s": med[2],
           "aug_spread": spread(t[:, 0]), "plain_spread": spread(t[:, 1]), "loop_spread": spread(t[:, 2]),
           "aug_vs_plain": (med[0] - med[1]) / med[1], "aug_vs_loop": (med[0] - med[2]) / med[2],
           "paired_aug_vs_plain": [float(x) for x in (t[:, 0] - t[:, 1]) / t[:, 1]],
           "aug_and_loop_histories_identical": identical, "parent": parent}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for m in (aug_m, plain_m, loop_m):
        m.close()


if __name__ == "__main__":
    main()

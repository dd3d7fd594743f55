#!/usr/bin/env python
"""usage (GPU box): python tools/clip_time.py [--steps 2000] [--rounds 5] [--pool 60000] [--parent-tree DIR] [--out profiles/clip_time.json]

What clipping by global norm costs a training step, at tools/train_run_time.py's configuration: cfg2_mnist_CH_M256, batch 32, S = 10,
dedup_layer0 on, a synthetic pool of 60 000 images.  Three models built from one spec take ``train_run`` legs of ``--steps`` steps:
  (off)    clipping off: the step as it always was;
  (inf)    ``set_grad_clip(inf)``: the norm is formed (two small launches), the scale is 1;
  (finite) ``set_grad_clip(half the smallest norm the warm-up leg saw)``: every step is scaled.
One warm-up leg of each, then ``--rounds`` alternating (off, inf, finite) rounds in this one process; each leg is a host clock around work
that ends in a device synchronisation.  ``--parent-tree DIR`` (a built checkout of the parent commit): its ``train_run`` rate, by the (off)
leg in a child process that imports the package from DIR, run in this invocation before the rounds.  Then the kernels alone, from the
library's own event timers (dcgp_timing_*) over one leg of per-step calls each: ``opt_step`` (the update), ``opt_norm`` (both norm launches)
and ``opt_step_clip`` (the update that reads the scale).  Prints one JSON line: the rounds in steps / s, the medians, each leg's spread
((max - min) / median), the legs' differences to (off) as a share of (off), the kernel averages in microseconds, and the parent's figures."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

CONFIG, BATCH, S, LR = "cfg2_mnist_CH_M256", 32, 10, 1e-4


def spread(v):
    return float((np.max(v) - np.min(v)) / np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pool", type=int, default=60000)
    ap.add_argument("--timed-steps", type=int, default=200, help="steps of the kernel-timer legs")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--off-only-from", default=None, help="(the child of --parent-tree) import the package from this tree, time the (off) leg alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tree = a.off_only_from or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    from deepcgp_amd import synthetic as syn
    from deepcgp_amd.models import build_from_spec, index_table

    cfg = syn.CONFIGS[CONFIG]
    spec = syn.make_spec(cfg["hwc"], cfg["convs"], cfg["head"], cfg["M"], S=S, num_data=a.pool, seed=1235, conv_q_sqrt_scale=0.1)
    X, Y = syn.make_batch(cfg["hwc"], a.pool, seed=1235)

    def model():
        m = build_from_spec(spec, X, Y)
        m.dedup_layer0 = True
        m._build()
        m.attach_dataset()
        return m

    def run_leg(m, seed0, steps=None):
        steps = steps or a.steps
        t0 = time.perf_counter()
        idx = index_table(np.random.default_rng(seed0), a.pool, BATCH, steps)
        hist = m.train_run(idx, LR, seed=seed0)
        return hist, steps / (time.perf_counter() - t0)

    if a.off_only_from:
        m = model()
        rates = [run_leg(m, k * a.steps)[1] for k in range(a.rounds + 1)][1:]
        print(json.dumps({"off_steps_per_s": float(np.median(rates)), "off_spread": spread(rates), "legs": rates}))
        m.close()
        return

    parent = None
    if a.parent_tree:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--off-only-from", os.path.abspath(a.parent_tree), "--steps", str(a.steps),
                            "--rounds", str(a.rounds), "--pool", str(a.pool)], capture_output=True, text=True, check=True)
        parent = json.loads(r.stdout.strip().splitlines()[-1])

    off_m, inf_m, fin_m = model(), model(), model()
    inf_m.set_grad_clip(np.inf)
    rounds, identical, max_norm, clipped = [], True, None, 0
    for k in range(a.rounds + 1):                 # round 0: warm-up, and the norms the finite leg's bound comes from
        seed = k * a.steps
        ho, ro = run_leg(off_m, seed)
        hi, ri = run_leg(inf_m, seed)
        identical = identical and bool(np.array_equal(ho, hi))      # scale 1: the same run
        if max_norm is None:
            max_norm = 0.5 * float(np.min(inf_m.last_grad_norms))
            fin_m.set_grad_clip(max_norm)
        _, rf = run_leg(fin_m, seed)
        clipped += int(np.sum(fin_m.last_grad_norms > max_norm))
        if k:
            rounds.append([ro, ri, rf])
    t = np.array(rounds)
    med = [float(np.median(t[:, j])) for j in range(3)]

    # the kernels alone: the library's event timers around every launch of a leg
    kern = {}
    ctx = off_m._ctx
    for name, m in (("off", off_m), ("finite", fin_m)):
        ctx.timing_enable(1)
        ctx.timing_reset()
        run_leg(m, 10 ** 6, a.timed_steps)
        tim = ctx.timing()
        ctx.timing_enable(0)
        for fam in ("opt_step", "opt_norm", "opt_step_clip"):
            if fam in tim and tim[fam][0]:
                kern[fam] = {"launches": int(tim[fam][0]), "avg_us": 1e3 * tim[fam][1] / tim[fam][0]}
    out = {"config": CONFIG, "batch": BATCH, "S": S, "dedup_layer0": True, "pool": a.pool, "steps_per_leg": a.steps,
           "rounds_steps_per_s": rounds, "off_steps_per_s": med[0], "inf_steps_per_s": med[1], "finite_steps_per_s": med[2],
           "off_spread": spread(t[:, 0]), "inf_spread": spread(t[:, 1]), "finite_spread": spread(t[:, 2]),
           "inf_vs_off": (med[1] - med[0]) / med[0], "finite_vs_off": (med[2] - med[0]) / med[0],
           "off_ms_per_step": 1e3 / med[0], "inf_extra_us_per_step": 1e6 * (1 / med[1] - 1 / med[0]), "finite_extra_us_per_step": 1e6 * (1 / med[2] - 1 / med[0]),
           "finite_max_norm": max_norm, "finite_steps_clipped": clipped, "finite_steps_total": (a.rounds + 1) * a.steps,
           "off_and_inf_histories_identical": identical, "kernels": kern, "parent": parent}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for m in (off_m, inf_m, fin_m):
        m.close()


if __name__ == "__main__":
    main()

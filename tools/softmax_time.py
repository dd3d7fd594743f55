"""Time the Softmax likelihood against RobustMax on one model (needs a GPU): the forward ELBO step and the training step (``train_step``,
de-duplicated first layer) of the same cfg2 model (MNIST conv layer + head, M = 256, batch 32, S = 10), once with MultiClass(10) and
once with Softmax(10) at --points nodes, and the likelihoods' own launches from the device timers.  Prints one JSON line (milliseconds:
medians of --reps runs of --steps steps each, after --warmup steps; microseconds per launch for the timers).

    python tools/softmax_time.py [--steps 50] [--warmup 10] [--reps 5] [--points 100] [--only robustmax|softmax]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("robustmax", "softmax")
TIMERS = ("elbo_tail", "softmax_tail", "robustmax_grad", "softmax_grad")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--only", choices=("all",) + KINDS, default="all")
    a = ap.parse_args()
    from deepcgp_amd import synthetic as syn, device as dev      # noqa: E402
    from deepcgp_amd.likelihoods import MultiClass, Softmax      # noqa: E402
    from deepcgp_amd.models import build_from_spec               # noqa: E402
    cfg = syn.CONFIGS["cfg2_mnist_CH_M256"]
    X, lab = syn.make_batch(cfg["hwc"], cfg["batch"], seed=2)
    ctx = dev.get_context()
    res = {"tool": "softmax_time", "config": "cfg2_mnist_CH_M256", "batch": cfg["batch"], "S": cfg.get("S", 10), "Q": a.points,
           "steps": a.steps, "reps": a.reps}
    spec = syn.make_spec(cfg["hwc"], cfg["convs"], cfg["head"], cfg["M"], S=cfg.get("S", 10), num_data=cfg["num_data"], seed=1)
    dX, dY = ctx.to_device(X), ctx.to_device(lab, np.int32)
    for kind in [k for k in KINDS if a.only in ("all", k)]:
        model = build_from_spec(spec, X, lab, likelihood=MultiClass(10) if kind == "robustmax" else Softmax(10, a.points))
        model.dedup_layer0 = True

        def timed(fn):
            for i in range(a.warmup):
                fn(i)
            ctx.sync()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for i in range(a.steps):
                    fn(i)
                ctx.sync()
                ts.append(1e3 * (time.perf_counter() - t0) / a.steps)
            return float(np.median(ts))
        res[kind + "_elbo_ms"] = round(timed(lambda i: model.compute_log_likelihood(dX, dY, seed=i)), 4)
        res[kind + "_train_step_ms"] = round(timed(lambda i: model.train_step(dX, dY, 1e-4, seed=i)), 4)
        # the likelihood's own launches: device timers over a few more training steps (every launch timed: slower steps, not reported)
        ctx.timing_enable(1)
        ctx.timing_reset()
        for i in range(a.steps):
            model.train_step(dX, dY, 1e-4, seed=i)
        ctx.sync()
        tm = ctx.timing()
        ctx.timing_enable(0)
        res[kind + "_timers_us"] = {k: round(1e3 * tm[k][1] / tm[k][0], 2) for k in TIMERS if k in tm and tm[k][0]}
        model.close()
    if all(k + "_elbo_ms" in res for k in KINDS):
        res["elbo_softmax_minus_robustmax_us"] = round(1e3 * (res["softmax_elbo_ms"] - res["robustmax_elbo_ms"]), 2)
        res["train_softmax_minus_robustmax_us"] = round(1e3 * (res["softmax_train_step_ms"] - res["robustmax_train_step_ms"]), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

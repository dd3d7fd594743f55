"""Time the Gaussian likelihood against RobustMax on one model (needs a GPU): the forward ELBO step and the training step
(``train_step``, de-duplicated first layer) of the same cfg2 model with its head at D = 10, once with MultiClass(10) and once with
Gaussian(1.0).  Prints one JSON line (milliseconds, medians of --reps runs of --steps steps each, after --warmup steps).

    python tools/gaussian_time.py [--steps 50] [--warmup 10] [--reps 5] [--only gaussian|multiclass]

The tail kernels' own times come from a kernel trace of the same runs:
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/gaussian_time.py --steps 20 --reps 1"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepcgp_amd import synthetic as syn, device as dev      # noqa: E402
from deepcgp_amd.likelihoods import Gaussian, MultiClass     # noqa: E402
from deepcgp_amd.models import build_from_spec               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("both", "gaussian", "multiclass"), default="both")
    a = ap.parse_args()
    cfg = syn.CONFIGS["cfg2_mnist_CH_M256"]
    spec = syn.make_spec(cfg["hwc"], cfg["convs"], cfg["head"], cfg["M"], S=cfg.get("S", 10), num_data=cfg["num_data"], seed=1)
    X, lab = syn.make_batch(cfg["hwc"], cfg["batch"], seed=2)
    Y = np.random.default_rng(3).standard_normal((cfg["batch"], 10))
    ctx = dev.get_context()
    res = {"tool": "gaussian_time", "config": "cfg2_mnist_CH_M256", "batch": cfg["batch"], "S": cfg.get("S", 10), "D": 10, "steps": a.steps,
           "reps": a.reps}
    kinds = [k for k in ("multiclass", "gaussian") if a.only in ("both", k)]
    for kind in kinds:
        lik, targets = (Gaussian(1.0), Y) if kind == "gaussian" else (MultiClass(10), lab)
        model = build_from_spec(spec, X, targets, likelihood=lik)
        model.dedup_layer0 = True
        dX, dY = ctx.to_device(X), (ctx.to_device(Y) if kind == "gaussian" else ctx.to_device(lab, np.int32))

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
        model.close()
    if len(kinds) == 2:
        res["elbo_ratio_gaussian_over_multiclass"] = round(res["gaussian_elbo_ms"] / res["multiclass_elbo_ms"], 4)
        res["train_ratio_gaussian_over_multiclass"] = round(res["gaussian_train_step_ms"] / res["multiclass_train_step_ms"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Time one evaluation of a synthetic test set (needs a GPU): DGP_Base.evaluate -- the whole set in one device call -- against the
loops it replaces, AccuracyLogger (one predict_proba call per batch) and a per-batch predict_density loop.  Prints one JSON line.

    python tools/eval_time.py [--n 10000] [--S 5] [--batch 32] [--reps 5]

The model is the cfg2 geometry (28 x 28 x 1 images, conv layer 5 x 5 / 2 with 10 maps, ConvKernel head 5 x 5 / 1, M = 256); every
timed run is preceded by one untimed run of the same kind, and the median of --reps runs is reported (milliseconds)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepcgp_amd import synthetic as syn, device as dev      # noqa: E402
from deepcgp_amd.models import AccuracyLogger, build_from_spec   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--S", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("all", "evaluate"), default="all", help="evaluate: the one-call path alone (profiler runs)")
    a = ap.parse_args()
    cfg = syn.CONFIGS["cfg2_mnist_CH_M256"]
    spec = syn.make_spec(cfg["hwc"], cfg["convs"], cfg["head"], cfg["M"], S=a.S, num_data=cfg["num_data"], seed=1)
    X, Y = syn.make_batch(cfg["hwc"], a.n, seed=2)
    model = build_from_spec(spec, X[:cfg["batch"]], Y[:cfg["batch"]])
    ctx = dev.get_context()
    nb = -(-a.n // a.batch)

    def timed(fn):
        fn()                                   # first run: workspaces, the parameter-only chain
        ctx.sync()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn()
            ctx.sync()
            ts.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ts)), out

    def density_loop():
        return np.concatenate([model.predict_density(X[lo:lo + a.batch], Y[lo:lo + a.batch], a.S, seed=i)[:, 0]
                               for i, lo in enumerate(range(0, a.n, a.batch))])

    skips0 = model.chain_skips
    t_eval, r = timed(lambda: model.evaluate(X, Y, S=a.S, batch_size=a.batch, seed=0, per_image=True))
    res = {"tool": "eval_time", "config": "cfg2_mnist_CH_M256", "n": a.n, "S": a.S, "batch": a.batch, "batches": nb, "reps": a.reps,
           "evaluate_ms": round(t_eval, 3), "evaluate_images_per_s": round(1e3 * a.n / t_eval, 1),
           "chain_skips_per_call": (model.chain_skips - skips0) / (a.reps + 1),
           "accuracy": r["accuracy"], "mean_log_density": r["mean_log_density"]}
    if a.only == "all":
        t_acc, acc = timed(lambda: AccuracyLogger(X, Y, a.batch, a.S)(model, seed=0))
        t_loop, ld = timed(density_loop)
        res.update(accuracy_logger_ms=round(t_acc, 3), predict_density_loop_ms=round(t_loop, 3),
                   speedup_vs_accuracy_logger=round(t_acc / t_eval, 2), speedup_vs_density_loop=round(t_loop / t_eval, 2),
                   accuracy_equal=bool(acc == r["accuracy"]),
                   density_loop_max_abs_diff=float(np.max(np.abs(ld - r["log_density"]))))
    print(json.dumps(res))
    model.close()


if __name__ == "__main__":
    main()

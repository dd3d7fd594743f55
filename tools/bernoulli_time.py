"""Time the Bernoulli likelihood against RobustMax on one model (needs a GPU): the forward ELBO step and the training step
(``train_step``, de-duplicated first layer) of the same cfg2 model, once with MultiClass(10) at D = 10 and once with Bernoulli() at
D = 10 and at D = 1 (binary targets).  Prints one JSON line (milliseconds, medians of --reps runs of --steps steps each, after
--warmup steps).

    python tools/bernoulli_time.py [--steps 50] [--warmup 10] [--reps 5] [--only multiclass|bernoulli10|bernoulli1]

The tail kernels' own times come from a kernel trace of the same runs, one likelihood per trace (the Bernoulli kernels -- the shared kernels' BernoulliDensity instantiations -- have the
same names at both widths):
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/bernoulli_time.py --steps 20 --reps 1 --warmup 3 --only bernoulli1
and --kernels summarises those tables (<dir>/run_kernel_stats.csv) into one JSON line (average microseconds of the forward and reverse tails per trace):
    python tools/bernoulli_time.py --kernels multiclass=<stats.csv> bernoulli10=<stats.csv> bernoulli1=<stats.csv>"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("multiclass", "bernoulli10", "bernoulli1")
TAILS = {"forward": ("elbo_tail_kernel", "quad_tail_kernel"), "reverse": ("robustmax_grad_kernel", "quad_grad_kernel")}


def kernels(pairs):
    res = {"tool": "bernoulli_time", "kernels_avg_us": {}}
    for pair in pairs:
        label, path = pair.split("=", 1)
        with open(path) as f:
            rows = {r["Name"]: r for r in csv.DictReader(f)}
        out = {}
        for tail, names in TAILS.items():
            for name in names:
                for k, r in rows.items():
                    if re.search(r"(^|::|\s)%s[<(]" % re.escape(name), k):   # "void (anonymous namespace)::name(args)" or "...::name<BernoulliDensity>(args)"
                        out[tail] = {"kernel": name, "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2)}
        res["kernels_avg_us"][label] = out
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("all",) + KINDS, default="all")
    ap.add_argument("--kernels", nargs="+", metavar="LABEL=STATS_CSV")
    a = ap.parse_args()
    if a.kernels:
        return kernels(a.kernels)
    from deepcgp_amd import synthetic as syn, device as dev      # noqa: E402
    from deepcgp_amd.likelihoods import Bernoulli, MultiClass    # noqa: E402
    from deepcgp_amd.models import build_from_spec               # noqa: E402
    cfg = syn.CONFIGS["cfg2_mnist_CH_M256"]
    X, lab = syn.make_batch(cfg["hwc"], cfg["batch"], seed=2)
    ctx = dev.get_context()
    res = {"tool": "bernoulli_time", "config": "cfg2_mnist_CH_M256", "batch": cfg["batch"], "S": cfg.get("S", 10), "steps": a.steps,
           "reps": a.reps}
    for kind in [k for k in KINDS if a.only in ("all", k)]:
        D = 1 if kind == "bernoulli1" else 10
        spec = syn.make_spec(cfg["hwc"], cfg["convs"], cfg["head"], cfg["M"], S=cfg.get("S", 10), num_data=cfg["num_data"], seed=1,
                             head_outputs=D)
        Y = (np.random.default_rng(3).random((cfg["batch"], D)) < 0.5).astype(np.float64)
        lik, targets = (MultiClass(10), lab) if kind == "multiclass" else (Bernoulli(), Y)
        model = build_from_spec(spec, X, targets, likelihood=lik)
        model.dedup_layer0 = True
        dX, dY = ctx.to_device(X), (ctx.to_device(lab, np.int32) if kind == "multiclass" else ctx.to_device(Y))

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
    for kind in ("bernoulli10", "bernoulli1"):
        if "multiclass_elbo_ms" in res and kind + "_elbo_ms" in res:
            res["elbo_ratio_%s_over_multiclass" % kind] = round(res[kind + "_elbo_ms"] / res["multiclass_elbo_ms"], 4)
            res["train_ratio_%s_over_multiclass" % kind] = round(res[kind + "_train_step_ms"] / res["multiclass_train_step_ms"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

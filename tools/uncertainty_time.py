"""Time the uncertainty evaluation of a synthetic test set (needs a GPU): DGP_Base.evaluate_uncertainty -- entropies, BALD and the
calibration table of the whole set in one device call -- against DGP_Base.evaluate alone and against the host route it replaces, one
predict_y call per batch (S x n x K probabilities to the host, one synchronisation each) reduced by tests/uncertainty_ref.py.  Prints one
JSON line.

    python tools/uncertainty_time.py [--n 10000] [--S 5] [--batch 32] [--reps 5]

The model is the cfg2 geometry (28 x 28 x 1 images, conv layer 5 x 5 / 2 with 10 maps, ConvKernel head 5 x 5 / 1, M = 256).  Every route
runs once untimed; then the three routes alternate --reps times and the median of each is reported (milliseconds)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import uncertainty_ref as ur                                      # noqa: E402
from deepcgp_amd import synthetic as syn, device as dev           # noqa: E402
from deepcgp_amd.models import build_from_spec                    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--S", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, default=15)
    ap.add_argument("--only", choices=("all", "device"), default="all", help="device: the one-call path alone (profiler runs)")
    a = ap.parse_args()
    cfg = syn.CONFIGS["cfg2_mnist_CH_M256"]
    spec = syn.make_spec(cfg["hwc"], cfg["convs"], cfg["head"], cfg["M"], S=a.S, num_data=cfg["num_data"], seed=1)
    X, Y = syn.make_batch(cfg["hwc"], a.n, seed=2)
    model = build_from_spec(spec, X[:cfg["batch"]], Y[:cfg["batch"]])
    ctx = dev.get_context()

    def device_route():
        return model.evaluate_uncertainty(X, Y, S=a.S, batch_size=a.batch, seed=0, bins=a.bins, per_image=True)

    def evaluate_route():
        return model.evaluate(X, Y, S=a.S, batch_size=a.batch, seed=0, per_image=True)

    def host_route():
        parts = [ur.multiclass(model.predict_y(X[lo:lo + a.batch], a.S, seed=i)[0]) for i, lo in enumerate(range(0, a.n, a.batch))]
        out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        out.update(ur.calibration(out["p_mean"], Y, a.bins))
        return out

    routes = {"evaluate_uncertainty": device_route} if a.only == "device" else \
        {"evaluate_uncertainty": device_route, "evaluate": evaluate_route, "host_predict_y_loop": host_route}
    times, outs = {k: [] for k in routes}, {}
    for fn in routes.values():                 # first runs: workspaces, the parameter-only chain
        fn()
    ctx.sync()
    for _ in range(a.reps):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            outs[name] = fn()
            ctx.sync()
            times[name].append(1e3 * (time.perf_counter() - t0))
    med = {k: float(np.median(v)) for k, v in times.items()}
    r = outs["evaluate_uncertainty"]
    res = {"tool": "uncertainty_time", "config": "cfg2_mnist_CH_M256", "n": a.n, "S": a.S, "batch": a.batch, "bins": a.bins,
           "batches": -(-a.n // a.batch), "reps": a.reps, "evaluate_uncertainty_ms": round(med["evaluate_uncertainty"], 3),
           "evaluate_uncertainty_ms_min_max": [round(min(times["evaluate_uncertainty"]), 3), round(max(times["evaluate_uncertainty"]), 3)],
           "accuracy": r["accuracy"], "ece": r["ece"], "brier": r["brier"], "mean_predictive_entropy": r["mean_predictive_entropy"],
           "mean_mutual_information": r["mean_mutual_information"]}
    if a.only == "all":
        e, h = outs["evaluate"], outs["host_predict_y_loop"]
        res.update(evaluate_ms=round(med["evaluate"], 3), evaluate_ms_min_max=[round(min(times["evaluate"]), 3), round(max(times["evaluate"]), 3)],
                   host_predict_y_loop_ms=round(med["host_predict_y_loop"], 3),
                   overhead_vs_evaluate_percent=round(100.0 * (med["evaluate_uncertainty"] / med["evaluate"] - 1.0), 2),
                   speedup_vs_host_loop=round(med["host_predict_y_loop"] / med["evaluate_uncertainty"], 2),
                   p_mean_equal_to_evaluate=bool(np.array_equal(r["p_mean"], e["p_mean"]) and np.array_equal(r["log_density"], e["log_density"])),
                   host_loop_max_abs_diff_mutual_information=float(np.max(np.abs(h["mutual_information"] - r["mutual_information"]))),
                   host_loop_ece_abs_diff=float(abs(h["ece"] - r["ece"])))
    print(json.dumps(res))
    model.close()


if __name__ == "__main__":
    main()

"""Time the head's image-pair kernel dcgp_convkernel_k (ConvKernel.K, symmetric conv mode) and one predict_f_full_cov (needs a GPU).
Prints one JSON line.

    python tools/fullcov_time.py [--reps 20]

Geometries: the MNIST head-only head (28 x 28 x 1, f = 5: P = 576, L = 25), the MNIST conv + head head (12 x 12 x 10, f = 5: P = 64,
L = 250) and the CIFAR-3 head (11 x 11 x 10, f = 5: P = 49), at N in {32, 128} and B in {1, 10}.  Each point: one untimed call, then
the median of --reps calls (host wall clock around the synchronous call, inputs already on the device).  Work is counted as
B N (N + 1) / 2 P^2 2L flop (the pairs n <= n' the symmetric call evaluates) and reported as a fraction of the measured
v_mfma_f64_16x16x4_f64 rate.  predict_f_full_cov: the cfg2 conv + head model at N = 32, S = 10, M = 256."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepcgp_amd import synthetic as syn, device as dev      # noqa: E402
from deepcgp_amd.models import build_from_spec                # noqa: E402

GEOMS = {"mnist_head": (28, 28, 1, 5, 1), "mnist_conv_head": (12, 12, 10, 5, 1), "cifar3_head": (11, 11, 10, 5, 1)}


def median_ms(fn, reps, ctx):
    fn()
    ctx.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ctx, L = dev.get_context(), dev.lib()
    peak = ctx.measured_mfma_f64_tflops()
    res = {"tool": "fullcov_time", "reps": a.reps, "mfma_f64_tflops": round(peak, 2), "convkernel_k": []}
    rng = np.random.default_rng(0)
    for name, (H, W, C, f, s) in GEOMS.items():
        P, Lp = ((H - f) // s + 1) * ((W - f) // s + 1), f * f * C
        w = ctx.to_device(0.5 + rng.random(P))
        for N in (32, 128):
            for B in (1, 10):
                dX = ctx.to_device(rng.standard_normal((B, N, H, W, C)))
                out = ctx.empty((B, N, N))
                ls = 0.4 * np.sqrt(Lp) + 0.5

                def call():
                    ctx._check(L.dcgp_convkernel_k(ctx.handle, dX.ptr, None, B, N, N, H, W, C, f, s, 5.0, ls, w.ptr, 0, out.ptr))
                ms = median_ms(call, a.reps, ctx)
                flop = B * N * (N + 1) / 2 * P * P * 2 * Lp
                tfs = flop / (ms * 1e-3) / 1e12
                res["convkernel_k"].append({"geom": name, "P": P, "L": Lp, "N": N, "B": B, "ms": round(ms, 4), "gflop": round(flop / 1e9, 2),
                                            "tflops": round(tfs, 2), "frac_of_mfma": round(tfs / peak, 3)})
    cfg = syn.CONFIGS["cfg2_mnist_CH_M256"]
    spec = syn.make_spec(cfg["hwc"], cfg["convs"], cfg["head"], cfg["M"], S=10, num_data=cfg["num_data"], seed=1)
    X, Y = syn.make_batch(cfg["hwc"], 32, seed=2)
    model = build_from_spec(spec, X, Y)
    res["predict_f_full_cov_ms"] = round(median_ms(lambda: model.predict_f_full_cov(X, 10, seed=0), max(3, a.reps // 4), ctx), 2)
    res["predict_f_ms"] = round(median_ms(lambda: model.predict_f(X, 10, seed=0), max(3, a.reps // 4), ctx), 3)
    model.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

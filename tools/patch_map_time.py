"""Time the per-patch evidence kernel dcgp_convkernel_patch_mean against the composed route it replaces and against the reduced sweep
(needs a GPU).  Prints one JSON line.

    python tools/patch_map_time.py [--reps 20]

Heads: the headline head (28 x 28 x 1, f = 5: P = 576, L = 25, M = 256, R = 10, N = 32 * 10 images) and the long-patch head of cfg3
(9 x 9 x 10, f = 5: P = 25, L = 250, M = 256, R = 10, N = 64 * 10).  Per head, on the same device inputs in one process:
  new_us       dcgp_convkernel_patch_mean (operand preparation + the fused launch);
  composed_us  dcgp_kuf_patches_rbf into a [P, M, N] buffer + dcgp_gemm_strided to [N, P, R] (without the w_p / P scale);
  kzx_us       dcgp_convkernel_kzx (the same sweep reduced over p, no second product).
Times are HIP-event times of the library's kernel families (ctx.timing: events around every launch of the call, summed), one untimed
call, then the median of --reps calls; *_wall_us is the host wall clock around the same synchronous calls.  mfma_frac: the flop count
2 N P M (L + R) over new_us against the v_mfma_f64_16x16x4_f64 rate measured in the same run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepcgp_amd import device as dev      # noqa: E402

HEADS = {"headline_mnist_head": (28, 28, 1, 5, 1, 256, 10, 320), "cfg3_long_patch_head": (9, 9, 10, 5, 1, 256, 10, 640)}


def timed(ctx, fn, reps):
    """(median event us, median wall us, kernel families seen)"""
    fn()
    ctx.sync()
    ev, wall, fam = [], [], set()
    for _ in range(reps):
        ctx.timing_reset()
        t0 = time.perf_counter()
        fn()
        wall.append(1e6 * (time.perf_counter() - t0))
        t = ctx.timing()
        fam.update(k for k, (n, _) in t.items() if n)
        ev.append(1e3 * sum(ms for _, ms in t.values()))
    return float(np.median(ev)), float(np.median(wall)), sorted(fam)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ctx, L = dev.get_context(), dev.lib()
    peak = ctx.measured_mfma_f64_tflops()
    res = {"tool": "patch_map_time", "reps": a.reps, "mfma_f64_tflops": round(peak, 2), "heads": []}
    rng = np.random.default_rng(0)
    ctx.timing_enable(1)
    for name, (H, W, C, f, s, M, R, N) in HEADS.items():
        P, Lp = ((H - f) // s + 1) * ((W - f) // s + 1), f * f * C
        ls = 0.4 * np.sqrt(Lp) + 0.5
        X = rng.standard_normal((N, H, W, C))
        dX, dZ = ctx.to_device(X), ctx.to_device(rng.standard_normal((M, Lp)))
        dw, db = ctx.to_device(0.5 + rng.random(P)), ctx.to_device(rng.standard_normal((M, R)))
        out, kuf, out2, kzx = ctx.empty((N, P, R)), ctx.empty((P, M, N)), ctx.empty((N, P, R)), ctx.empty((M, N))

        def new():
            ctx._check(L.dcgp_convkernel_patch_mean(ctx.handle, dX.ptr, N, H, W, C, f, s, dZ.ptr, M, 5.0, ls, dw.ptr, db.ptr, R, out.ptr))

        def composed():
            ctx._check(L.dcgp_kuf_patches_rbf(ctx.handle, dX.ptr, N, H, W, C, f, s, dZ.ptr, M, 5.0, ls, kuf.ptr, 0))
            ctx.gemm(kuf, (1, N, M * N), db, (R, 1, 0), out2, P * R, R, N, R, M, batch=P)

        def reduced():
            ctx._check(L.dcgp_convkernel_kzx(ctx.handle, dX.ptr, N, H, W, C, f, s, dZ.ptr, M, 5.0, ls, dw.ptr, kzx.ptr))

        n_us, n_wall, n_fam = timed(ctx, new, a.reps)
        c_us, c_wall, c_fam = timed(ctx, composed, a.reps)
        k_us, k_wall, k_fam = timed(ctx, reduced, a.reps)
        # the two routes agree (the composed one lacks the w_p / P scale)
        got, want = out.numpy(), out2.numpy() * (dw.numpy() / P)[None, :, None]
        flop = 2.0 * N * P * M * (Lp + R)
        res["heads"].append({"head": name, "P": P, "L": Lp, "M": M, "R": R, "N": N,
                             "new_us": round(n_us, 1), "composed_us": round(c_us, 1), "kzx_us": round(k_us, 1),
                             "new_wall_us": round(n_wall, 1), "composed_wall_us": round(c_wall, 1), "kzx_wall_us": round(k_wall, 1),
                             "gflop": round(flop / 1e9, 2), "mfma_frac": round(flop / (n_us * 1e-6) / 1e12 / peak, 3),
                             "max_rel_diff_routes": float(np.max(np.abs(got - want)) / np.max(np.abs(want))),
                             "families": {"new": n_fam, "composed": c_fam, "kzx": k_fam}})
    ctx.timing_enable(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

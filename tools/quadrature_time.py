"""Time the StudentT and Poisson likelihoods beside the Gaussian and Bernoulli ones on one model (needs a GPU): the forward ELBO step
and the training step (``train_step``, de-duplicated first layer) of the headline cfg2 model (MNIST conv layer + head, M = 256, batch 32,
S = 10) with a D = 10 head, the four models built in the same run, and each likelihood's own launches -- the ELBO tail and the gradient
tail -- from the device timers of ``ctx.timing()``.  Prints one JSON line (medians of --reps runs of --steps steps each, after --warmup
steps; the timers over --steps further training steps).

    python tools/quadrature_time.py [--steps 50] [--warmup 10] [--reps 5] [--only studentt|poisson|gaussian|bernoulli]

Bernoulli's tails are the yardstick: the same 20-node rule, in the same run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("studentt", "poisson", "gaussian", "bernoulli")
TAILS = {kind: ("quad_tail", "quad_grad") for kind in KINDS}      # one set of kernels (csrc/pointwise.hip), one timer each


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("all",) + KINDS, default="all")
    a = ap.parse_args()
    from deepcgp_amd import synthetic as syn, device as dev                          # noqa: E402
    from deepcgp_amd.likelihoods import Bernoulli, Gaussian, Poisson, StudentT       # noqa: E402
    from deepcgp_amd.models import build_from_spec                                   # noqa: E402
    cfg = syn.CONFIGS["cfg2_mnist_CH_M256"]
    D = 10
    X, _ = syn.make_batch(cfg["hwc"], cfg["batch"], seed=2)
    ctx = dev.get_context()
    res = {"tool": "quadrature_time", "config": "cfg2_mnist_CH_M256", "batch": cfg["batch"], "S": cfg.get("S", 10), "D": D, "steps": a.steps,
           "reps": a.reps}
    spec = syn.make_spec(cfg["hwc"], cfg["convs"], cfg["head"], cfg["M"], S=cfg.get("S", 10), num_data=cfg["num_data"], seed=1, head_outputs=D)
    rng = np.random.default_rng(3)
    cases = {"studentt": (StudentT(1.0, 3.0), rng.standard_normal((cfg["batch"], D))),
             "poisson": (Poisson(), rng.poisson(2.5, (cfg["batch"], D)).astype(np.float64)),
             "gaussian": (Gaussian(1.0), rng.standard_normal((cfg["batch"], D))),
             "bernoulli": (Bernoulli(), (rng.random((cfg["batch"], D)) < 0.5).astype(np.float64))}
    dX = ctx.to_device(X)
    for kind in [k for k in KINDS if a.only in ("all", k)]:
        lik, Y = cases[kind]
        model = build_from_spec(spec, X, Y, likelihood=lik)
        model.dedup_layer0 = True
        dY = ctx.to_device(Y)

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
        elbo_ms = timed(lambda i: model.compute_log_likelihood(dX, dY, seed=i))
        res[kind + "_elbo_steps_per_s"] = round(1e3 / elbo_ms, 1)
        res[kind + "_train_step_ms"] = round(timed(lambda i: model.train_step(dX, dY, 1e-4, seed=i)), 4)
        # the likelihood's own launches: device timers over a few more training steps (every launch timed: slower steps, not reported)
        ctx.timing_enable(1)
        ctx.timing_reset()
        for i in range(a.steps):
            model.train_step(dX, dY, 1e-4, seed=i)
        ctx.sync()
        tm = ctx.timing()
        ctx.timing_enable(0)
        for label, name in zip(("elbo_tail_us", "grad_tail_us"), TAILS[kind]):
            if name in tm and tm[name][0]:
                res["%s_%s" % (kind, label)] = round(1e3 * tm[name][1] / tm[name][0], 2)
        model.close()
    for kind in ("studentt", "poisson"):
        for label in ("elbo_tail_us", "grad_tail_us"):
            if "%s_%s" % (kind, label) in res and "bernoulli_" + label in res:
                res["%s_over_bernoulli_%s" % (kind, label[:-3])] = round(res["%s_%s" % (kind, label)] / res["bernoulli_" + label], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

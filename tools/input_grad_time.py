"""Time DGP_Base.input_gradient beside the training reverse pass and the forward pass on a bench configuration (needs a GPU), one JSON line:
    python tools/input_grad_time.py [config] [repeats]          (DCGP_DEDUP=1: with dedup_layer0, as tools/grad_time.py)
Headline: cfg2 (conv + head, M = 256), batch 32, S = 10.  Every figure is the median over `repeats` calls after 3 warm-up calls on
device-resident inputs with device RNG (seed = call index).  Unlike tools/grad_time.py, which times a batch of steps behind one
synchronisation, each call is timed on its own from the host and ends in its own synchronisation; input_gradient's figure also includes the
copy of J and dX back to the host, which the other two calls do not pay, so input_grad_ms < elbo_grad_ms is read conservatively."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepcgp_amd import synthetic as syn, device as dev
from deepcgp_amd.models import build_from_spec

name = sys.argv[1] if len(sys.argv) > 1 else "cfg2_mnist_CH_M256"
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 30
cfg = syn.CONFIGS[name]
S = 10
spec = syn.make_spec(cfg["hwc"], cfg["convs"], cfg["head"], cfg["M"], S=S, num_data=cfg["num_data"], seed=1)
X, Y = syn.make_batch(cfg["hwc"], cfg["batch"], seed=1)
model = build_from_spec(spec, X, Y)
model.dedup_layer0 = bool(int(os.environ.get("DCGP_DEDUP", "0")))
model.set_factor_reuse(0)   # every call runs its own parameter-only chain, as a training step does
ctx = dev.get_context()
dX, dY = ctx.to_device(X), ctx.to_device(Y, np.int32)


def median_ms(fn):
    for i in range(3):
        fn(i)
    ctx.sync()
    ts = []
    for i in range(repeats):
        t0 = time.perf_counter()
        fn(i)
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


out = {"config": name, "batch": int(X.shape[0]), "S": S, "dedup_layer0": bool(model.dedup_layer0), "repeats": repeats}
out["forward_ms"] = median_ms(lambda i: model.compute_log_likelihood(dX, dY, seed=i))
out["elbo_grad_ms"] = median_ms(lambda i: model.compute_gradients(dX, dY, seed=i, fetch=False))
out["input_grad_ms"] = {o: median_ms(lambda i, o=o: model.input_gradient(dX, dY, objective=o, seed=i)) for o in ("density", "elbo")}
print(json.dumps(out))

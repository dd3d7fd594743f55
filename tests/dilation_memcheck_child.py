"""Worker of tests/test_gpu_dilation_memcheck.py (not collected by pytest): ``python tests/dilation_memcheck_child.py <stack>`` runs a dilated
stack of tests/dilation_ref.py in a fresh process and prints the ``MODES`` and ``RESULT`` lines of tests/memcheck_scenarios.py (whose ``Results``
hashes every output whole).  Scenarios: ``dil2_odd`` and ``dil3_pad``, the stacks with phantom outputs; each runs the ELBO, the gradient (tiled
and de-duplicated), ``input_gradient`` (both objectives) and a 3-step ``train_run``.  A phantom column that reached a sum, or a fill zero of
the split batch that was not rewritten, reads a NaN under DCGP_POISON_WS and changes the hash."""
import copy
import gc
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from memcheck_scenarios import Results, values      # noqa: E402

SCENARIOS = ("dil2_odd", "dil3_pad")


def run_stack(res, name):
    import dilation_ref as dr
    from deepcgp_amd import synthetic as syn
    from deepcgp_amd.models import build_from_spec
    spec, X, Y, zs = dr.make_stack(name)
    model = build_from_spec(copy.deepcopy(spec), X.copy(), Y.copy())
    res.add(name + "/elbo", model.compute_log_likelihood(X, Y, zs=zs, return_parts=True))
    for dedup in (False, True):
        model.dedup_layer0 = dedup
        e, g = model.compute_gradients(X, Y, zs=zs)
        res.add("%s/grad dedup=%d/elbo" % (name, dedup), e)
        res.add("%s/grad dedup=%d" % (name, dedup), g)
        for objective in ("density", "elbo"):
            res.add("%s/input_gradient %s dedup=%d" % (name, objective, dedup), model.input_gradient(X, Y, objective=objective, zs=zs))
    res.add(name + "/layers", model.predict_all_layers(X, spec["S"], zs=zs))
    res.close(model, name)
    pool, batch, steps = 9, 4, 3
    Xp, _ = syn.make_batch(dr.STACKS[name]["hwc"], pool, seed=7)
    Yp = np.random.default_rng(99).integers(0, 10, pool).astype(np.int32)
    idx = np.stack([np.random.default_rng(5 + i).choice(pool, batch, replace=False) for i in range(steps)])
    model = build_from_spec(copy.deepcopy(spec), Xp, Yp)
    model.attach_dataset()
    res.add(name + "/train_run", model.train_run(idx, np.full(steps, 0.01), seed=11))
    res.add(name + "/after train_run", values(model))
    model.detach_dataset()
    res.close(model, name + " train_run")


def main(name):
    from deepcgp_amd import device as dev
    res = Results()
    ctx = dev.get_context()
    run_stack(res, name)
    gc.collect()
    res.check(ctx, "the end")
    assert res.count > 0
    print("MODES guard %d poison %d" % (ctx.guard_bytes(), int("DCGP_POISON_WS" in os.environ)))
    print("RESULT %s %d %d" % (res.h.hexdigest(), res.n_bad, int(res.finite)))


if __name__ == "__main__":
    assert len(sys.argv) == 2 and sys.argv[1] in SCENARIOS, sys.argv
    main(sys.argv[1])

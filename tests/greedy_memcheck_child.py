"""Worker of tests/test_gpu_greedy_memcheck.py (not collected by pytest): ``python tests/greedy_memcheck_child.py <scenario>`` runs the operator
cases of tests/test_gpu_greedy.py in a fresh process and prints the ``MODES`` and ``RESULT`` lines of tests/memcheck_scenarios.py (whose
``Results`` hashes every output whole).  Scenarios: ``parity`` (every shape under every kernel, with the factor), ``paths`` (several columns a
lane, k = n, the stall on duplicates with and without the caller's factor, a floor that selects nothing, the host fill)."""
import gc
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from memcheck_scenarios import Results      # noqa: E402

SCENARIOS = ("parity", "paths")
VARIANCE = 5.0
SHAPES = [(1, 3, 1), (64, 9, 8), (257, 25, 32), (517, 27, 33), (300, 490, 24)]
KERNELS = ["rbf", "rbf_ard", "matern32", "matern52", "acos"]


def make_kernel(kern, d, rng):
    from deepcgp_amd.kernels import RBF, ArcCosine, Matern32, Matern52
    ls = float(np.sqrt(d))
    if kern == "rbf":
        return RBF(d, VARIANCE, ls)
    if kern == "rbf_ard":
        return RBF(d, VARIANCE, ls * rng.uniform(0.5, 1.5, d), ARD=True)
    if kern == "matern32":
        return Matern32(d, VARIANCE, ls)
    if kern == "matern52":
        return Matern52(d, VARIANCE, ls)
    return ArcCosine(d, 0, VARIANCE, 1.0, 1.0)


def run_parity(res, ctx):
    from deepcgp_amd.kernels import greedy_variance_device
    for n, d, k in SHAPES:
        for kern in KERNELS:
            rng = np.random.default_rng(n)
            X = rng.standard_normal((n, d))
            res.add("parity %d %d %d %s" % (n, d, k, kern), greedy_variance_device(X, k, make_kernel(kern, d, rng), min_variance=0.0, factor=True))
        res.check(ctx, "parity n = %d" % n)


def run_paths(res, ctx):
    from deepcgp_amd.kernels import RBF, greedy_variance, greedy_variance_device
    rng = np.random.default_rng(517)
    X = rng.standard_normal((517, 27))
    for kern in ("rbf", "acos"):
        with ctx.options(greedy_wgs=2):
            res.add("two columns a lane " + kern, greedy_variance_device(X, 33, make_kernel(kern, 27, rng), min_variance=0.0, factor=True))
    X = np.random.default_rng(64).standard_normal((64, 9))
    res.add("k = n", greedy_variance_device(X, 64, RBF(9, VARIANCE, 3.0), min_variance=0.0, factor=True))
    res.add("nothing above the floor", greedy_variance_device(X, 8, RBF(9, VARIANCE, 3.0), min_variance=VARIANCE, factor=True))
    res.check(ctx, "paths")
    rng = np.random.default_rng(40)
    X = np.repeat(rng.standard_normal((10, 9)), 4, axis=0)[rng.permutation(40)]
    res.add("stall, factor", greedy_variance_device(X, 16, RBF(9, VARIANCE, 3.0), factor=True))
    res.add("stall, no factor", greedy_variance_device(X, 16, RBF(9, VARIANCE, 3.0)))      # the factor in the call's own scratch: rows 10.. stay unwritten
    Z, info = greedy_variance(X, 16, RBF(9, VARIANCE, 3.0), return_info=True)
    res.add("fill", (Z, info))
    res.check(ctx, "stall")


def main(name):
    from deepcgp_amd import device as dev
    res = Results()
    ctx = dev.get_context()
    {"parity": run_parity, "paths": run_paths}[name](res, ctx)
    gc.collect()
    res.check(ctx, "the end")
    assert res.count > 0
    print("MODES guard %d poison %d" % (ctx.guard_bytes(), int("DCGP_POISON_WS" in os.environ)))
    print("RESULT %s %d %d" % (res.h.hexdigest(), res.n_bad, int(res.finite)))


if __name__ == "__main__":
    main(sys.argv[1])

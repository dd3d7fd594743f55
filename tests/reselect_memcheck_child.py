"""Worker of tests/test_gpu_reselect_memcheck.py (not collected by pytest): ``python tests/reselect_memcheck_child.py <scenario>`` runs cases of
tests/test_gpu_reselect.py in a fresh process and prints the ``MODES`` and ``RESULT`` lines of tests/memcheck_scenarios.py (whose ``Results``
hashes every output whole).  Scenarios: ``transfer`` (the cross Gram matrix under every kernel; the transfer at every shape, whitened and not,
under every kernel, with the 1e-5-scaled q_sqrt, and the call that is not positive definite, whose output buffers must keep their bits);
``model`` (``reselect_inducing`` on a trained conv + conv + patch-head model and on one with the dense head, then two more steps)."""
import ctypes as C
import gc
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from memcheck_scenarios import Results      # noqa: E402

SCENARIOS = ("transfer", "model")


def run_transfer(res, ctx):
    import test_gpu_reselect as tg
    from deepcgp_amd import device as dev
    from deepcgp_amd.kernels import cross_gram, transfer_inducing
    for kern in tg.KERNELS:
        rng = np.random.default_rng(70)
        A, B = rng.standard_normal((70, 250)), rng.standard_normal((24, 250))
        B[3] = A[5]
        res.add("cross_gram " + kern, cross_gram(A, B, tg.make_kernel(kern, 250, rng)[0]))
    res.check(ctx, "cross_gram")
    for M, Mn in tg.SHAPES:
        for white in (False, True):
            Z, Zn, bk, _, q_mu, q_sqrt = tg.case(M, Mn, 9, 3, "rbf")
            res.add("transfer %d %d %d" % (M, Mn, white), transfer_inducing(Z, Zn, bk, q_mu, q_sqrt, white=white, jitter=tg.JITTER))
        res.check(ctx, "transfer M = %d, M' = %d" % (M, Mn))
    for kern in tg.KERNELS[1:]:
        for white in (False, True):
            Z, Zn, bk, _, q_mu, q_sqrt = tg.case(70, 33, 25, 3, kern)
            res.add("transfer %s %d" % (kern, white), transfer_inducing(Z, Zn, bk, q_mu, q_sqrt, white=white, jitter=tg.JITTER))
    Z, Zn, bk, _, q_mu, q_sqrt = tg.case(24, 24, 9, 3, "rbf", scale=1e-5)
    res.add("small q_sqrt", transfer_inducing(Z, Zn, bk, q_mu, q_sqrt, jitter=tg.JITTER))
    res.check(ctx, "kernels")
    # not positive definite: the status, and the caller's buffers as they were
    Z, Zn, bk, _, q_mu, q_sqrt = tg.case(24, 16, 9, 3, "rbf")
    Zd = Zn.copy()
    Zd[1] = Zd[0]
    dZ, dZn, dm, dS = ctx.to_device(Z), ctx.to_device(Zd), ctx.to_device(q_mu), ctx.to_device(q_sqrt)
    om, oS = ctx.to_device(np.full((16, 3), 7.25)), ctx.to_device(np.full((3, 16, 16), -3.5))
    info = (C.c_int * 2)(0, 0)
    rc = dev.lib().dcgp_inducing_transfer(ctx.handle, dZ.ptr, 24, dZn.ptr, 16, 9, 0, bk.variance, bk.lengthscales, 0.0, None, 0.0, 0, dm.ptr, dS.ptr,
                                          3, om.ptr, oS.ptr, info)
    res.add("not PD", [np.array([rc, info[0], info[1]]), om.numpy(), oS.numpy()])
    res.check(ctx, "not PD")


def run_model(res, ctx):
    import test_gpu_reselect as tg
    for variant in ("rbf", "dense"):
        spec, X, Y, model = tg.trained_model(variant)
        report = model.reselect_inducing(images=30, seed=tg.SEED, candidates=20)
        res.add("report " + variant, report)
        res.check(ctx, "reselect " + variant)
        res.add("steps " + variant, model.train_run(np.random.default_rng(6).integers(0, tg.NTRAIN, (2, 4)), 0.01, seed=40))
        res.add("state " + variant, tg.all_bits(model))
        res.check(ctx, "steps " + variant)
        model.close()


def main(name):
    from deepcgp_amd import device as dev
    res = Results()
    ctx = dev.get_context()
    {"transfer": run_transfer, "model": run_model}[name](res, ctx)
    gc.collect()
    res.check(ctx, "the end")
    assert res.count > 0
    print("MODES guard %d poison %d" % (ctx.guard_bytes(), int("DCGP_POISON_WS" in os.environ)))
    print("RESULT %s %d %d" % (res.h.hexdigest(), res.n_bad, int(res.finite)))


if __name__ == "__main__":
    main(sys.argv[1])

"""The layer kernel on a tiled batch: the strips that show the same images at the same patches share one prologue (csrc/fused_plan.h:
plan_layer_launch; ctx option fused_rep_share, -1 chosen / 0 off).

DGP_Base.propagate tiles the minibatch S times in front of the first layer, so strip i of layer 0 and strip i + k D (D = N P / strip width, where that
is a whole number) compute the same K_uf, A1 and sum A1^2.  The shared launch runs D of them whole, has those leave their A1 in memory on the way, and
starts every strip behind the first round at the second product.  Same instructions on the same operands: every case compares the launch with
fused_rep_share = 0 against the default with assert_array_equal, three shared launches in one process (device counter, flag epochs).

Small layers are put through several rounds by fused_wgs (that many persistent workgroups instead of one per CU) and fused_shape (6: 16-column strips,
0: 64-column strips, both one workgroup per CU, as the hand-over needs).  dcgp_debug_fused_plan says which plan the last launch took, so a case that is
meant to share (or to fall back) cannot pass by doing the other; and every launch took the plan that the planner (csrc/fused_plan.h, asked through
dcgp_debug_plan_layer_launch) gives for a query built here from the spec, the ctx's options and its device."""
import os

import numpy as np
import pytest

import fused_plan_cases as fc

pytestmark = pytest.mark.gpu

HWC = (12, 12, 1)      # f = 5, s = 2: P = 16 patches per image
CONV = (5, 2)


def _plan(ctx):
    """(workgroups, items, hand-over slots, distinct strips D of the shared plan or 0) of the most recent layer-kernel launch"""
    return fc.last_launch(ctx)


def _planned(ctx, M, R, N, S, base="rbf"):
    """the same four values of the plan for layer 0 on N images tiled S times, under the ctx's options of the moment"""
    return fc.debug_plan_of(fc.plan(fc.ctx_query(ctx, HWC, CONV[0], CONV[1], M, R, N * S, N, base=base)))


_models = {}


def _model(M, R, base="rbf", idm=False):
    """one model per parameter set for the whole module (building one factors its matrices on the device)"""
    key = (M, R, base, idm)
    if key not in _models:
        from deepcgp_amd import synthetic as syn
        from deepcgp_amd.models import build_from_spec
        spec = syn.make_spec(HWC, [CONV + (R,)], (3, 1), M=M, S=3, num_data=500, seed=17 + M + R, conv_q_sqrt_scale=0.3, base_kernel=base)
        if idm:
            spec["convs"][0]["mean_function"] = "conv2d"
        X, Y = syn.make_batch(HWC, 4, seed=3)
        _models[key] = (spec, build_from_spec(spec, X, Y))
    return _models[key]


def _layer0(model, X, S, zs, seed):
    Fs, Fm, Fv = model.propagate(X, S=S, zs=zs, seed=seed)
    return Fs[0], Fm[0], Fv[0]


def _check(ctx, M, R, N, S, shape, wgs, want_D, noise="z", base="rbf", idm=False):
    from deepcgp_amd import synthetic as syn
    spec, model = _model(M, R, base, idm)
    X, _ = syn.make_batch(HWC, N, seed=100 + N)
    zs = None
    if noise == "z":
        spec_s = dict(spec, S=S)
        zs = syn.make_noise(spec_s, N, seed=7)
    BN = 16 if shape == 6 else 64
    strips = (N * S * 16 + BN - 1) // BN
    with ctx.options(fused_shape=shape, fused_persist=1, fused_wgs=wgs):
        with ctx.options(fused_rep_share=0):
            ref = _layer0(model, X, S, zs, 11)
            plan0 = _plan(ctx)
            assert plan0 == _planned(ctx, M, R, N, S, base)
        assert plan0[0] == wgs and plan0[3] == 0, plan0
        for _ in range(3):
            got = _layer0(model, X, S, zs, 11)
            plan = _plan(ctx)
            assert plan == _planned(ctx, M, R, N, S, base)
            assert plan[0] == wgs and plan[3] == want_D, (plan, want_D)
            if want_D:
                assert plan[1] == strips and plan[2] == want_D, plan     # one item per strip, one slot per distinct strip
            else:
                assert plan[1:] == plan0[1:], (plan, plan0)                # the fall-back is today's launch
            for g, r, what in zip(got, ref, ("sample", "mean", "variance")):
                assert np.all(np.isfinite(g)), what
                np.testing.assert_array_equal(g, r, err_msg=what)
    return ref


@pytest.mark.parametrize("noise", ["z", "philox"])
@pytest.mark.parametrize("M,R,N,S,shape,wgs,D", [
    (32, 3, 4, 3, 6, 4, 4),      # 12 strips of 16 columns on 4 workgroups: whole rounds, D = slots
    (32, 3, 4, 3, 6, 5, 4),      # ... on 5: a partial last round, a first-round strip that neither leaves nor fetches
    (256, 10, 4, 3, 6, 4, 4),
    (256, 3, 4, 3, 6, 5, 4),
    (256, 10, 8, 3, 0, 2, 2),    # 64-column strips: 6 strips, D = 2 = slots
    (32, 10, 8, 6, 0, 4, 2),     # 12 strips on 4 workgroups, D < slots
    (32, 3, 8, 3, 6, 3, 8),      # D > slots: the strips 3 .. 7 leave their A1 from a later round, still ahead of their readers
    (256, 3, 8, 4, 6, 3, 8),     # ... and 32 strips on 3 workgroups: a partial last round
    (32, 3, 4, 5, 0, 2, 1),      # D = 1: every strip a replica of strip 0; 5 strips on 2 workgroups
    (256, 10, 4, 6, 0, 2, 1),
])
def test_replicas_share_a_prologue(ctx, noise, M, R, N, S, shape, wgs, D):
    _check(ctx, M, R, N, S, shape, wgs, D, noise=noise)


@pytest.mark.parametrize("noise", ["z", "philox"])
@pytest.mark.parametrize("M,R,N,S,shape,wgs", [
    (32, 3, 3, 4, 0, 2),         # a period of 48 columns on 64-column strips: strips straddle replicas
    (256, 10, 3, 4, 0, 2),
    (32, 3, 5, 3, 0, 3),         # 240 columns: a period of 80 and a last strip of which 48 columns lie in the matrix
    (256, 10, 5, 3, 0, 2),
])
def test_misaligned_period_and_ragged_last_strip_fall_back(ctx, noise, M, R, N, S, shape, wgs):
    """A tiled batch ends on a period boundary, so a last strip that is partly past the matrix always comes with a period that is no whole number of
    strips: both take today's plan."""
    _check(ctx, M, R, N, S, shape, wgs, 0, noise=noise)


@pytest.mark.parametrize("M,R,N,S,shape,wgs", [(256, 10, 8, 4, 0, 3), (32, 10, 4, 4, 0, 3)])
def test_the_simulated_deal_keeps_prologues_ahead_where_they_do_as_well(ctx, M, R, N, S, shape, wgs):
    """8 strips (D = 2) and 4 strips (D = 1) on 3 workgroups at R = 10: the spare workgroups of the partial first round already run every later prologue
    ahead, the shared deal is no shorter (33.25 against 33.05 units, 22.55 against 22.55), and the launch stays as it is."""
    _check(ctx, M, R, N, S, shape, wgs, 0)


def test_untiled_rows_fall_back(ctx):
    _check(ctx, 32, 3, 12, 1, 6, 4, 0)


@pytest.mark.parametrize("S,shape,wgs,D", [(3, 6, 4, 4), (5, 0, 2, 1)])
def test_shared_prologue_with_conv2d_mean(ctx, S, shape, wgs, D):
    """Conv2dMean adds the centre pixel of the strip's OWN rows' images: a consumer reads it at its own columns"""
    ref = _check(ctx, 32, 3, 4, S, shape, wgs, D, idm=True)
    plain = _check(ctx, 32, 3, 4, S, shape, wgs, D)
    assert np.abs(ref[1] - plain[1]).max() > 1e-3     # (the mean function is there)


@pytest.mark.parametrize("base", ["matern32", "matern52", "acos"])
@pytest.mark.parametrize("M,R,N,S,shape,wgs,D", [(32, 3, 4, 3, 6, 5, 4), (256, 10, 8, 3, 0, 2, 2)])
def test_shared_prologue_with_other_base_kernels(ctx, base, M, R, N, S, shape, wgs, D):
    """Matern and ArcCosine apply |z_m|^2 after the sweep (the zn path of the prologue)"""
    _check(ctx, M, R, N, S, shape, wgs, D, base=base)


def test_consumers_draw_their_own_noise(ctx):
    """Replicas share A1, not their samples: with Philox noise the S copies of an image differ, and mean and variance do not"""
    from deepcgp_amd import synthetic as syn
    _, model = _model(32, 3)
    X, _ = syn.make_batch(HWC, 4, seed=104)
    with ctx.options(fused_shape=6, fused_persist=1, fused_wgs=4):
        smp, mean, var = _layer0(model, X, 3, None, 5)
        assert _plan(ctx)[3] == 4 and _plan(ctx) == _planned(ctx, 32, 3, 4, 3)
    np.testing.assert_array_equal(mean[0], mean[1])
    np.testing.assert_array_equal(var[0], var[2])
    assert np.abs(smp[0] - smp[1]).min() > 0 and np.abs(smp[0] - smp[2]).min() > 0


def test_live_spec_elbo_with_two_steps_in_flight_on_the_masked_stream(ctx):
    """The flagship spec (720 strips, 72 distinct) on a CU-masked main stream (DCGP_CU_PARTITION=1, read at ctx creation: a fresh process): more workgroups
    than CUs, so some start when every producer has long left.  Exact ELBO, fused_rep_share = 0 against the default, synchronous and with two steps in flight."""
    import subprocess
    import sys
    code = r'''
import sys, ctypes as C, numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
from deepcgp_amd import synthetic as syn, device as dev
from deepcgp_amd.models import build_from_spec
spec, X, Y = syn.make_config("cfg2_mnist_CH_M256")
model = build_from_spec(spec, X, Y)
ctx = dev.get_context()
def plan():
    out = (C.c_int * 4)()
    assert dev.lib().dcgp_debug_fused_plan(ctx.handle, out) == 0
    return list(out)
out, plans = [], []
for share in (0, -1, -1, -1):
    with ctx.options(fused_rep_share=share):
        out.append(model.compute_log_likelihood(X, Y, seed=5))
        plans.append(plan())
        tickets = [model.enqueue_log_likelihood(X, Y, seed=5) for _ in range(2)]
        out += [model.collect_log_likelihood(t) for t in tickets]
print("RESULT", " ".join(repr(v) for v in out))
print("PLANS", repr(plans))
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env["DCGP_CU_PARTITION"] = "1"
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    vals = [float(v) for v in [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1].split()[1:]]
    plans = eval([ln for ln in r.stdout.splitlines() if ln.startswith("PLANS")][-1][6:])
    assert all(np.isfinite(vals)) and len(set(vals)) == 1, vals
    assert plans[0][3] == 0 and all(p[3] == 72 and p[1] == 720 for p in plans[1:]), plans

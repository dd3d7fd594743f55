"""Head rows riding the layer kernel's persistent launch (csrc/fused_plan.h: plan_head_ride; csrc/conv_fused.hip: HEAD; ctx option head_ride, -1 chosen / 0 never).

Where a conv layer is followed by the head, the layer's persistent launch deals the rows of the head's Kzx sweep behind its last strip item: a row waits for the
strips that cover its columns and runs the device code of head_units_kernel itself (csrc/head_units_dev.h), so every Kzx value is the same bits and ELBO, data
term and KL compare with assert-equal between head_ride = 0 and the chosen route.  The model is a conv layer on 28 x 28 x 1 (5 x 5, stride 2, R = 10: 144
patches, never a whole number of 64-column strips per row) and a head on 5 x 5 x 10 patches; fused_shape = 0 (64-column strips: so few columns would
otherwise get 32-column ones) and fused_persist = 1 with fused_wgs = 3 and 5 put the strips through several rounds on few workgroups, so that rows straddle strips whose workgroups are still running.  dcgp_debug_head_ride says whether the last
launch carried rows: a case that is meant to ride (or to fall back) cannot pass by doing the other.  Three steps per case: flag epochs and the device counter
return to their state.  Every case also agrees with the oracle to 1e-9."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HWC = (28, 28, 1)
CONV = (5, 2, 10)
HEAD = (5, 1)

_models, _oracle = {}, {}


def _model(M, S):
    """one model per (M, S) for the whole module"""
    if (M, S) not in _models:
        from deepcgp_amd import synthetic as syn
        from deepcgp_amd.models import build_from_spec
        spec = syn.make_spec(HWC, [CONV], HEAD, M=M, S=S, num_data=500, seed=31 + M, conv_q_sqrt_scale=0.3)
        X, Y = syn.make_batch(HWC, 4, seed=3)
        _models[(M, S)] = (spec, build_from_spec(spec, X, Y))
    return _models[(M, S)]


def _batch(M, N, S):
    from deepcgp_amd import synthetic as syn
    spec, model = _model(M, S)
    X, Y = syn.make_batch(HWC, N, seed=200 + N)
    zs = syn.make_noise(spec, N, seed=9)
    return spec, model, X, Y, zs


def _oracle_parts(M, N, S):
    """(ELBO, data term, KL) of the CPU oracle, once per case"""
    key = (M, N, S)
    if key not in _oracle:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from oracle_build import oracle_model
        spec, _, X, Y, zs = _batch(M, N, S)
        ref = oracle_model(spec, X, Y)
        _oracle[key] = (ref.compute_log_likelihood(X, Y, zs=zs), ref.data_term(X, Y, zs=zs), ref.KL())
    return _oracle[key]


def _rode(ctx):
    """(head rows the most recent layer-kernel launch carried, launches of the ctx that carried any)"""
    from deepcgp_amd import device as dev
    out = (C.c_longlong * 2)()
    assert dev.lib().dcgp_debug_head_ride(ctx.handle, out) == 0
    return out[0], out[1]


def _parts(model, X, Y, zs, S):
    assert zs[0].shape[0] == S == model.num_samples
    return model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)


def _planned_rows(ctx, M, N, S):
    """rows the planner (csrc/fused_plan.h through dcgp_debug_plan_head_ride) puts on layer 0's launch under the ctx's options of the moment"""
    import fused_plan_cases as fc
    from test_host_head_ride import ride
    q = fc.ctx_query(ctx, HWC, CONV[0], CONV[1], M, CONV[2], N * S, N)
    return ride(q, 0, head_HWC=144 * CONV[2], head_nfm=(M + 15) // 16, head_ride=ctx.get_option("head_ride"))["rows"]


@pytest.mark.parametrize("wgs", [3, 5])
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("M", [32, 48])
def test_head_rows_ride_and_give_the_same_bits(ctx, M, N, S, wgs):
    """head_ride = 0 against the chosen count (-1: what the deal's workgroups have room for), every row (a count past the rows) and one row short of all:
    rows in the layer launch, the others in the head's own"""
    spec, model, X, Y, zs = _batch(M, N, S)
    rows = N * S
    with ctx.options(fused_shape=0, fused_persist=1, fused_wgs=wgs):
        with ctx.options(head_ride=0):
            n0 = _rode(ctx)[1]
            ref = _parts(model, X, Y, zs, S)
            assert _rode(ctx) == (0, n0)                         # today's route: no launch carried a row
        print("head_ride=0:", ref)
        for how, want in ((-1, None), (1000, rows), (rows - 1, rows - 1)):
            with ctx.options(head_ride=how):
                want = _planned_rows(ctx, M, N, S) if want is None else want
                assert want == _planned_rows(ctx, M, N, S) and 0 <= want <= rows
                for rep in range(3):
                    n0 = _rode(ctx)[1]
                    got = _parts(model, X, Y, zs, S)
                    print("head_ride=%d (%d rows), step %d:" % (how, want, rep), got)
                    assert _rode(ctx) == (want, n0 + (1 if want else 0)), _rode(ctx)      # in the one layer launch of the step
                    assert all(np.isfinite(got))
                    assert got == ref, (got, ref)
    want = _oracle_parts(M, N, S)
    for g, w, what in zip(ref, want, ("elbo", "data term", "kl")):
        print(what, g, w)
        assert abs(g - w) <= 1e-9 * abs(g), (what, g, w)


def _falls_back(ctx, run, **options):
    """run() under head_ride = 0 and with every row asked for: the same bits, and no launch carried a row either time"""
    with ctx.options(**options):
        with ctx.options(head_ride=0):
            ref = run()
        with ctx.options(head_ride=1000):
            n0 = _rode(ctx)[1]
            got = run()
            assert _rode(ctx) == (0, n0), _rode(ctx)
    return got, ref


def test_a_launch_that_cannot_carry_rows_falls_back(ctx):
    """32-column strips on 8 waves, two workgroups per CU"""
    _, model, X, Y, zs = _batch(32, 3, 3)
    got, ref = _falls_back(ctx, lambda: _parts(model, X, Y, zs, 3), fused_shape=2, fused_persist=1, fused_wgs=3)
    with ctx.options(fused_shape=0, fused_persist=1, fused_wgs=3, head_ride=1000):
        assert got == ref and got == _parts(model, X, Y, zs, 3)  # ... and the same bits as the riding step
        assert _rode(ctx)[0] == 9


def test_steps_in_flight_fall_back(ctx):
    _, model, X, Y, zs = _batch(32, 3, 3)

    def run():
        tickets = [model.enqueue_log_likelihood(X, Y, zs=zs) for _ in range(2)]
        return [model.collect_log_likelihood(t, return_parts=True) for t in tickets]
    got, ref = _falls_back(ctx, run, fused_shape=0, fused_persist=1, fused_wgs=3)
    with ctx.options(fused_shape=0, fused_persist=1, fused_wgs=3, head_ride=1000):
        assert got == ref and got[0] == got[1] == _parts(model, X, Y, zs, 3)
        assert _rode(ctx)[0] == 9


def test_a_training_step_falls_back(ctx):
    _, model, X, Y, zs = _batch(32, 3, 3)

    def run():
        e, grads = model.compute_gradients(X, Y, zs=zs)
        return e, grads
    (e, grads), (e0, grads0) = _falls_back(ctx, run, fused_shape=0, fused_persist=1, fused_wgs=3)
    assert e == e0
    for g, g0 in zip(grads, grads0):
        for k in g0:
            np.testing.assert_array_equal(g[k], g0[k], err_msg=k)
    with ctx.options(fused_shape=0, fused_persist=1, fused_wgs=3, head_ride=1000):
        assert _parts(model, X, Y, zs, 3)[0] == e               # a forward step behind it rides again, same value
        assert _rode(ctx)[0] == 9


def test_dedup_layer0_falls_back(ctx):
    _, model, X, Y, zs = _batch(32, 3, 3)
    model.dedup_layer0 = True
    try:
        got, ref = _falls_back(ctx, lambda: _parts(model, X, Y, zs, 3), fused_shape=0, fused_persist=1, fused_wgs=3)
    finally:
        model.dedup_layer0 = False
    assert got == ref

"""The head's whole sweep in the layer kernel's persistent launch (csrc/fused_plan.h: plan_head_tail; csrc/conv_fused.hip: HEAD = 2; ctx option head_ride_tail,
-1 chosen / 0 never / 1 wherever the launch can carry it).

Behind the whole rows of plan_head_ride the launch's counter deals the rest of the head's sweep: one Kdiag item per row that rode whole, and sub-row items (a
part of the row's Z-fragment units, the last part also the row's Kdiag chunks) for the others.  Every value comes out of the device code of head_units_kernel
(csrc/head_units_dev.h) and every Kdiag partial sum lands in the slot, with the chunk boundaries, of the stand-alone launch's plan, so ELBO, data term and KL
compare with assert-equal against head_ride_tail = 0 (rows ride, the sweep launch runs the rest) and head_ride = 0 (nothing rides).  The model is that of
tests/test_gpu_head_ride.py -- a conv layer on 28 x 28 x 1 (5 x 5, stride 2, R = 10: 144 patches, never a whole number of 64-column strips per row) and a head
on 5 x 5 x 10 patches -- at M = 32 and 256 (2 and 16 Z fragments per row); fused_shape = 0, fused_persist = 1 and fused_wgs = 3 / 5 put the strips through
several rounds on few workgroups.  dcgp_debug_head_tail says what the last launch carried and how many sweep launches were skipped: a case that is meant to
carry the tail (or to fall back) cannot pass by doing the other.  Three steps per case: flag epochs and the device counter return to their state.  Every case
also agrees with the oracle to 1e-9."""
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
    """(head rows the most recent layer-kernel launch carried whole, launches of the ctx that carried any head item)"""
    from deepcgp_amd import device as dev
    out = (C.c_longlong * 2)()
    assert dev.lib().dcgp_debug_head_ride(ctx.handle, out) == 0
    return out[0], out[1]


def _tail(ctx):
    """(Kdiag items, sub-row items, parts of the most recent layer-kernel launch; head sweep launches the ctx has skipped)"""
    from deepcgp_amd import device as dev
    out = (C.c_longlong * 4)()
    assert dev.lib().dcgp_debug_head_tail(ctx.handle, out) == 0
    return tuple(out)


def _parts(model, X, Y, zs, S):
    assert zs[0].shape[0] == S == model.num_samples
    return model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)


def _planned_rows(ctx, M, N, S):
    """whole rows plan_head_ride puts on layer 0's launch under the ctx's options of the moment"""
    import fused_plan_cases as fc
    from test_host_head_ride import ride
    q = fc.ctx_query(ctx, HWC, CONV[0], CONV[1], M, CONV[2], N * S, N)
    return ride(q, 0, head_HWC=144 * CONV[2], head_nfm=(M + 15) // 16, head_ride=ctx.get_option("head_ride"))["rows"]


@pytest.mark.parametrize("wgs", [3, 5])
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("M", [32, 256])
def test_the_whole_sweep_rides_and_gives_the_same_bits(ctx, M, N, S, wgs):
    """head_ride_tail = 1 against head_ride_tail = 0 and head_ride = 0, with the whole rows the deal has room for (head_ride = -1) and with two forced"""
    spec, model, X, Y, zs = _batch(M, N, S)
    rows = N * S
    with ctx.options(fused_shape=0, fused_persist=1, fused_wgs=wgs):
        with ctx.options(head_ride=0, head_ride_tail=1):
            n0, k0 = _rode(ctx)[1], _tail(ctx)[3]
            ref = _parts(model, X, Y, zs, S)
            assert _rode(ctx) == (0, n0) and _tail(ctx) == (0, 0, 0, k0)      # nothing rides: the head's own sweep launch
        print("head_ride=0:", ref)
        for whole in (-1, 2):
            with ctx.options(head_ride=whole, head_ride_tail=0):
                k0 = _tail(ctx)[3]
                rows_only = _parts(model, X, Y, zs, S)
                print("head_ride=%d head_ride_tail=0:" % whole, rows_only)
                assert _tail(ctx) == (0, 0, 0, k0)                              # rows may ride, the sweep launch runs the rest
                assert rows_only == ref, (rows_only, ref)
            with ctx.options(head_ride=whole, head_ride_tail=1):
                want = _planned_rows(ctx, M, N, S)
                assert 0 <= want <= rows and (whole < 0 or want == whole)
                for rep in range(3):
                    n0, k0 = _rode(ctx)[1], _tail(ctx)[3]
                    got = _parts(model, X, Y, zs, S)
                    print("head_ride=%d head_ride_tail=1 (%d whole rows), step %d:" % (whole, want, rep), got, _tail(ctx))
                    assert _rode(ctx) == (want, n0 + 1), _rode(ctx)
                    assert _tail(ctx) == (want, (rows - want) * 2, 2, k0 + 1), _tail(ctx)      # every other row as two parts; no sweep launch
                    assert all(np.isfinite(got))
                    assert got == ref, (got, ref)
    want = _oracle_parts(M, N, S)
    for g, w, what in zip(ref, want, ("elbo", "data term", "kl")):
        print(what, g, w)
        assert abs(g - w) <= 1e-9 * abs(g), (what, g, w)


def test_four_parts_per_row_give_the_same_bits(ctx):
    """M = 256: 16 Z fragments as four items of four units; the row's Kdiag chunks behind the last"""
    _, model, X, Y, zs = _batch(256, 3, 3)
    with ctx.options(fused_shape=0, fused_persist=1, fused_wgs=5):
        with ctx.options(head_ride_tail=0):
            ref = _parts(model, X, Y, zs, 3)
        with ctx.options(head_ride=1, head_ride_tail=4):
            k0 = _tail(ctx)[3]
            got = _parts(model, X, Y, zs, 3)
            assert _tail(ctx) == (1, 8 * 4, 4, k0 + 1), _tail(ctx)
    assert got == ref, (got, ref)


def _falls_back(ctx, run, **options):
    """run() under head_ride_tail = 0 and with the tail asked for: the same bits, no launch carried a tail item and no sweep launch was skipped"""
    with ctx.options(**options):
        with ctx.options(head_ride_tail=0):
            ref = run()
        with ctx.options(head_ride_tail=1):
            n0, k0 = _rode(ctx)[1], _tail(ctx)[3]
            got = run()
            assert _rode(ctx) == (0, n0), _rode(ctx)
            assert _tail(ctx) == (0, 0, 0, k0), _tail(ctx)
    return got, ref


def _rides_again(ctx, model, X, Y, zs):
    """... and a plain forward step behind it carries the tail again"""
    with ctx.options(fused_shape=0, fused_persist=1, fused_wgs=3, head_ride_tail=1):
        k0 = _tail(ctx)[3]
        got = _parts(model, X, Y, zs, 3)
        assert _tail(ctx)[2:] == (2, k0 + 1), _tail(ctx)
    return got


def test_steps_in_flight_fall_back(ctx):
    _, model, X, Y, zs = _batch(32, 3, 3)

    def run():
        tickets = [model.enqueue_log_likelihood(X, Y, zs=zs) for _ in range(2)]
        return [model.collect_log_likelihood(t, return_parts=True) for t in tickets]
    got, ref = _falls_back(ctx, run, fused_shape=0, fused_persist=1, fused_wgs=3)
    assert got == ref and got[0] == got[1] == _rides_again(ctx, model, X, Y, zs)


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
    assert _rides_again(ctx, model, X, Y, zs)[0] == e


def test_dedup_layer0_falls_back(ctx):
    _, model, X, Y, zs = _batch(32, 3, 3)
    model.dedup_layer0 = True
    try:
        got, ref = _falls_back(ctx, lambda: _parts(model, X, Y, zs, 3), fused_shape=0, fused_persist=1, fused_wgs=3)
    finally:
        model.dedup_layer0 = False
    assert got == ref


def test_a_trace_falls_back(ctx):
    """phase stamps on (dcgp_debug_set_fused_trace): the launch is the traced one, without head items"""
    from deepcgp_amd import device as dev
    _, model, X, Y, zs = _batch(32, 3, 3)
    buf = ctx.to_device(np.zeros((32, 16, 16), np.int64), np.int64)
    assert dev.lib().dcgp_debug_set_fused_trace(ctx.handle, buf.ptr) == 0
    try:
        got, ref = _falls_back(ctx, lambda: _parts(model, X, Y, zs, 3), fused_shape=0, fused_persist=1, fused_wgs=3)
    finally:
        assert dev.lib().dcgp_debug_set_fused_trace(ctx.handle, None) == 0
    assert got == ref == _rides_again(ctx, model, X, Y, zs)

"""The launch plan of the one-launch conv layer kernel (csrc/fused_plan.h: plan_layer_launch), pinned down without a GPU through
dcgp_debug_plan_layer_launch.

tests/fused_plan_table.json holds the answers of the planning functions this header replaced (plan_fused, last_round, plan_parts, plan_prologues,
plan_rep_share and the decision part of conv_fused()), recorded from a stand-alone build of them before they were removed: every field of every plan, and the
makespans of the simulated deals to the last bit.  The queries are those of fused_plan_cases.table_cases()."""
import json
import os
import shutil
import subprocess

import pytest

import fused_plan_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table():
    with open(os.path.join(ROOT, "tests", "fused_plan_table.json")) as fh:
        return json.load(fh)


def test_recorded_plans_are_reproduced_exactly():
    rows = _table()
    cases = fc.table_cases()
    assert [(r["name"], r["query"]) for r in rows] == [(n, q) for n, q in cases]     # the table is the table of these queries
    assert len(rows) > 120
    for r in rows:
        got = fc.plan(r["query"])
        if not r["plan"]["ok"]:
            assert got["ok"] == 0, r["name"]
            continue
        assert set(r["plan"]) == set(fc.PLAN_FIELDS)
        assert got == r["plan"], (r["name"], {k: (v, got[k]) for k, v in r["plan"].items() if got[k] != v})


def _named(name):
    return fc.plan(dict(fc.table_cases())[name])


def test_headline_layer_and_its_options():
    """cfg2's first layer: 720 strips of 64 columns on 256 CUs, 72 of them distinct"""
    p = _named("cfg2")
    assert (p["shape"], p["grid"], p["persist"], p["deal"], p["n_strips"], p["n_items"]) == (0, 256, 256, 1, 720, 720)
    assert (p["pre_D"], p["pre_n"], p["pre_whole"], p["pre_first"]) == (72, 72, 256, 0)
    assert (p["units_plain"], p["units_ahead"], p["units_shared"]) == pytest.approx((36.15, 34.60, 33.25), abs=1e-9)
    p = _named("cfg2 fused_rep_share=0")
    assert (p["pre_D"], p["pre_n"], p["pre_first"], p["n_items"]) == (0, 224, 720 % 256, 720 + 224)
    assert _named("cfg2 fused_pre=0")["pre_n"] == 0
    assert _named("cfg2 fused_pre=9")["pre_n"] == 224 and _named("cfg2 fused_pre=3")["pre_n"] == 32
    assert _named("cfg2 fused_persist=0")["persist"] == 0 and _named("cfg2 fused_persist=0")["grid"] == 720
    assert _named("cfg2 fused_persist=2")["deal"] == 2 and _named("cfg2 fused_persist=2")["pre_n"] == 0      # the fixed deal hands nothing over
    assert _named("cfg2 keeps_state")["persist"] == 0                                                          # the training step: one workgroup per strip
    assert _named("Kc=1<<23")["ok"] == 0 and _named("Kc=(1<<23)-16")["ok"] == 1
    assert _named("M=384 fused_large=0")["ok"] == 0 and _named("M=384 fused_large=1")["shape"] == 4
    assert _named("long patches")["patch_rows"] == 1 and _named("long patches sweep_no_rows")["patch_rows"] == 0


@pytest.mark.parametrize("strips,slots,R,n_mod,D,ahead,units", [
    (12, 4, 3, 4, 4, 0, (15.15, 0.0, 12.25)),
    (9, 4, 3, 3, 3, 5, (15.15, 12.45, 12.05)),
    (10, 4, 2, 5, 5, 2, (12.15, 10.60, 9.25)),
    (17, 4, 10, 17, 0, 13, (60.25, 54.05, 0.0)),
])
def test_simulated_deal_on_small_launches(strips, slots, R, n_mod, D, ahead, units):
    """`strips` 16-column strips of `n_mod` images on `slots` workgroups: plain / prologues ahead / shared makespans (0: not simulated), the shared D
    and the prologues ahead that the launch would run without sharing"""
    q = fc.layer_query(fc.SMALL, 5, 2, 32, R, strips, n_mod, 256, fused_shape=6, fused_persist=1, fused_wgs=slots)
    p = fc.plan(q)
    assert (p["units_plain"], p["units_ahead"], p["units_shared"]) == pytest.approx(units, abs=1e-9)
    assert p["pre_D"] == D and p["persist"] == slots
    q0 = fc.layer_query(fc.SMALL, 5, 2, 32, R, strips, n_mod, 256, fused_shape=6, fused_persist=1, fused_wgs=slots, fused_rep_share=0)
    assert fc.plan(q0)["pre_n"] == ahead and fc.plan(q0)["pre_D"] == 0


def test_parts_on_a_four_image_shard():
    """90 strips of 64 columns on 256 CUs at R = 10, two teams: 8.45 units as two parts, 6.95 as five (which the simulated deal picks), against 12.05 for
    one workgroup per strip with no strip shared"""
    def shard(**kw):
        return fc.plan(fc.layer_query(fc.MNIST, 5, 2, 256, 10, 40, 4, 256, fused_shape=0, **kw))
    p2, p5, chosen = shard(fused_parts=2, fused_split=0), shard(fused_parts=5, fused_split=0), shard(fused_parts=-2, fused_split=0)
    assert (p2["units_plain"], p2["units_ahead"]) == pytest.approx((12.05, 8.45), abs=1e-9)
    assert (p5["units_plain"], p5["units_ahead"]) == pytest.approx((12.05, 6.95), abs=1e-9)
    assert (p2["pre_sq"], p5["pre_sq"], chosen["pre_sq"]) == (2, 5, 5)
    for p in (p2, p5):
        assert (p["persist"], p["pre_n"], p["pre_first"], p["n_items"]) == (256, 90, 0, 90 + 90 * p["pre_sq"])
    off = shard()
    assert off["persist"] == 0 and off["split_q"] == 2 and off["grid"] == 180          # parts stay off by default: the last round is shared instead


@pytest.mark.parametrize("M,R,N,S,shape,wgs,units", [(256, 10, 8, 4, 0, 3, (33.25, 33.05)), (32, 10, 4, 4, 0, 3, (22.55, 22.55))])
def test_the_simulated_deal_keeps_prologues_ahead_where_they_do_as_well(M, R, N, S, shape, wgs, units):
    """tests/test_gpu_fused_rep_share.py, the test of the same name: the shared deal is no shorter than the prologues ahead, and the launch stays as it is"""
    p = fc.plan(fc.rep_share_query(M, R, N, S, shape, wgs))
    assert (p["units_shared"], p["units_ahead"]) == pytest.approx(units, abs=1e-9)
    assert p["pre_D"] == 0 and p["pre_n"] > 0
    assert p == dict(fc.plan(fc.rep_share_query(M, R, N, S, shape, wgs, fused_rep_share=0)), units_shared=p["units_shared"])


@pytest.mark.parametrize("case", fc.REP_SHARE_CASES)
def test_expected_D_of_the_gpu_cases(case):
    """what tests/test_gpu_fused_rep_share.py expects dcgp_debug_fused_plan to say after its launches"""
    M, R, N, S, shape, wgs, D = case
    strips = (N * S * 16 + (16 if shape == 6 else 64) - 1) // (16 if shape == 6 else 64)
    p = fc.plan(fc.rep_share_query(M, R, N, S, shape, wgs))
    assert p["persist"] == wgs and p["pre_D"] == D and p["n_strips"] == strips
    if D:
        assert fc.debug_plan_of(p) == (wgs, strips, D, D)
    assert fc.plan(fc.rep_share_query(M, R, N, S, shape, wgs, fused_rep_share=0))["pre_D"] == 0


def _items(p):
    """The items of a persistent launch with a hand-over in the order the counter deals them, as the kernel decodes them:
    (strip, part, slot written or None, slot read or None)"""
    out = []
    for t in range(p["n_items"]):
        if p["pre_D"] > 0:
            out.append((t, None, t if t < p["pre_D"] else None, t % p["pre_D"] if t >= p["pre_whole"] else None))
        elif t >= p["n_strips"]:
            slot, part = divmod(t - p["n_strips"], p["pre_sq"])
            out.append((p["pre_first"] + slot, part if p["pre_sq"] > 1 else None, None, slot))
        elif p["pre_first"] <= t < p["pre_first"] + p["pre_n"]:
            out.append((None, None, t - p["pre_first"], None))                  # a prologue only: its strip comes as a later item
        else:
            out.append((t, None, None, None))
    return out


def _check_properties(p):
    assert p["ok"] == 1
    if p["pre_D"] > 0:
        assert p["n_items"] == p["n_strips"]
        assert p["pre_n"] == p["pre_D"] and p["pre_first"] == 0 and p["pre_D"] < p["n_strips"] and p["pre_whole"] >= p["pre_D"]
    else:
        assert p["n_items"] == p["n_strips"] + p["pre_n"] * p["pre_sq"]
        if p["pre_sq"] == 1 and p["pre_n"] > 0:
            assert p["pre_first"] == p["n_strips"] % p["persist"]
    if p["pre_n"] == 0:
        return
    assert p["persist"] > 0 and p["deal"] == 1 and p["pre_stride"] > 0
    written, done = {}, {}
    for t, (strip, part, wr, rd) in enumerate(_items(p)):
        if wr is not None:
            assert 0 <= wr < p["pre_n"] and wr not in written
            written[wr] = t
        if rd is not None:
            assert rd in written and written[rd] < t                              # a slot's writer is dealt before every one of its readers
        if strip is not None:
            done.setdefault(strip, []).append(part)
    want = [None] if p["pre_sq"] == 1 else list(range(p["pre_sq"]))
    handed = range(p["pre_first"], p["pre_first"] + p["pre_n"]) if p["pre_D"] == 0 else ()
    assert sorted(done) == list(range(p["n_strips"]))                          # every strip is run, once, whole or in all its parts
    assert all(sorted(v, key=lambda x: -1 if x is None else x) == (want if s in handed else [None]) for s, v in done.items())


def test_header_stands_alone_and_its_grid_has_the_properties(tmp_path):
    """tests/fused_plan_grid.cc includes the header and nothing else of the project: built here with the host compiler, it plans the grid (strips 1..40 x
    workgroups 1..8 x R in {1, 2, 3, 10} x every tiling of the rows x the deal forced persistent, chosen, and with parts) and the library must give the same
    answers.  Properties of every plan: the item count, the layout of the shared plan, where the prologues ahead begin, every slot written before it is read,
    every strip run exactly once, and the memo returning what it returned before."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fused_plan_grid")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "deepcgp_amd", "csrc"),
                    os.path.join(ROOT, "tests", "fused_plan_grid.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    want_queries = set()
    for strips in range(1, 41):
        for wgs in range(1, 9):
            for R in (1, 2, 3, 10):
                for n_mod in [d for d in range(1, strips + 1) if strips % d == 0]:
                    for persist, parts in ((1, -1), (-1, -1), (-1, 3)):
                        want_queries.add(tuple(fc.layer_query(fc.SMALL, 5, 2, 32, R, strips, n_mod, 256, fused_shape=6, fused_persist=persist, fused_wgs=wgs,
                                                              fused_parts=parts)))
    assert len(lines) == len(want_queries)
    kinds = set()
    first = {}
    for ln in lines:
        qs, ps = ln.split("|")
        q = [int(x) for x in qs.split()]
        assert tuple(q) in want_queries
        w = ps.split()
        alone = {k: (float(x) if k in fc.UNITS else int(x)) for k, x in zip(fc.PLAN_FIELDS, w)}
        p = fc.plan(q)
        assert p == alone, (q, p, alone)
        assert fc.plan(q) == p
        first[tuple(q)] = p
        _check_properties(p)
        kinds.add((p["deal"], p["pre_D"] > 0, p["pre_sq"] > 1, p["pre_n"] > 0, p["split_q"] > 1))
    # the grid reaches every way of dealing a launch that the planner has, bar the fixed stride (an A/B switch)
    assert {(0, False, False, False, False), (0, False, False, False, True), (1, False, False, False, False), (1, False, False, True, False),
            (1, True, False, True, False), (1, False, True, True, False)} <= kinds
    for q, p in list(first.items())[:300]:          # (the memo is bounded: these were dropped from it long ago and are planned afresh)
        assert fc.plan(list(q)) == p


def test_flat_arrays_of_the_wrong_length_are_refused():
    import ctypes as C
    from deepcgp_amd import device as dev
    q = (C.c_longlong * 29)(*fc.table_cases()[0][1])
    out = (C.c_longlong * 24)()
    assert dev.lib().dcgp_debug_plan_layer_launch(q, 28, out, 24) != 0
    assert dev.lib().dcgp_debug_plan_layer_launch(q, 29, out, 23) != 0
    assert dev.lib().dcgp_debug_plan_layer_launch(q, 29, out, 24) == 0 and out[0] == 1

"""Whether a layer launch carries the head's whole sweep, and what its tail items are (csrc/fused_plan.h: plan_head_tail, through dcgp_debug_plan_head_tail).
No device needed."""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

import fused_plan_cases as fc
from test_host_head_ride import RIDE_FIELDS, WHY, headline, ride

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL_FIELDS = ("head_ride_tail", "n_kd")
OUT_FIELDS = ("ok", "why", "rows", "parts", "upp", "first_item", "items", "row", "kz_lo", "kz_hi", "kd", "strip_lo", "strip_hi", "last_writer")
TAIL_WHY = dict(rides=0, off=1, no_ride=2, geometry=3, few_workgroups=4, no_gain=5)


def tail(query, item=0, head_ride_tail=1, n_kd=4, **kw):
    from deepcgp_amd import device as dev
    r = dict(next_is_head=1, head_form=1, head_HWC=1440, head_lds=16 * 1024, head_nfm=16, in_flight=0, chain_beside=0, head_ride=-1)
    assert set(kw) <= set(r), kw
    r.update(kw)
    qa = (C.c_longlong * len(query))(*query)
    ra = (C.c_longlong * len(RIDE_FIELDS))(*[r[k] for k in RIDE_FIELDS])
    ta = (C.c_longlong * len(TAIL_FIELDS))(head_ride_tail, n_kd)
    out = (C.c_longlong * len(OUT_FIELDS))()
    assert dev.lib().dcgp_debug_plan_head_tail(qa, len(query), ra, len(RIDE_FIELDS), ta, len(TAIL_FIELDS), item, out, len(OUT_FIELDS)) == 0
    return dict(zip(OUT_FIELDS, out))


@pytest.mark.parametrize("parts", [1, 2, 4])
def test_headline_tail_covers_every_unit_and_every_rows_kdiag_chunks_once(parts):
    """cfg2's conv layer: 144 whole rows (plan_head_ride's count, as pinned by tests/test_host_head_ride.py), then 144 Kdiag items and `parts` sub-row items
    for each of the other 176 rows; head_ride_tail = 1 leaves the parts to the planner (two)"""
    q = headline()
    p = fc.plan(q)
    t0 = tail(q, 0, head_ride_tail=parts)
    want_parts = 2 if parts == 1 else parts
    assert (t0["ok"], t0["why"], t0["rows"], t0["parts"], t0["upp"]) == (1, 0, 144, want_parts, 16 // want_parts)
    assert t0["first_item"] == p["n_items"] + 144 == 720 + 144 and t0["items"] == 144 + 176 * want_parts
    units, kd = {}, {}
    for i in range(t0["items"]):
        t = tail(q, i, head_ride_tail=parts)
        item = t["first_item"] + i
        assert item >= p["n_items"] + t["rows"]                                   # behind the last strip item and the whole rows
        assert (t["strip_lo"], t["strip_hi"]) == (t["row"] * 144 // 64, (t["row"] * 144 + 143) // 64)
        assert 0 <= t["last_writer"] < p["n_items"] <= item                       # the row's last writer strip is an earlier item
        assert (t["kz_hi"] - t["kz_lo"]) + (4 if t["kd"] else 0) <= 16            # one wave each
        for u in range(t["kz_lo"], t["kz_hi"]):
            units[(t["row"], u)] = units.get((t["row"], u), 0) + 1
        kd[t["row"]] = kd.get(t["row"], 0) + t["kd"]
    assert units == {(row, u): 1 for row in range(144, 320) for u in range(16)}
    assert kd == {row: 1 for row in range(320)}
    assert tail(q, t0["items"], head_ride_tail=parts)["row"] == -1


def test_forced_row_counts_move_the_boundary():
    q = headline()
    assert [tail(q, 0, head_ride=k)[f] for k in (96, 320) for f in ("rows", "items")] == [96, 96 + 224 * 2, 320, 320]
    t = tail(q, 319, head_ride=320)
    assert (t["row"], t["kz_lo"], t["kz_hi"], t["kd"]) == (319, 0, 0, 1)


def test_a_launch_with_no_room_for_a_whole_row_still_carries_the_tail():
    q = fc.layer_query(fc.MNIST, 5, 2, 256, 10, 4, 2, 256, fused_shape=0, fused_persist=1, fused_wgs=3)      # 9 strips on 3 workgroups: whole rounds
    assert ride(q, 0)["why"] == WHY["no_room"]
    t = tail(q, 0, head_nfm=2)
    assert (t["ok"], t["rows"], t["parts"], t["upp"], t["first_item"], t["items"]) == (1, 0, 2, 1, 9, 8)
    assert [tuple(tail(q, i, head_nfm=2)[k] for k in ("row", "kz_lo", "kz_hi", "kd")) for i in range(4)] == [(0, 0, 1, 0), (0, 1, 2, 1), (1, 0, 1, 0), (1, 1, 2, 1)]


def test_chosen_only_with_a_workgroup_on_every_cu():
    q = fc.layer_query(fc.MNIST, 5, 2, 256, 10, 4, 2, 256, fused_shape=0, fused_persist=1, fused_wgs=3)
    t = tail(q, 0, head_ride_tail=-1, head_nfm=2)
    assert (t["ok"], t["why"], t["items"]) == (0, TAIL_WHY["few_workgroups"], 0)
    t = tail(headline(), 0, head_ride_tail=-1)                                   # the headline: the simulated deal has the tail ahead, as halves
    assert (t["ok"], t["why"], t["rows"], t["parts"], t["items"]) == (1, 0, 144, 2, 176 * 2 + 144)
    assert ride(headline(), 0)["rows"] == 144                                    # ... behind the whole rows plan_head_ride gives, as it gave them


@pytest.mark.parametrize("why,query_kw,ride_kw", [
    ("off", {}, dict(head_ride=0)),
    ("not_head", {}, dict(next_is_head=0)),
    ("form", {}, dict(head_form=0)),
    ("launch", dict(fused_shape=2, fused_persist=1), {}),
    ("launch", dict(fused_persist=2), {}),
    ("launch", dict(fused_persist=0), {}),
    ("launch", dict(rep=10), {}),
    ("launch", dict(base="acos"), {}),
    ("state", dict(keeps_state=1, fused_persist=1), {}),
    ("trace", dict(has_trace=1, fused_persist=1), {}),
    ("in_flight", {}, dict(in_flight=1)),
    ("in_flight", {}, dict(chain_beside=1)),
    ("geometry", {}, dict(head_HWC=1441)),
    ("geometry", {}, dict(head_nfm=17)),
    ("geometry", {}, dict(head_lds=200 * 1024)),
])
def test_ineligible_queries_give_no_tail(why, query_kw, ride_kw):
    """the `why` list of tests/test_host_head_ride.py: whatever keeps the rows off the launch keeps the tail off it, forced or chosen"""
    q = headline(**query_kw)
    assert ride(q, 0, **ride_kw)["why"] == WHY[why]
    for how in (1, 2, -1):
        t = tail(q, 0, head_ride_tail=how, **ride_kw)
        assert (t["ok"], t["why"], t["rows"], t["items"], t["row"]) == (0, TAIL_WHY["no_ride"], 0, 0, -1), t
    assert tail(headline(), 0, head_ride_tail=0)["why"] == TAIL_WHY["off"]
    assert tail(headline(), 0, n_kd=0)["why"] == TAIL_WHY["geometry"]            # a sweep without Kdiag chunks
    assert tail(headline(), 0, n_kd=17)["why"] == TAIL_WHY["geometry"]


def test_plan_head_ride_answers_what_it_answered():
    """tests/golden/head_ride_answers.json: plan_head_ride over the grid of tests/fused_plan_cases.py (chosen count, and every row asked for), recorded
    before the tail was added"""
    with open(os.path.join(ROOT, "tests", "golden", "head_ride_answers.json")) as f:
        want = json.load(f)
    cases = fc.table_cases()
    assert len(want) == len(cases)
    for (name, q), (wname, answers) in zip(cases, want):
        assert name == wname
        head_HWC = q[fc.QUERY_FIELDS.index("P")] * q[fc.QUERY_FIELDS.index("R")]      # a head row is the layer's output of one image
        got = [[ride(q, 0, head_ride=how, head_HWC=head_HWC)[k] for k in ("ok", "why", "rows", "first_item")] for how in (-1, 1000)]
        assert got == answers, name


def test_header_stands_alone_and_the_tail_has_the_properties(tmp_path):
    """tests/head_tail_grid.cc includes csrc/fused_plan.h alone: built with the host compiler under the address and undefined-behaviour sanitizers and run
    as a program, it checks for every query of its grid that carries a tail that every unit and every row's Kdiag chunks are run exactly once, that tail items
    sit behind the strips and their rows' writers are earlier items, and that ineligible queries carry none; the library must give the same answers."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "head_tail_grid")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "deepcgp_amd", "csrc"),
                    os.path.join(ROOT, "tests", "head_tail_grid.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 12 * 4 * 2 * 3 * 6 * 12 + 12
    riding = 0
    for ln in lines[::11] + lines[-12:]:                      # every eleventh query, and the headline's, through the library as well
        qs, rs, ts, outs = (part.split() for part in ln.split("|"))
        want = [int(v) for v in outs]
        got = tail([int(v) for v in qs], 0, head_ride_tail=int(ts[0]), n_kd=int(ts[1]), **dict(zip(RIDE_FIELDS, (int(v) for v in rs))))
        assert [got[k] for k in ("ok", "why", "rows", "parts", "upp", "first_item", "items")] == want, ln
        riding += want[0]
    assert riding > 0

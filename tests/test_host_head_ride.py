"""Whether a layer launch carries the head's rows, and where they sit in its deal (csrc/fused_plan.h: plan_head_ride, through dcgp_debug_plan_head_ride).
No device needed."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import fused_plan_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RIDE_FIELDS = ("next_is_head", "head_form", "head_HWC", "head_lds", "head_nfm", "in_flight", "chain_beside", "head_ride")
OUT_FIELDS = ("ok", "why", "rows", "first_item", "item", "strip_lo", "strip_hi", "last_writer")
WHY = dict(rides=0, off=1, not_head=2, form=3, launch=4, state=5, trace=6, in_flight=7, geometry=8, no_room=9)


def ride(query, row=0, **kw):
    from deepcgp_amd import device as dev
    r = dict(next_is_head=1, head_form=1, head_HWC=1440, head_lds=16 * 1024, head_nfm=16, in_flight=0, chain_beside=0, head_ride=-1)
    assert set(kw) <= set(r), kw
    r.update(kw)
    qa = (C.c_longlong * len(query))(*query)
    ra = (C.c_longlong * len(RIDE_FIELDS))(*[r[k] for k in RIDE_FIELDS])
    out = (C.c_longlong * len(OUT_FIELDS))()
    assert dev.lib().dcgp_debug_plan_head_ride(qa, len(query), ra, len(RIDE_FIELDS), row, out, len(OUT_FIELDS)) == 0
    return dict(zip(OUT_FIELDS, out))


def headline(**kw):
    """cfg2's conv layer: 320 rows of 144 patches, 720 strips of 64 columns on 256 CUs"""
    return fc.layer_query(fc.MNIST, 5, 2, 256, 10, 320, 32, 256, **kw)


def test_headline_launch_carries_the_rows_its_spare_workgroups_have_room_for():
    """720 strips on 256 workgroups: 48 of them are done a fetched strip (10.5 units) ahead of the others, room for three rows of 3 units each"""
    q = headline()
    p = fc.plan(q)
    assert (p["n_items"], p["pre_D"], p["pre_whole"]) == (720, 72, 256)      # the recorded plan, as it was
    for row in (0, 1, 95, 143):
        r = ride(q, row)
        assert (r["ok"], r["why"], r["rows"], r["first_item"], r["item"]) == (1, 0, 144, 720, 720 + row)
        assert (r["strip_lo"], r["strip_hi"]) == (row * 144 // 64, (row * 144 + 143) // 64)
        assert r["last_writer"] == r["strip_hi"] < 720                         # one item per strip: the strip's own
    assert ride(q, 144)["last_writer"] == -1
    assert ride(q, 319, head_ride=1000)["rows"] == 320 and ride(q, 319, head_ride=1000)["item"] == 720 + 319
    assert ride(q, 0, head_ride=7)["rows"] == 7


def test_whole_rounds_leave_no_room():
    q = fc.layer_query(fc.MNIST, 5, 2, 256, 10, 4, 2, 256, fused_shape=0, fused_persist=1, fused_wgs=3)      # 9 strips on 3 workgroups
    assert fc.plan(q)["pre_n"] == 0
    r = ride(q, 0)
    assert (r["ok"], r["why"], r["rows"]) == (0, WHY["no_room"], 0)
    assert ride(q, 0, head_ride=4)["rows"] == 4


@pytest.mark.parametrize("why,query_kw,ride_kw", [
    ("off", {}, dict(head_ride=0)),
    ("not_head", {}, dict(next_is_head=0)),
    ("form", {}, dict(head_form=0)),
    ("launch", dict(fused_shape=2, fused_persist=1), {}),       # 32-column strips on 8 waves
    ("launch", dict(fused_persist=2), {}),                      # a fixed-stride deal
    ("launch", dict(fused_persist=0), {}),                      # one workgroup per strip
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
def test_ineligible_queries_say_so(why, query_kw, ride_kw):
    r = ride(headline(**query_kw), 0, **ride_kw)
    assert (r["ok"], r["why"], r["rows"], r["last_writer"]) == (0, WHY[why], 0, -1), r


def test_prologues_ahead_write_a_strips_samples_from_their_consumer_item():
    """fused_rep_share = 0 at the headline: 720 strips + 256 prologues ahead = 976 items, the head rows behind them; a strip whose prologue ran ahead has
    its samples written by the item that fetches it"""
    q = headline(fused_rep_share=0)
    p = fc.plan(q)
    assert p["pre_n"] > 0 and p["pre_D"] == 0 and p["n_items"] == 720 + p["pre_n"]
    first, n_pre = p["pre_first"], p["pre_n"]
    row = (first * 64) // 144 + 1            # a row inside the handed-over strips
    r = ride(q, row, head_ride=320)
    assert r["ok"] == 1 and r["first_item"] == p["n_items"] and first <= r["strip_lo"] and r["strip_hi"] < first + n_pre
    assert r["last_writer"] == 720 + (r["strip_hi"] - first) < r["item"]


def test_header_stands_alone_and_the_item_order_has_the_properties(tmp_path):
    """tests/head_ride_grid.cc includes csrc/fused_plan.h alone: built with the host compiler, it walks (rows, patches per row, strip shape, workgroups, kind
    of step), checks for every riding query that each row is one item, that the strips of a row are earlier items and that ineligible queries say why, and
    the library must give the same answers."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "head_ride_grid")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "deepcgp_amd", "csrc"), os.path.join(ROOT, "tests", "head_ride_grid.cc"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 12 * 4 * 2 * 3 * 6 * 10
    riding = 0
    for ln in lines[::7]:                      # every seventh query through the library as well
        qs, rs, outs = (part.split() for part in ln.split("|"))
        want = [int(v) for v in outs]
        got = ride([int(v) for v in qs], 0, **dict(zip(RIDE_FIELDS, (int(v) for v in rs))))
        assert [got["ok"], got["why"], got["rows"], got["first_item"]] == want, ln
        riding += want[0]
    assert riding > 0

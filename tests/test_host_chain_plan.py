"""The launch arithmetic of the factorisation chain (csrc/chain_plan.h: plan_launch, decode_iso, decode_rhs -- the functions factor_inverse_batched and
chol_rl_kernel themselves call) without a GPU, through dcgp_debug_plan_chain: every workgroup of every launch of an enumerated table of chains is decoded
and counted, and every case of tests/chain_cases.py is on the configuration it declares.

What an item does with its rows is rhs_tile's (csrc/chol_fused.hip) and is written down here once more, in `finals`: an item of the lagged panel p makes the
rows of panel p final in its column tile when it is its row group 0; in the last launch that same item goes on to make the last panel's rows final, and
the final_only item does so for the last panel's diagonal tile (alpha: for a one-panel matrix)."""
import ctypes as C

import numpy as np
import pytest

import chain_cases as cc
from chain_cases import DIAG_ONLY, EXIT, INVERSE, LOOKAHEAD, RHS, TRAILING

RIDE_MPS = tuple(range(16, 257, 16))
PLAIN_MPS = RIDE_MPS + (384, 1008, 1024)
MAX_RS = (1, 3, 10, 32)


def table_batch(batch, max_R):
    """(R, carries) per matrix: a matrix of smaller R first, the largest R second, one that carries nothing third; a batch of one has the largest R"""
    small = max(1, max_R // 3)
    pattern = [(small, True), (max_R, True), (max_R, False), (max_R, True), (small, True), (max_R, False), (max_R, True), (small, True)]
    return [(max_R, True)] if batch == 1 else pattern[:batch]


def check_coverage(p, wgs, batch):
    """every (b, bx) of the 2-D grid exactly once; on the isolated grid the look-ahead item on the slots (lin + 1) & 7 == 0 and nothing else there"""
    per = max(p["gx"], 1)
    live = wgs[:, 0] >= 0
    b, bx = wgs[live, 0], wgs[live, 1]
    assert np.all((b < batch) & (bx >= 0) & (bx < per))
    count = np.bincount(b * per + bx, minlength=batch * per)
    assert count.shape == (batch * per,) and np.all(count == 1), (p, np.flatnonzero(count != 1)[:8])
    lin = np.arange(len(wgs))
    if p["iso"]:
        assert p["grid_y"] == 1 and p["grid_x"] % 8 == 0 and p["iso_per"] == per - (p["la_idx"] >= 0)
        la_slot = ((lin + 1) & 7) == 0
        is_la = live & (wgs[:, 1] == p["la_idx"]) if p["la_idx"] >= 0 else np.zeros(len(wgs), bool)
        assert np.all(is_la <= la_slot), "a look-ahead workgroup off its XCD"
        assert np.all(~(la_slot & live) | is_la), "another item on the look-ahead XCD"
        assert np.all(wgs[is_la, 2] == LOOKAHEAD)
        # the look-ahead workgroup of matrix b is the one of slot b
        assert np.array_equal(wgs[is_la, 0], lin[is_la] >> 3)
    else:
        assert (p["grid_x"], p["grid_y"]) == (per, batch) and np.all(live)
        assert np.array_equal(wgs[:, 0], lin // per) and np.array_equal(wgs[:, 1], lin % per)
    # kinds by position in a matrix's row
    k = wgs[live, 2]
    if p["la_idx"] >= 0:
        assert np.all((k == LOOKAHEAD) == (bx == p["la_idx"]))
    n_chain = p["nT"] + (1 + p["nt"]) * p["nct"]
    if p["gx"] == 0:
        assert np.all(k == DIAG_ONLY) and len(k) == batch
    else:
        assert np.all((k == TRAILING) == (bx < p["nT"]))
        inv = k == INVERSE
        assert np.all(inv == ((bx >= p["nT"]) & (bx < n_chain)))
        if inv.any():      # every (row tile -1 .. nt - 1, column tile) once per matrix
            key = (b[inv] * (1 + p["nt"]) + wgs[live, 3][inv] + 1) * p["nct"] + wgs[live, 4][inv]
            assert np.all(np.bincount(key, minlength=batch * (1 + p["nt"]) * p["nct"]) == 1)
    if p["has_rhs"]:
        assert np.all(np.isin(k[bx >= p["rhs_base"]], (RHS, EXIT))) and np.all(~np.isin(k[bx < p["rhs_base"]], (RHS,)))
    else:
        assert not np.any(k == RHS) and not np.any(k == EXIT)


def finals(p, item):
    """the panels whose rows right-hand-side item (q, ct, g, final_only) makes final in its column tile (rhs_tile)"""
    q, ct, g, final_only = item
    last = p["np"] - 1
    if final_only:
        return [last]
    out = []
    if g == 0:
        out.append(p["rhs_p"])
        if p["rhs_last"]:
            out.append(last)
    return out


def walk_chain(Mp, ents, alone, seen):
    """every launch of the chain of a batch [(R, carries)]: coverage of each, then completeness of the right-hand sides over all of them"""
    batch = len(ents)
    rides = any(c for _, c in ents)
    max_R = max([R for R, c in ents if c], default=0)
    R_of = [R for R, _ in ents]
    np_ = (Mp + 31) // 32
    ns = np_ * (np_ + 1) // 2
    g_final = [np.zeros((R, ns), int) for R, _ in ents]       # writers of (q, slot p (p + 1) / 2 + ct): the final block and its sums slot
    a_final = [np.zeros(np_, int) for _ in ents]
    for jp in range(np_):
        p, wgs = cc.plan(Mp, batch, jp, 1, int(rides), max_R, int(alone), 0, R_of if rides else None, want_wgs=True)
        assert p["np"] == np_ and p["j"] == 32 * jp
        check_coverage(p, wgs, batch)
        assert p["iso"] == int(alone and np_ > 1)
        assert (p["la_idx"] >= 0) == (np_ > 1 and jp + 1 < np_)
        seen["tpw"].add(p["rhs_tpw"] if p["has_rhs"] else 0)
        if not rides:
            assert not p["has_rhs"]
            continue
        assert p["has_rhs"] == int(jp > 0 or jp == np_ - 1) and p["has_xself"] == int(jp == 0 and np_ > 1)
        if not p["has_rhs"]:
            continue
        assert p["rhs_p"] == jp - 1 and p["rhs_last"] == int(jp == np_ - 1) and p["rhs_ng"] == max(1, -(-p["rhs_nt"] // p["rhs_tpw"]))
        if p["rhs_tpw"] == 2:
            seen["tpw2_groups"].add((p["rhs_nt"], p["rhs_ng"]))
        items = wgs[wgs[:, 2] == RHS]
        tiles = {}                                                   # (b, q, ct) -> row tiles below the lagged panel that get updated
        for b, _, _, q, ct, g, fo, t0 in items.tolist():
            R, c = ents[b]
            assert q <= R
            if fo and p["rhs_p"] < 0:
                seen["one_panel_final_only"] = True
                assert not p["has_xin"]
            for pan in finals(p, (q, ct, g, fo)):
                if q < R:
                    assert ct <= pan
                    g_final[b][q, pan * (pan + 1) // 2 + ct] += 1
                else:
                    assert ct == 0
                    a_final[b][pan] += 1
            if not fo:
                t = tiles.setdefault((b, q, ct), [])
                t += [x for x in range(t0, t0 + p["rhs_tpw"]) if x < p["rhs_nt"]]      # (rhs_tile: rhs_tpw consecutive tiles from the group's first)
        for (b, q, ct), t in tiles.items():                         # every 64-row tile below the lagged panel exactly once
            assert sorted(t) == list(range(p["rhs_nt"])), (Mp, jp, b, q, ct, t)
        # the lagged items of a launch: every (q < R, ct <= p) and alpha
        for b, (R, c) in enumerate(ents):
            want = {(q, ct) for q in range(R) for ct in range(jp)} | ({(R, 0)} if jp > 0 else set())
            assert {k[1:] for k in tiles if k[0] == b} == want
    for b, (R, c) in enumerate(ents):
        if c:
            assert np.all(g_final[b] == 1), (Mp, batch, b, g_final[b])
            assert np.all(a_final[b] == 1), (Mp, batch, b, a_final[b])


@pytest.mark.parametrize("Mp", RIDE_MPS)
def test_every_launch_of_the_riding_chain_is_covered_and_complete(Mp):
    seen = {"tpw": set(), "tpw2_groups": set(), "one_panel_final_only": False}
    for batch in range(1, 9):
        for max_R in MAX_RS:
            for alone in (True, False):
                walk_chain(Mp, table_batch(batch, max_R), alone, seen)
    # reach: one and two row tiles per workgroup (two from three panels on: batch 8, R = 32 at jp = 2 is 8 x 65 = 520 workgroups; two panels stay at
    # 8 x 33 = 264), a one-panel matrix's final_only item without Xin
    assert 1 in seen["tpw"]
    assert (2 in seen["tpw"]) == (Mp > 64), (Mp, seen)
    assert seen["one_panel_final_only"] == (Mp <= 32)
    if Mp == 256:      # two tiles per workgroup with an odd and an even count of row tiles, and with a single one (the second tile of the workgroup idle)
        assert {(3, 2), (2, 1), (1, 1), (4, 2)} <= seen["tpw2_groups"], seen["tpw2_groups"]


@pytest.mark.parametrize("Mp", PLAIN_MPS)
def test_every_launch_without_right_hand_sides_is_covered(Mp):
    np_ = (Mp + 31) // 32
    for batch in range(1, 9):
        for alone in (True, False):
            seen = {"tpw": set(), "tpw2_groups": set(), "one_panel_final_only": False}
            walk_chain(Mp, [(0, False)] * batch, alone, seen)
            assert seen["tpw"] == {0}
        for jp in range(np_):      # a plain factor: no inverse, no look-ahead, never the isolated grid; the last launch has nothing but the diagonal block
            p, wgs = cc.plan(Mp, batch, jp, 0, 0, 0, 1, 0, None, want_wgs=True)
            check_coverage(p, wgs, batch)
            assert not p["iso"] and p["la_idx"] < 0 and p["nct"] == 0 and not p["has_xla"]
            assert (p["gx"] == 0) == (jp == np_ - 1)


def test_plan_arguments_are_checked():
    from deepcgp_amd import device as dev
    L = dev.lib()
    q = (C.c_longlong * 8)(64, 2, 0, 1, 1, 3, 1, 0)
    out = (C.c_longlong * 24)()
    assert L.dcgp_debug_plan_chain(q, 7, None, 0, out, 24, None, 0) != 0 and L.dcgp_debug_plan_chain(q, 8, None, 0, out, 23, None, 0) != 0
    assert L.dcgp_debug_plan_chain(q, 8, None, 0, out, 24, None, 0) == 0
    for bad in ((64, 2, 2, 1, 1, 3, 1, 0), (64, 2, 0, 0, 1, 3, 1, 0), (272, 2, 0, 1, 1, 3, 1, 0), (64, 0, 0, 1, 0, 0, 1, 0)):      # jp beyond; rides without inverse; rides beyond 256
        assert L.dcgp_debug_plan_chain((C.c_longlong * 8)(*bad), 8, None, 0, out, 24, None, 0) != 0, bad
    # the workgroup table needs its exact size and, with right-hand-side items, every matrix's R
    q = (C.c_longlong * 8)(64, 2, 1, 1, 1, 3, 1, 0)
    assert L.dcgp_debug_plan_chain(q, 8, None, 0, out, 24, None, 0) == 0
    wgs = np.zeros((out[23], 8), np.int64)
    assert L.dcgp_debug_plan_chain(q, 8, None, 0, out, 24, wgs.ctypes.data, out[23]) != 0
    R_of = (C.c_longlong * 2)(3, 1)
    assert L.dcgp_debug_plan_chain(q, 8, R_of, 2, out, 24, wgs.ctypes.data, out[23] - 1) != 0
    assert L.dcgp_debug_plan_chain(q, 8, R_of, 2, out, 24, wgs.ctypes.data, out[23]) == 0


def test_chain_no_iso_takes_the_two_dimensional_grid():
    for alone in (0, 1):
        p = cc.plan(256, 3, 2, 1, 1, 10, alone, no_iso=1, R_of=[10, 10, 10])
        assert not p["iso"] and (p["grid_x"], p["grid_y"]) == (p["gx"], 3)
    assert cc.plan(256, 3, 2, 1, 1, 10, 1, no_iso=0, R_of=[10, 10, 10])["iso"]


# ---- the GPU cases (tests/test_gpu_chain.py) are on the configurations they declare -------------------------------------------------------------------
GPU_CASES = ([(b, M, True) for b, M in cc.RIDE_CASES + cc.LARGE_CASES] + [cc.PLAIN_FACTOR_CASE + (False,), ("b", cc.STATUS_MP, True)])


@pytest.mark.parametrize("batch,M,has_inv", GPU_CASES, ids=[cc.case_id(b, M) + ("" if inv else " no inverse") for b, M, inv in GPU_CASES])
def test_gpu_case_lands_on_its_declared_configuration(batch, M, has_inv):
    d = cc.declared(batch, M, has_inv)
    ents = cc.BATCHES[batch]
    assert d["Mp"] % 16 == 0 and d["Mp"] - M < 16
    assert not d["rides"] or d["Mp"] <= cc.MAX_RIDE_MP
    R_of = [e["R"] for e in ents]
    tpw2 = set()
    for alone in (1, 0):
        for jp in range(d["np"]):
            p = cc.plan(d["Mp"], len(ents), jp, int(has_inv), int(d["rides"]), d["max_R"], alone, 0, R_of if d["rides"] else None)
            assert p["np"] == d["np"]
            assert (p["la_idx"] >= 0) == (d["lookahead"] and jp + 1 < d["np"])
            assert p["iso"] == int(bool(alone and d["lookahead"]))
            assert p["has_rhs"] == int(d["rides"] and (jp > 0 or d["one_panel"]))
            if p["has_rhs"] and p["rhs_tpw"] == 2:
                tpw2.add(jp)
            if jp == d["np"] - 1:
                assert (p["gx"] == 0) == (not has_inv)
                if d["ragged"]:
                    assert d["Mp"] - p["j"] == 16
    assert tpw2 == d["tpw2"], (tpw2, d["tpw2"])


def test_gpu_cases_as_a_whole_reach_what_the_issue_lists():
    decl = [cc.declared(b, M, inv) for b, M, inv in GPU_CASES]
    assert {d["np"] for d in decl if d["rides"]} == set(range(1, 9))                         # 1 .. 8 panels under right-hand sides
    assert any(d["ragged"] and d["rides"] for d in decl) and any(d["one_panel"] and d["rides"] for d in decl)
    assert any(d["tpw2"] for d in decl) and any(d["rides"] and not d["tpw2"] for d in decl)
    # two tiles per workgroup over 1, 2, 3 and 4 row tiles: a lone tile, one full group, a full group and a half, two full groups
    tiles = set()
    for (b, M, inv), d in zip(GPU_CASES, decl):
        for jp in d["tpw2"]:
            p = cc.plan(d["Mp"], len(cc.BATCHES[b]), jp, 1, 1, d["max_R"], 1, 0, [e["R"] for e in cc.BATCHES[b]])
            assert p["rhs_tpw"] == 2 and p["rhs_nt"] == -(-(d["Mp"] - 32 * jp) // 64)
            tiles.add(p["rhs_nt"])
    assert tiles == cc.TPW2_ROW_TILES
    assert {d["Mp"] for d in decl if not d["rides"] and d["lookahead"]} >= {384, 1008}
    assert any(not inv for _, _, inv in GPU_CASES)
    # odd and even counts of 64-row tiles below the first panel, 1 .. 4 inverse column tiles
    assert {((d["Mp"] - 32 + 63) // 64) % 2 for d in decl if d["rides"] and d["np"] > 1} == {0, 1}
    assert {(d["Mp"] + 63) // 64 for d in decl if d["rides"]} == {1, 2, 3, 4}
    # the status-word columns: panel 0, a middle panel, the ragged last one, the first column of a panel
    cols = cc.STATUS_COLUMNS
    assert cols["panel 0"] // 32 == 0 and cols["panel 0"] % 32 and 0 < cols["middle panel"] // 32 < (cc.STATUS_MP - 1) // 32 and cols["middle panel"] % 32
    assert cols["ragged last panel"] // 32 == (cc.STATUS_MP - 1) // 32 and cc.STATUS_MP % 32 == 16
    assert cols["first column of a panel"] % 32 == 0 and cols["first column of a panel"] > 0

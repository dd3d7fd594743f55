"""The launch plan of the strided GEMM (csrc/gemm_plan.h: plan_gemm, the function gemm_gen() launches from), pinned down without a GPU through
dcgp_debug_plan_gemm: every case of tests/gemm_cases.py is on the configuration it declares, the table as a whole reaches every instantiation, epilogue,
grid, route and split count that tests/test_gpu_gemm.py is meant to run, and the reference of the exact cases is exact."""
import itertools

import numpy as np
import pytest

import gemm_cases as gc
import gemm_ref

GENERAL = [c for c in gc.CASES if c["expect"]["route"] == gc.GENERAL]


def _plans(cases):
    return [(c, gc.plan(gc.query(c))) for c in cases]


def test_every_case_is_on_the_configuration_it_declares():
    assert len(gc.CASES) > 200
    for c, p in _plans(gc.CASES):
        assert (c["a_cs"] == 1) == (c["layout"][0] == "n") and (c["b_rs"] == 1) == (c["layout"][1] == "t"), c["name"]
        assert gc.check_plan(c, p) == {}, (c["name"], p)
        assert {"route"} <= set(c["expect"]) and (c["expect"]["route"] != gc.GENERAL or {"tile", "split", "compact"} <= set(c["expect"])), c["name"]
        if c["gemm_tile"]:
            assert c["expect"]["tile"] == c["gemm_tile"] and ("vec" in c["expect"] or c["sym"]), c["name"]


def test_the_older_kernel_tests_take_the_32_tile():
    """the run(...) calls of test_strided_gemm_layouts_edges_and_epilogues and test_strided_gemm_adjoint_epilogues (tests/test_gpu_ops.py): all on
    <32, 256, 16>, the long contractions split 35, 29, 63 and 21 ways"""
    cases = gc.legacy_cases()
    assert len(cases) == 4 * 9 + 6
    for c, p in _plans(cases):
        assert gc.check_plan(c, p) == {}, (c["name"], p)
        assert p["tile"] == 32 and p["threads"] == 256 and p["wave_tile"] == 16


def _reach(cases):
    """{(tile, AKF, BKF, VEC, split)} of the plans, from the planning function itself"""
    return {(p["tile"], p["akf"], p["bkf"], p["vec"], p["ksplit"] > 1) for c, p in _plans(cases) if p["route"] == gc.GENERAL}


def test_all_24_instantiations_direct_and_split():
    want = set(itertools.product(gc.TILES, (0, 1), (0, 1), (0, 1), (False, True)))
    forced = [c for c in GENERAL if c["gemm_tile"]]
    assert _reach(forced) == want
    # scalar loads through an odd stride and, with even strides, through a base 8 bytes off the 16-byte grid
    odd = [c for c in forced if c["a_off"] == 0 and (c["a_ld"] & 1) and (c["b_ld"] & 1)]
    off8 = [c for c in forced if c["a_off"] == 1 and not (c["a_ld"] & 1 or c["b_ld"] & 1 or c["a_bs"] & 1 or c["b_bs"] & 1)]
    scalar = set(itertools.product(gc.TILES, (0, 1), (0, 1), (0,), (False, True)))
    assert _reach(odd) == scalar and _reach(off8) == scalar
    # the block of the table that is there for this: one case per tile x layout x way to the load width x {direct, split}, none of them missing
    inst = {(p["tile"], p["akf"], p["bkf"], "odd" if c["a_ld"] & 1 else ("off8" if c["a_off"] else "vec"), p["vec"], p["ksplit"] > 1)
            for c, p in _plans(c for c in forced if c["name"].startswith("inst"))}
    assert inst == {(t, a, b, how, int(how == "vec"), s) for t, a, b, how, s in itertools.product(gc.TILES, (0, 1), (0, 1), ("vec", "odd", "off8"), (False, True))}


def test_ragged_extents_on_every_tile():
    for gt in gc.TILES:
        mine = [c for c in GENERAL if c["gemm_tile"] == gt and c["name"].startswith("ragged")]
        ext = {1, gt - 1, gt, gt + 1, 2 * gt + 3}
        assert {c["M"] for c in mine} == ext and {c["N"] for c in mine} == ext
        assert {c["K"] for c in mine} == {0, 1, 15, 16, 17, 33}
        # K = 0 writes alpha 0 (+ C0): with and without the previous content on more than one row and output, and behind each triangular store
        empty = {(c["accumulate"], c["colscale"] and c["kscale"], c["lower"], c["mirror"], bool(c["expect"]["compact"]))
                 for c in GENERAL if c["gemm_tile"] == gt and c["K"] == 0 and c["M"] > 1 and c["batch"] > 1}
        assert empty == {(True, False, False, False, False), (True, True, False, False, False), (False, False, False, False, False),
                         (False, False, True, False, False), (True, False, True, False, True), (False, False, True, True, False),
                         (True, False, True, True, True)}
    # a four-element fetch group that is half valid, under 16-byte loads: rows of a transposed A, columns of a row-major B
    half = [c for c in GENERAL if c["gemm_tile"] == 64 and c["expect"].get("vec")]
    assert any(c["layout"][0] == "t" and c["M"] % 4 == 2 for c in half) and any(c["layout"][1] == "n" and c["N"] % 4 == 2 for c in half)


def test_every_epilogue_on_every_tile_direct_and_split():
    got, alone = set(), set()
    for c, p in _plans(c for c in GENERAL if c["gemm_tile"] and c["batch"] > 1 and c["kind"] == "exact"):
        got |= {(e, p["tile"], p["ksplit"] > 1) for e in gc.epilogues(c)}
        if len(gc.epilogues(c)) == 1:
            alone |= {(e, p["tile"], p["ksplit"] > 1) for e in gc.epilogues(c)}
    # the simple ones also on their own, so that a failure names its epilogue
    assert alone >= set(itertools.product(("alpha", "accumulate", "colscale", "kscale", "phi"), gc.TILES, (False, True)))
    want = set(itertools.product(gc.EPILOGUES, gc.TILES, (False, True))) - {("lower_rect", gt, True) for gt in gc.TILES}   # (a split launch is always compact)
    assert got == want
    # both lower_only grids on every tile, as the planning function reports them; more than one tile row, so that tiles above the diagonal exist
    grids = {(p["tile"], p["lower_compact"]) for c, p in _plans(c for c in GENERAL if c["gemm_tile"] and c["lower"]) if c["M"] > p["tile"]}
    assert grids == set(itertools.product(gc.TILES, (0, 1)))
    assert any(c["mirror"] and c["accumulate"] for c in GENERAL)


def test_split_counts_cover_the_reduction():
    """splitk_reduce_kernel adds batches of 8 partials, then a tail: below 8, a multiple of 8, above 8 with a remainder -- on each tile; and every split
    of the 'just past the threshold' cases ends inside a k tile"""
    for gt in gc.TILES:
        ks = {p["ksplit"] for c, p in _plans(c for c in GENERAL if c["gemm_tile"] == gt) if p["ksplit"] > 1}
        assert any(k < 8 for k in ks) and any(k % 8 == 0 for k in ks) and any(k > 8 and k % 8 for k in ks), (gt, ks)
        short = [(c, p) for c, p in _plans(c for c in GENERAL if c["gemm_tile"] == gt and c["name"].startswith("inst") and c["expect"]["split"])]
        assert len(short) == 12
        for c, p in short:
            last = c["K"] - (p["ksplit"] - 1) * p["kchunk"]
            assert gc.SPLIT_MIN_K[gt] < c["K"] < gc.SPLIT_MIN_K[gt] + 16 and 0 < last < p["kchunk"] and last % 16, (c["name"], p)


def test_natural_dispatch_and_its_thresholds():
    nat = {c["name"]: p for c, p in _plans(gc.natural())}
    assert {(p["tile"], p["ksplit"] > 1) for p in nat.values()} >= {(64, False), (64, True), (128, False), (128, True), (32, False), (32, True)}
    assert any(p["tile"] == 128 and p["lower_compact"] for p in nat.values())
    # one pair on either side of each threshold of the tile choice and of the split
    for a, b, ta, tb in (("fill 128: batch 16", "fill 128: batch 15", 128, 64), ("fill 128: K 4096", "fill 128: K 4095", 128, 64),
                         ("fill 128: M 128", "fill 128: M 127", 128, 64), ("small 32: 4 x 64", "small 64: 4 x 65", 32, 64),
                         ("small 32: 64 x 4 ranges", "small 64: 65 x 4 ranges", 32, 64)):
        assert (nat[a]["tile"], nat[b]["tile"]) == (ta, tb), (a, b)
    for a, b, t in (("split 32: K 1024", "split 32: K 1023", 32), ("split 64: K 2048", "split 64: K 2047", 64), ("split 128: 256 tiles", "split 128: 260 tiles", 128)):
        assert nat[a]["tile"] == nat[b]["tile"] == t and nat[a]["ksplit"] > 1 and nat[b]["ksplit"] == 1, (a, b)


def test_syrk_route_and_its_neighbours():
    sy = [c for c in gc.syrk() if c["expect"]["route"] == gc.SYRK]
    assert {c["M"] for c in sy} == {129, 130, 200, 255, 256} and {c["K"] for c in sy} == {8192, 8193, 8222, 11520} and {c["batch"] for c in sy} == {1, 3}
    assert {c["a_ld"] - c["K"] for c in sy if c["K"] % 2 == 0} == {0, 2, 6} and all(c["a_ld"] > c["K"] for c in sy if c["K"] % 2)
    for K in (8192, 8193, 8222, 11520):
        assert any(c["a_ld"] > K for c in sy if c["K"] == K)
    for c, p in _plans(sy):
        assert p["route"] == gc.SYRK and p["threads"] == 768 and p["grid_x"] == p["ksplit"] and p["grid_y"] == c["batch"] and p["kchunk"] % 32 == 0
        assert p["lds"] == (2 * 256 * 33 + 2 * 32) * 8 and p["part_doubles"] == p["ksplit"] * c["batch"] * c["M"] ** 2
        # the same call with no_syrk = 1, and with 104 compute units
        assert gc.plan(gc.query(dict(c, no_syrk=1)))["route"] == gc.GENERAL
        assert gc.plan(gc.query(c, n_cus=104))["ksplit"] <= 104 // c["batch"]
    out = {c["name"]: c for c in gc.syrk() if c["expect"]["route"] == gc.GENERAL}
    assert set(out) == {"not syrk: M 128", "not syrk: K 8191", "not syrk: odd row stride", "not syrk: batch 65", "not syrk: no_syrk"}
    assert (out["not syrk: M 128"]["M"], out["not syrk: K 8191"]["K"], out["not syrk: odd row stride"]["a_ld"] & 1, out["not syrk: batch 65"]["batch"],
            out["not syrk: no_syrk"]["no_syrk"]) == (128, 8191, 1, 65, 1)
    for c in out.values():      # each is one step outside: the same call moved back inside takes the kernel
        inside = dict(c, M=max(c["M"], 129), N=max(c["N"], 129), K=max(c["K"], 8192), batch=min(c["batch"], 64), no_syrk=0)
        if c["a_ld"] & 1:
            inside.update(a_rs=c["a_ld"] + 1, b_cs=c["a_ld"] + 1)
        assert gc.plan(gc.query(inside))["route"] == gc.SYRK, c["name"]


def test_argument_errors_and_empty_results():
    base = gc.make("x", 40, 40, 1500, batch=2, gemm_tile=32, tile=32)
    assert gc.plan(gc.query(dict(base, M=0)))["route"] == gc.NOTHING and gc.plan(gc.query(dict(base, N=0)))["route"] == gc.NOTHING
    p = gc.plan(gc.query(dict(base, batch=0)))
    assert (p["route"], p["error"], p["grid_x"]) == (gc.NOTHING, 0, 0)
    assert gc.plan(gc.query(dict(base, K=-1)))["error"] == 1
    q = gc.query(base)
    q[gc.QUERY_FIELDS.index("null_ptr")] = 1
    assert gc.plan(q)["error"] == 1
    # batch x split is the grid's z extent.  A split keeps the launch within one round of 1024 workgroups, so only a batch on its own can be too large
    assert gc.plan(gc.query(dict(base, batch=65535)))["error"] == 0
    p = gc.plan(gc.query(dict(base, batch=65536)))
    assert (p["error"], p["ksplit"]) == (2, 1)
    # lower_only on the compact grid needs a square result; on the rectangular grid (direct store, no accumulation) it never did
    assert gc.plan(gc.query(dict(base, N=41, lower=True)))["error"] == 3
    assert gc.plan(gc.query(dict(base, N=41, K=20, lower=True, accumulate=True)))["error"] == 3
    assert gc.plan(gc.query(dict(base, N=41, K=20, lower=True)))["error"] == 0
    from deepcgp_amd import device as dev
    import ctypes as C
    qa, pa = (C.c_longlong * 24)(*q), (C.c_longlong * 17)()
    assert dev.lib().dcgp_debug_plan_gemm(qa, 23, pa, 17) != 0 and dev.lib().dcgp_debug_plan_gemm(qa, 24, pa, 16) != 0
    assert dev.lib().dcgp_debug_plan_gemm(qa, 24, pa, 17) == 0


def test_grid_and_partial_buffer_of_a_plan():
    for c, p in _plans(GENERAL):
        gt = p["tile"]
        nt_m, nt_n = -(-c["M"] // gt), -(-c["N"] // gt)
        assert (p["threads"], p["wave_tile"]) == {32: (256, 16), 64: (256, 32), 128: (1024, 32)}[gt]
        assert p["grid_z"] == c["batch"] * p["ksplit"] <= 65535
        if p["lower_compact"]:
            assert (p["grid_x"], p["grid_y"]) == (nt_m * (nt_m + 1) // 2, 1) and c["M"] == c["N"]
        else:
            assert (p["grid_x"], p["grid_y"]) == (nt_n, nt_m)
        if p["ksplit"] > 1:
            assert p["kchunk"] % 16 == 0 and (p["ksplit"] - 1) * p["kchunk"] < c["K"] <= p["ksplit"] * p["kchunk"] and p["kchunk"] >= gc.SPLIT_CHUNK[gt]
            assert p["part_doubles"] == p["ksplit"] * c["batch"] * c["M"] * c["N"] and p["reduce_blocks"] == -(-c["batch"] * c["M"] * c["N"] // 256)
        else:
            assert p["kchunk"] == c["K"] and p["part_doubles"] == 0 and p["reduce_blocks"] == 0


@pytest.mark.parametrize("part", range(8))
def test_reference_of_the_exact_cases_is_exact(part):
    """For every integer case the float64 reference equals the same contraction in int64, and the sum of the terms' magnitudes -- a bound on every partial
    sum in any order, epilogue included -- stays far below 2^53: the device result cannot depend on tile, split or order of summation."""
    rng = np.random.default_rng(11)
    exact = [c for c in gc.CASES if c["kind"] == "exact"]
    assert len(exact) == len(gc.CASES) - 6
    worst = 0.0
    for c in exact[part::8]:
        d = gc.build(c, rng)
        ops, ep = gc.ref_args(c, d)
        for x in (d["A"], d["B"], d["C0"], d["ks"], d["cs"], d["sv"], d["sx"]):
            assert x is None or (np.array_equal(x, np.rint(x)) and (np.abs(x).max(initial=0) <= 3)), c["name"]
        f = gemm_ref.contraction(d["A"], d["B"], ep["kscale"], np.float64)      # (scales shared by the batch: one contraction)
        i = gemm_ref.contraction(d["A"], d["B"], ep["kscale"], np.int64)
        assert f.dtype == np.float64 and i.dtype == np.int64 and np.array_equal(f, i), c["name"]
        assert np.log2(abs(c["alpha"])) % 1 == 0
        worst = max(worst, gemm_ref.magnitude(*ops, **ep).max(initial=0))
        if c["alpha"] % 1 == 0 and not c["phi"]:        # the whole operator in integers (phi halves the diagonal)
            assert np.array_equal(gemm_ref.epilogue(f, d["C0"], **{k: v for k, v in ep.items() if k != "kscale"}),
                                  gemm_ref.epilogue(i, d["C0"].astype(np.int64), **{k: v for k, v in ep.items() if k != "kscale"})), c["name"]
    assert worst < 2.0 ** 53 / 1e6, worst

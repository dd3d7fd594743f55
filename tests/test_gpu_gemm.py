"""The strided fp64 GEMM of the reverse pass (csrc/gemm_gen.hip) on every tile, layout, load width, split and epilogue, and syrk_kscale_kernel through the
operator entry -- the cases of tests/gemm_cases.py against the plain NumPy statement of the operator (tests/gemm_ref.py).

Exact cases: operands, scales, corrections and previous content are small integers and alpha a power of two, so every product and partial sum is an
integer far below 2^53 (tests/test_host_gemm_plan.py checks that) and the double result does not depend on tile, split or order of summation: the device
result must EQUAL the reference; a dropped, duplicated or misplaced term fails.  Rounding cases: standard normals against a long-double reference within
the textbook dot-product bound, which holds for any order of fused multiply-adds:
    |got - want|_ij <= (K + ksplit + 8) 2^-53 (|alpha| |A| diag|ks| |B| |cs| + |alpha| |sub_v| |sub_x| + |C0|)_ij.
Every case: C is a view into a wider buffer and everything outside the result must be bit-identical afterwards; every gap of A and B (row stride beyond
the extent, batch stride beyond the matrix, the tail behind the last batch), kscale past K and colscale past N hold NaN, so a read past an extent shows.
Each case first asserts, through the launch plan (dcgp_debug_plan_gemm under the ctx's options), that it runs on the configuration it declares."""
import numpy as np
import pytest

import gemm_cases as gc
import gemm_ref

pytestmark = pytest.mark.gpu


def _call(ctx, c, d):
    """the case on the device: (C buffer afterwards, the plan it ran on)"""
    from deepcgp_amd import device as dev
    L = dev.lib()
    dA = ctx.to_device(d["A_buf"])
    dB = dA if c["sym"] else ctx.to_device(d["B_buf"])
    dC = ctx.to_device(d["C_buf"])
    assert dA.ptr % 16 == 0 and dB.ptr % 16 == 0
    vec = {k: ctx.to_device(d[k + "_buf"]) if d[k + "_buf"] is not None else None for k in ("ks", "cs", "sv", "sx")}

    def ptr(k):
        return vec[k].ptr if vec[k] is not None else None
    pa, pb = dA.ptr + 8 * c["a_off"], dB.ptr + 8 * c["b_off"]
    with ctx.options(gemm_tile=c["gemm_tile"], no_syrk=c["no_syrk"]):
        p = gc.plan(gc.query(c, n_cus=ctx.get_option("n_cus")))
        assert gc.check_plan(c, p) == {}, (c["name"], p)
        head = (ctx.handle, pa, c["a_rs"], c["a_cs"], c["a_bs"], pb, c["b_rs"], c["b_cs"], c["b_bs"], dC.ptr, c["c_rs"], c["c_bs"], c["M"], c["N"], c["K"],
                c["batch"], c["alpha"], int(c["accumulate"]))
        if c["entry"] == "strided":
            ctx._check(L.dcgp_gemm_strided(*head, ptr("cs"), c["cs_s"], c["cs_bs"], ptr("ks"), c["ks_s"], c["ks_bs"], c["flags"]))
        else:
            ctx._check(L.dcgp_gemm_strided_ex(*head, ptr("sv"), c["sv_bs"], ptr("sx"), c["sx_rs"], c["sx_bs"], c["flags"]))
    return dC.numpy(), p


def _result(c, d, out):
    """the result cut out of the buffer, after checking that nothing beside it changed"""
    same = out.view(np.uint64) == d["C_buf"].view(np.uint64)
    assert same[~d["inside"]].all(), (c["name"], "written outside the result", np.flatnonzero(~same & ~d["inside"])[:8])
    return gc._view(out, 0, c["c_bs"], c["c_rs"], 1, c["batch"], c["M"], c["N"])


def _run(ctx, c, rng):
    d = gc.build(c, rng)
    out, p = _call(ctx, c, d)
    got = _result(c, d, out)
    ops, ep = gc.ref_args(c, d)
    if c["kind"] == "exact":
        want = gemm_ref.gemm(*ops, **ep)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError("%s: %d of %d entries differ, first (b, i, j) = %s: got %r, want %r; plan %r"
                                 % (c["name"], len(bad), want.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])], p))
    else:
        want = gemm_ref.gemm(*ops, dtype=np.longdouble, **ep)
        bound = (c["K"] + p["ksplit"] + 8) * 2.0 ** -53 * gemm_ref.magnitude(*ops, **ep)
        err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        print("%s: max error / bound = %.3f" % (c["name"], (err / np.maximum(bound, 1e-300)).max()))
        assert np.isfinite(got).all() and (err <= bound).all(), (c["name"], float((err / np.maximum(bound, 1e-300)).max()), p)
    return d, got, p


@pytest.mark.parametrize("layout", gc.LAYOUTS)
@pytest.mark.parametrize("tile", gc.TILES)
def test_forced_tile(ctx, tile, layout):
    """gemm_gen_kernel<tile, ...> under ctx option gemm_tile: 16-byte and scalar loads, ragged extents, split counts, every epilogue direct and split"""
    cases = gc.forced(tile, layout)
    assert len(cases) >= 8
    rng = np.random.default_rng(100 * tile + gc.LAYOUTS.index(layout))
    for c in cases:
        _run(ctx, c, rng)


def test_natural_dispatch(ctx):
    """gemm_tile = 0: the shapes that reach the 64 and 128 tiles on their own, and both sides of each threshold of the dispatch"""
    assert ctx.get_option("gemm_tile") == 0
    rng = np.random.default_rng(7)
    tiles = set()
    for c in gc.natural():
        tiles.add(_run(ctx, c, rng)[2]["tile"])
    assert tiles == {32, 64, 128}


def test_syrk_route(ctx):
    """syrk_kscale_kernel through dcgp_gemm_strided (kscale, lower_only + mirror, A == B): ragged K, padded rows with NaN in the gap, 129 .. 256 rows, one
    and three outputs -- equal to the reference, equal to the general kernel (no_syrk = 1), both triangles stored; and the neighbours just outside it"""
    rng = np.random.default_rng(8)
    for c in gc.syrk():
        d, got, p = _run(ctx, c, rng)
        assert np.array_equal(got, np.transpose(got, (0, 2, 1))), c["name"]
        if c["expect"]["route"] != gc.SYRK:
            continue
        assert p["route"] == gc.SYRK
        other = dict(c, no_syrk=1, expect=dict(route=gc.GENERAL, tile=gc.plan(gc.query(dict(c, no_syrk=1)))["tile"], compact=True, split=True))
        out, p2 = _call(ctx, other, d)
        assert p2["route"] == gc.GENERAL and np.array_equal(_result(other, d, out), got), c["name"]


def test_degenerate_extents_and_refused_flags(ctx):
    """M = 0, N = 0 or batch = 0: OK and nothing written (K = 0, which writes alpha 0 (+ C0), is in the table); mirror without lower_only or on a
    non-square result, and bits beyond the two, are refused by dcgp_gemm_strided as by dcgp_gemm_strided_ex"""
    from deepcgp_amd import device as dev
    L = dev.lib()
    rng = np.random.default_rng(9)
    C0 = rng.standard_normal(64)
    dA, dB, dC = ctx.to_device(np.full(64, np.nan)), ctx.to_device(np.full(64, np.nan)), ctx.to_device(C0)

    def call(M, N, K, batch, flags=0, accumulate=0):
        return L.dcgp_gemm_strided(ctx.handle, dA.ptr, K, 1, M * K, dB.ptr, N, 1, K * N, dC.ptr, N, M * N, M, N, K, batch, 1.0, accumulate, None, 0, 0, None, 0, 0,
                                   flags)
    for tile in (0,) + gc.TILES:
        with ctx.options(gemm_tile=tile):
            for M, N, K, batch in ((0, 4, 3, 2), (4, 0, 3, 2), (4, 4, 3, 0), (0, 0, 0, 0)):
                assert call(M, N, K, batch) == 0 and call(M, N, K, batch, flags=1, accumulate=1) == 0
    assert np.array_equal(dC.numpy().view(np.uint64), C0.view(np.uint64))
    for M, N, flags in ((4, 4, 2), (4, 5, 3), (4, 4, 4), (4, 4, 7)):
        assert call(M, N, 3, 1, flags=flags) == dev.ERR_ARG
    assert np.array_equal(dC.numpy().view(np.uint64), C0.view(np.uint64))

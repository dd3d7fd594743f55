"""The factorisation chain as an operator (csrc/chol_fused.hip: factor_inverse_batched, chol_rl_kernel, rhs_tile) through dcgp_debug_factor_chain, which
fills a factor group as a model does and calls its run() and finish(): L, inv(L) and its transpose, the right-hand sides G_r = inv(L) Lq_r and
alpha = inv(L) q_mu that ride the panel launches, their sums of squares and the status word, element by element against tests/chain_ref.py (NumPy / SciPy
float64).  The cases are tests/chain_cases.py's; tests/test_host_chain_plan.py holds each to the launch configuration it declares.

Every output buffer and the sums are NaN before the call, so an element nobody writes shows.  Bounds: 1e-9 relative to the tensor's maximum for L, inv(L),
G, alpha and the sums against the reference (the bound tests/test_gpu_ops.py holds these quantities to), 1e-13 for L L^T against A and 1e-9 for
inv(L) L against I (test_kuu_potrf_trtri_realistic_large_M's); a sums slot against the extended-precision sum of squares of the device's own block:
2 * 1024 * 2^-53 relative (two sums of at most 1024 non-negative terms each err by at most n u).  Everything else is bit for bit: inv(L)^T against
inv(L), the structural zeros, and the outputs of a matrix under every route (alone or not, finish deferred or not, in a batch or by itself -- the
arithmetic of a tile does not depend on rhs_tpw or on the grid decode).  The measured maxima are printed per case."""
import numpy as np
import pytest

import chain_cases as cc
import chain_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MODES = [(alone, defer) for alone in (True, False) for defer in (False, True)]
_CASES = {}


def case(batch, M):
    """inputs and reference of a case, computed once and left unchanged"""
    if (batch, M) not in _CASES:
        inp = cc.build(batch, M)
        _CASES[(batch, M)] = (inp, chain_ref.reference(inp))
    return _CASES[(batch, M)]


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def check_against_reference(out, inp, ref, worst, inverse=True):
    """values, bit-level structure and sums of one call's outputs"""
    Mp, eye = inp["Mp"], np.eye(inp["Mp"])

    def note(key, err, bound):
        worst[key] = max(worst.get(key, 0.0), err)
        assert err <= bound, "%s: %.3e > %.1e" % (key, err, bound)
    assert np.all(out["info"] == 0), out["info"]
    for b, e in enumerate(inp["ents"]):
        L = out["L"][b]
        assert np.all(np.isfinite(L)) and np.all(np.triu(L, 1) == 0.0)
        note("L", rel(L, ref["L"][b]), 1e-9)
        note("L L^T - A", rel(L @ L.T, inp["A"][b]), 1e-13)
        if inverse:
            Li = out["Linv"][b]
            assert np.all(np.isfinite(Li)) and np.all(np.triu(Li, 1) == 0.0)
            if out["LinvT"] is not None:
                assert np.array_equal(out["LinvT"][b], Li.T), "inv(L)^T is not the transpose of inv(L), matrix %d" % b
            note("Linv", rel(Li, ref["Linv"][b]), 1e-9)
            note("Linv L - I", rel(Li @ L, eye), 1e-9)
        G, alpha, sums = out["G"][b], out["alpha"][b], out["sums"][b]
        assert (G is not None) == bool(e["G"]) and (alpha is not None) == bool(e["alpha"]) and (sums is not None) == cc.carries(e)
        if G is not None:
            assert np.all(np.isfinite(G)), "NaN left in G of matrix %d: %s" % (b, np.argwhere(~np.isfinite(G))[:4])
            assert np.all(np.triu(G, 1) == 0.0), "structural zeros of G, matrix %d" % b
            note("G", rel(G, ref["G"][b]), 1e-9)
        if alpha is not None:
            assert np.all(np.isfinite(alpha))
            assert np.all(alpha[:, e["R"]:] == 0.0) and np.all(alpha[inp["M"]:] == 0.0)      # padded columns and rows
            note("alpha", rel(alpha, ref["alpha"][b]), 1e-9)
        if sums is not None:
            mask = ref["mask"][b]
            assert np.array_equal(mask, cc.written_slots(e, Mp))
            assert np.all(np.isfinite(sums[mask])), "sums slots nobody wrote, matrix %d: %s" % (b, np.argwhere(mask & ~np.isfinite(sums))[:4])
            assert np.all(np.isnan(sums[~mask])), "sums slots that belong to nobody were written, matrix %d" % b
            note("sums", float(np.max(np.abs(sums[mask] - ref["sums"][b][mask])) / np.max(ref["sums"][b][mask])), 1e-9)
            own, own_mask = chain_ref.block_sums(G, alpha, e["R"], Mp, dtype=np.longdouble)
            if own_mask.any():
                err = np.abs(sums[own_mask] - own[own_mask]) / np.maximum(own[own_mask], 1e-300)
                err[(own[own_mask] == 0.0) & (sums[own_mask] == 0.0)] = 0.0
                note("sums vs own block / (2048 u)", float(err.max()) / (2 * 1024 * U), 1.0)


def parts(out, b):
    """every output of matrix b of a call"""
    p = {k: out[k][b] for k in ("L", "Linv", "LinvT") if out[k] is not None}
    p.update({k: out[k][b] for k in ("G", "alpha", "sums") if out[k][b] is not None})
    return p


def assert_same_bits(got, want, what, only=None):
    for k in want:
        if k in got and (only is None or k in only):
            assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), \
                "%s: %s differs at %s" % (what, k, np.argwhere(~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k]))))[:4])


def show(name, worst):
    print("chain %-12s " % name + "  ".join("%s %.2e" % kv for kv in sorted(worst.items())))


def run_modes(ctx, inp, ref, worst, **kw):
    """the case under alone x defer_finish: each against the reference, all bit-identical; with defer_finish everything but L is complete before finish()"""
    first = None
    for alone, defer in MODES:
        out = cc.run(ctx, inp, alone=alone, defer=defer, snapshot=defer, **kw)
        check_against_reference(out, inp, ref, worst, inverse=kw.get("inverse", True))
        if defer:
            for b in range(len(inp["ents"])):
                before = parts(out["before"], b)
                assert_same_bits(before, parts(out, b), "before finish(), matrix %d" % b, only=("Linv", "LinvT", "G", "alpha", "sums"))
        if first is None:
            first = out
        for b in range(len(inp["ents"])):
            assert_same_bits(parts(out, b), parts(first, b), "alone=%d defer=%d against alone=1 defer=0, matrix %d" % (alone, defer, b))
    return first


@pytest.mark.parametrize("batch,M", cc.RIDE_CASES, ids=[cc.case_id(b, M) for b, M in cc.RIDE_CASES])
def test_chain_with_riding_right_hand_sides(ctx, batch, M):
    inp, ref = case(batch, M)
    worst = {}
    out = run_modes(ctx, inp, ref, worst)
    if len(inp["ents"]) > 1:
        # every matrix by itself (a batch of one never takes two row tiles per workgroup), storing G / alpha even where the batch keeps the sums only
        for b, e in enumerate(inp["ents"]):
            solo_inp = cc.subset(inp, [b], full=True)
            solo = cc.run(ctx, solo_inp)
            assert np.all(solo["info"] == 0)
            assert_same_bits(parts(out, b), parts(solo, 0), "in batch %s against alone, matrix %d" % (batch, b))
            if cc.carries(e) and not e["G"]:
                assert out["sums"][b].tobytes() == solo["sums"][0].tobytes(), "sums-only entry against the same entry storing G"
                sub_ref = chain_ref.reference(solo_inp)
                check_against_reference(solo, solo_inp, sub_ref, worst)
    show(cc.case_id(batch, M), worst)


@pytest.mark.parametrize("batch,M", cc.LARGE_CASES, ids=[cc.case_id(b, M) for b, M in cc.LARGE_CASES])
def test_chain_beyond_the_riding_size(ctx, batch, M):
    inp, ref = case(batch, M)
    worst = {}
    run_modes(ctx, inp, ref, worst)
    show(cc.case_id(batch, M), worst)


def test_plain_factor_without_inverse(ctx):
    """Linv == NULL: no look-ahead, and the last launch has nothing left but the diagonal block (gx == 0)"""
    inp, ref = case(*cc.PLAIN_FACTOR_CASE)
    worst = {}
    run_modes(ctx, inp, ref, worst, inverse=False)
    no_t = cc.run(ctx, inp, transpose=False)          # and the inverse without its transpose
    check_against_reference(no_t, inp, ref, worst)
    show(cc.case_id(*cc.PLAIN_FACTOR_CASE) + " plain", worst)


def test_descriptors_that_cannot_ride_are_refused(ctx):
    from deepcgp_amd.device import ERR_ARG, DcgpError
    inp, ref = case("b", 48)
    with ctx.options(no_rhs_ride=1):
        with pytest.raises(DcgpError) as e:
            cc.run(ctx, inp)
        assert e.value.code == ERR_ARG
        worst = {}
        plain = cc.build("plain", 48)                 # nothing asks to ride: the option does not matter
        check_against_reference(cc.run(ctx, plain), plain, chain_ref.reference(plain), worst)
    with pytest.raises(DcgpError) as e:
        cc.run(ctx, inp, may_ride=False)
    assert e.value.code == ERR_ARG
    check_against_reference(cc.run(ctx, inp), inp, ref, {})      # and the ctx is as usable as before


def indefinite(inp, b, col):
    A = inp["A"].copy()
    A[b, col, col] = -1.0
    return dict(inp, A=A)


@pytest.mark.parametrize("where", list(cc.STATUS_COLUMNS))
def test_status_word_names_the_matrix_and_the_column(ctx, where):
    """one matrix of three indefinite: its info is the 1-based column, its neighbours' 0 and their outputs those of a clean run"""
    inp, ref = case("b", cc.STATUS_MP)
    col = cc.STATUS_COLUMNS[where]
    bad = list(cc.STATUS_COLUMNS).index(where) % 3
    clean = cc.run(ctx, inp)
    for alone in (True, False):
        out = cc.run(ctx, indefinite(inp, bad, col), alone=alone)
        want = [0, 0, 0]
        want[bad] = col + 1
        assert out["info"].tolist() == want, (where, alone, out["info"])
        for b in range(3):
            if b != bad:
                assert_same_bits(parts(out, b), parts(clean, b), "neighbour %d of the indefinite matrix %d" % (b, bad))


def test_a_stale_status_word_does_not_survive_the_next_call(ctx):
    inp, ref = case("b", cc.STATUS_MP)
    clean = cc.run(ctx, inp)
    for alone in (True, False):
        out = cc.run(ctx, indefinite(inp, 1, 70), alone=alone, A_again=inp["A"])
        assert out["info"].tolist() == [[0, 71, 0], [0, 0, 0]], out["info"]
        for b in range(3):
            assert_same_bits(parts(out, b), parts(clean, b), "second, clean call on the same group, matrix %d" % b)

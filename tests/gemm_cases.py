"""The case table of the strided GEMM (csrc/gemm_gen.hip) and what each case DECLARES it reaches.

A case is a plain dict: extents, batch, layout, strides with their gaps, base-pointer offsets, epilogue switches, the forced ctx option gemm_tile
(0: natural dispatch) and its declared expectation `expect` = {route, tile, vec, split, compact[, ksplit]}.  tests/test_host_gemm_plan.py holds every
declaration against csrc/gemm_plan.h (through dcgp_debug_plan_gemm) and asserts what the table as a whole covers; tests/test_gpu_gemm.py runs the cases.
The expectations are written down from the shapes by the loops below, never read back from the planning function.

Layouts: first letter A, second B; 'n' is the row-major operand of the product (A [M][K], B [K][N]), 't' the transposed store (A [K][M], B [N][K]).
The kernel's AKF / BKF (the contraction index is the contiguous one) are therefore A 'n' and B 't'."""
import ctypes as C

import numpy as np

QUERY_FIELDS = ("M", "N", "K", "batch", "a_rs", "a_cs", "a_bs", "b_rs", "b_cs", "b_bs", "accumulate", "colscale", "kscale", "sub", "lower_only", "mirror", "phi",
                "a_aligned", "b_aligned", "same_ab", "null_ptr", "gemm_tile", "no_syrk", "n_cus")
PLAN_FIELDS = ("route", "error", "tile", "threads", "wave_tile", "ksplit", "kchunk", "lower_compact", "akf", "bkf", "vec", "grid_x", "grid_y", "grid_z",
               "part_doubles", "reduce_blocks", "lds")
NOTHING, GENERAL, SYRK = 0, 1, 2
TILES = (32, 64, 128)
LAYOUTS = ("nn", "tn", "nt", "tt")
SPLIT_MIN_K = {32: 1024, 64: 2048, 128: 2048}     # the contraction length from which a tile splits
SPLIT_CHUNK = {32: 128, 64: 512, 128: 512}        # ... into ranges no shorter than this
EPILOGUES = ("alpha", "accumulate", "colscale", "kscale", "lower_rect", "lower_compact", "mirror", "phi", "sub")
TAIL = 5                                          # NaN behind the last batch of every operand


def _even_up(x, least=2):
    """the smallest even number >= x + least"""
    return (x + least + 1) // 2 * 2


def _odd_up(x):
    """the smallest odd number > x"""
    return (x + 1) // 2 * 2 + 1


def make(name, M, N, K, batch=1, layout="nn", gemm_tile=0, strides="even", offset=0, bcast="", alpha=1.0, accumulate=False, colscale=False, kscale=False,
         lower=False, mirror=False, phi=False, sub=False, sym=False, kind="exact", no_syrk=0, a_ld=None, interleave=False, **expect):
    """strides: 'even' (every stride even, gaps included: 16-byte loads possible), 'odd' (odd leading dimensions and batch strides).  offset: elements the
    base pointers of A and B are moved by (1: 8 bytes off the 16-byte grid).  bcast: which of 'a', 'b' and 'k' (kscale) have batch stride 0.  sym: B is A itself, read
    transposed.  a_ld: the leading dimension of A where the case sets it itself.  interleave: the scale vectors of the outputs lie interleaved, element
    (b, k) at b + k (batch + 1), as the reverse pass hands them over (one slot per k is a gap); otherwise one vector behind the other."""
    assert set(expect) <= {"route", "tile", "vec", "split", "compact", "ksplit"} and len(layout) == 2
    ld = _even_up if strides == "even" else _odd_up
    a_rows, a_minor = (K, M) if layout[0] == "t" else (M, K)
    b_rows, b_minor = (N, K) if layout[1] == "t" else (K, N)
    a_ld = a_ld if a_ld is not None else ld(a_minor)
    b_ld = ld(b_minor)
    gap = 4 if strides == "even" else 3 + (a_rows * a_ld & 1)     # even: the batch stride stays even; odd: it comes out odd
    c = dict(name=name, M=M, N=N, K=K, batch=batch, layout=layout, gemm_tile=gemm_tile, no_syrk=no_syrk, kind=kind, sym=sym,
             alpha=float(alpha), accumulate=accumulate, colscale=colscale, kscale=kscale, lower=lower, mirror=mirror, phi=phi, sub=sub,
             a_off=offset, b_off=offset, a_rows=a_rows, a_minor=a_minor, a_ld=a_ld, b_rows=b_rows, b_minor=b_minor, b_ld=b_ld)
    c["a_bs"] = 0 if "a" in bcast else a_rows * a_ld + gap
    gap_b = 4 if strides == "even" else 3 + (b_rows * b_ld & 1)
    c["b_bs"] = 0 if "b" in bcast else b_rows * b_ld + gap_b
    c["a_rs"], c["a_cs"] = (1, a_ld) if layout[0] == "t" else (a_ld, 1)
    c["b_rs"], c["b_cs"] = (1, b_ld) if layout[1] == "t" else (b_ld, 1)
    if sym:      # B_b(k, j) = A_b(j, k): the same pointer, strides swapped
        assert M == N and layout in ("nt", "tn")
        c.update(b_rs=c["a_cs"], b_cs=c["a_rs"], b_bs=c["a_bs"], b_rows=a_rows, b_minor=a_minor, b_ld=a_ld)
    # C is a view into a wider buffer; so are the vectors
    c["c_rs"] = N + 3
    c["c_bs"] = M * c["c_rs"] + 7
    c["ks_bs"], c["cs_bs"], c["sv_bs"], c["sx_rs"] = 0 if "k" in bcast else K + 3, N + 2, M + 1, N + 1
    c["ks_s"] = c["cs_s"] = 1
    if interleave:
        assert "k" not in bcast
        c["ks_s"] = c["cs_s"] = batch + 1
        c["ks_bs"] = c["cs_bs"] = 1
    c["sx_bs"] = M * c["sx_rs"] + 2
    assert not ((colscale or kscale) and (sub or phi)), "one entry point takes the scales, the other the adjoint epilogues"
    assert not mirror or (lower and M == N)
    c["entry"] = "ex" if (sub or phi) else "strided"
    c["flags"] = int(lower) | int(mirror) << 1 | int(phi) << 2
    c["expect"] = dict({"route": GENERAL, "compact": False}, **expect)
    return c


def query(c, n_cus=256):
    """the flat query of dcgp_debug_plan_gemm for a case (device allocations are 16-byte aligned, so alignment is the offset's)"""
    q = dict(M=c["M"], N=c["N"], K=c["K"], batch=c["batch"], a_rs=c["a_rs"], a_cs=c["a_cs"], a_bs=c["a_bs"], b_rs=c["b_rs"], b_cs=c["b_cs"], b_bs=c["b_bs"],
             accumulate=c["accumulate"], colscale=c["colscale"], kscale=c["kscale"], sub=c["sub"], lower_only=c["lower"], mirror=c["mirror"], phi=c["phi"],
             a_aligned=c["a_off"] % 2 == 0, b_aligned=c["b_off"] % 2 == 0, same_ab=c["sym"], null_ptr=0, gemm_tile=c["gemm_tile"], no_syrk=c["no_syrk"],
             n_cus=n_cus)
    return [int(q[k]) for k in QUERY_FIELDS]


def plan(q):
    """dcgp_debug_plan_gemm's answer as a dict"""
    from deepcgp_amd import device as dev
    qa = (C.c_longlong * len(q))(*q)
    pa = (C.c_longlong * len(PLAN_FIELDS))()
    rc = dev.lib().dcgp_debug_plan_gemm(qa, len(q), pa, len(PLAN_FIELDS))
    assert rc == 0, rc
    return dict(zip(PLAN_FIELDS, pa))


def check_plan(c, p):
    """the plan p of case c against what the case declares; returns the mismatches"""
    e = c["expect"]
    want = dict(route=e["route"], error=0)
    if e["route"] == GENERAL:
        # (every leading dimension of the table is >= 2, so a stride of 1 is the layout's; the older tests' 1 x 1 x 1 product has all strides 1)
        want.update(tile=e["tile"], akf=int(c["a_cs"] == 1), bkf=int(c["b_rs"] == 1), lower_compact=int(e["compact"]))
        if "vec" in e:
            want["vec"] = int(e["vec"])
    got = {k: p[k] for k in want}
    if "split" in e:
        want["split"], got["split"] = bool(e["split"]), p["ksplit"] > 1
    if "ksplit" in e:
        want["ksplit"], got["ksplit"] = e["ksplit"], p["ksplit"]
    return {k: (want[k], got[k]) for k in want if want[k] != got[k]}


def epilogues(c):
    """which of EPILOGUES a case exercises"""
    e = c["expect"]
    out = {k for k in ("accumulate", "colscale", "kscale", "phi", "sub") if c[k]}
    if c["alpha"] != 1.0:
        out.add("alpha")
    if c["mirror"]:
        out.add("mirror")
    elif c["lower"] and not c["phi"]:
        out.add("lower_compact" if e.get("compact") else "lower_rect")
    return out


# ---- host data of a case -----------------------------------------------------------------------------------------------------------------------
def _view(buf, off, bs, rs, cs, batch, rows, cols):
    w = buf.itemsize
    return np.lib.stride_tricks.as_strided(buf[off:], (batch, rows, cols), (w * bs, w * rs, w * cs), writeable=True)


def _operand(off, bs, rows, ld, batch):
    nb = 1 if bs == 0 else batch
    return np.full(off + (nb - 1) * bs + rows * ld + TAIL, np.nan)


def build(c, rng):
    """The buffers of a case as they go to the device, every gap NaN, and the logical operands cut out of them.  Exact cases draw small integers (every
    product and partial sum an integer far below 2^53, so the double result does not depend on the order of summation); rounding cases standard normals."""
    M, N, K, batch = c["M"], c["N"], c["K"], c["batch"]
    if c["kind"] == "exact":
        def draw(shape):
            return rng.integers(-3, 4, size=shape).astype(np.float64)
    else:
        draw = rng.standard_normal
    d = {}
    d["A_buf"] = _operand(c["a_off"], c["a_bs"], c["a_rows"], c["a_ld"], batch)
    A = _view(d["A_buf"], c["a_off"], c["a_bs"], c["a_rs"], c["a_cs"], 1 if c["a_bs"] == 0 else batch, M, K)
    A[...] = draw(A.shape)
    if c["sym"]:
        d["B_buf"] = None
        B = np.transpose(A, (0, 2, 1))
    else:
        d["B_buf"] = _operand(c["b_off"], c["b_bs"], c["b_rows"], c["b_ld"], batch)
        B = _view(d["B_buf"], c["b_off"], c["b_bs"], c["b_rs"], c["b_cs"], 1 if c["b_bs"] == 0 else batch, K, N)
        B[...] = draw(B.shape)
    d["A"], d["B"] = A.copy(), B.copy()
    d["C_buf"] = draw(batch * c["c_bs"] + TAIL)
    d["C0"] = _view(d["C_buf"], 0, c["c_bs"], c["c_rs"], 1, batch, M, N).copy()
    inside = np.zeros(d["C_buf"].shape, bool)
    _view(inside, 0, c["c_bs"], c["c_rs"], 1, batch, M, N)[...] = True
    d["inside"] = inside

    def vector(key, on, bs, rows, rs, cols, es=1):
        d[key + "_buf"] = d[key] = None
        if on:
            d[key + "_buf"] = np.full((batch - 1) * bs + (rows - 1) * rs + max(cols - 1, 0) * es + 3 + TAIL, np.nan)
            v = _view(d[key + "_buf"], 0, bs, rs, es, batch, rows, cols)
            v[...] = draw(v.shape)
            d[key] = v.copy() if rows > 1 else v[:, 0, :].copy()
    vector("ks", c["kscale"], c["ks_bs"], 1, 0, K, c["ks_s"])
    vector("cs", c["colscale"], c["cs_bs"], 1, 0, N, c["cs_s"])
    vector("sv", c["sub"], c["sv_bs"], 1, 0, M)
    vector("sx", c["sub"], c["sx_bs"], M, c["sx_rs"], N)
    if c["sub"] and M == 1:
        d["sx"] = d["sx"][:, None, :]
    return d


def ref_args(c, d):
    """the operands and switches of gemm_ref.gemm / gemm_ref.magnitude for a built case"""
    ks = d["ks"][:1] if d["ks"] is not None and c["ks_bs"] == 0 else d["ks"]      # shared by the batch: one contraction
    return (d["A"], d["B"], d["C0"]), dict(kscale=ks, alpha=c["alpha"], accumulate=c["accumulate"], colscale=d["cs"], sub_v=d["sv"], sub_x=d["sx"],
                                            lower_only=c["lower"], mirror=c["mirror"], phi=c["phi"])


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
def _instantiation_cases():
    """every tile x layout x load width, direct and behind split-k: 16-byte loads (even strides, aligned base), and scalar loads reached once through an
    odd stride and once through a base 8 bytes off with even strides -- all 24 instantiations of gemm_gen_kernel.
    Per tile GT, (M, N) by layout: nn (GT + 1, GT - 1), tn (GT + 3, GT), nt (GT + 5, GT + 1), tt (GT + 7, GT + 2); batch 2; K = 33 direct, and split
    K = 1027 .. 1030 on the 32 tile, 2051 .. 2054 on the others (threshold + 3 + the layout's index), B shared by the two outputs."""
    out = []
    for gt in TILES:
        for li, lay in enumerate(LAYOUTS):
            for how, kw, vec in (("vec", dict(strides="even"), True), ("odd", dict(strides="odd"), False), ("off8", dict(strides="even", offset=1), False)):
                M, N = gt + 1 + 2 * li, gt - 1 + li       # two tile rows, one ragged tile column
                out.append(make("inst %d %s %s direct" % (gt, lay, how), M, N, 33, batch=2, layout=lay, gemm_tile=gt, tile=gt, vec=vec, split=False, **kw))
                # just past the split threshold and no multiple of 16: the last range is short and ends inside a k tile
                out.append(make("inst %d %s %s split" % (gt, lay, how), M, N, SPLIT_MIN_K[gt] + 3 + li, batch=2, layout=lay, gemm_tile=gt, bcast="b",
                                tile=gt, vec=vec, split=True, **kw))
    return out


def _ragged_cases():
    """M and N from {1, GT - 1, GT, GT + 1, 2 GT + 3}, K from {0, 1, 15, 16, 17, 33}; for the 64 tile (four-element fetch groups) also M or N = 2 mod 4
    with 16-byte loads: a group that is half valid.  K = 0 also behind the previous content, the scales, both lower_only grids and the mirrored store."""
    out = []
    for g in TILES:
        # (name prefix, M, N, K, layout, strides, further switches): every extent as M and as N, every K, every layout with both parities of the strides
        rows = (("ragged", 1, g - 1, 0, "nn", "even", dict(batch=2, alpha=-2.0)),
                ("ragged", g - 1, g + 1, 1, "tn", "odd", {}),
                ("ragged", g, 1, 15, "nt", "even", {}),
                ("ragged", g + 1, g, 16, "tt", "odd", dict(batch=2, accumulate=True)),
                ("ragged", 2 * g + 3, 2 * g + 3, 17, "nn", "even", {}),
                ("ragged", 1, g - 1, 33, "tn", "odd", {}),
                # the other pairing of the extents, the other parity of the strides
                ("ragged'", g + 1, 1, 33, "nt", "odd", {}),
                ("ragged'", 2 * g + 3, g - 1, 17, "tt", "even", {}),
                ("ragged'", 1, g, 16, "nn", "odd", {}),
                ("ragged'", g - 1, g + 1, 15, "tn", "even", {}),
                ("ragged'", g, 2 * g + 3, 1, "nt", "odd", {}))
        for pre, M, N, K, lay, strides, kw in rows:
            out.append(make("%s %d M%d N%d K%d %s" % (pre, g, M, N, K, lay), M, N, K, layout=lay, gemm_tile=g, strides=strides, tile=g, vec=(strides == "even"),
                            split=False, **kw))
        # K = 0 writes alpha 0 (+ C0): more than one row and tile, two outputs; with and without the previous content, behind the scales, and behind
        # lower_only on both grids (rectangular: zero above the diagonal; compact: C0 stays there) and the mirrored store
        S = g + 2
        for name, M, N, lay, strides, kw in (
                ("K0 accumulate", g + 1, g - 1, "nn", "even", dict(accumulate=True, alpha=-2.0)),
                ("K0 accumulate scales", g + 1, 5, "tt", "odd", dict(accumulate=True, colscale=True, kscale=True)),
                ("K0 overwrite", 3, g + 1, "tn", "odd", dict(alpha=4.0)),
                ("K0 lower rect", S, S, "nt", "even", dict(lower=True)),
                ("K0 lower compact", S, S, "tn", "even", dict(lower=True, accumulate=True, compact=True)),
                ("K0 mirror", S, S, "nn", "odd", dict(lower=True, mirror=True)),
                ("K0 mirror accumulate", S, S, "tt", "even", dict(lower=True, mirror=True, accumulate=True, compact=True))):
            out.append(make("%s %d %s" % (name, g, lay), M, N, 0, batch=2, layout=lay, gemm_tile=g, strides=strides, tile=g, vec=(strides == "even"), split=False,
                            **kw))
    # rows of A ('t': M is the contiguous index) and columns of B ('n') are fetched four at a time on the 64 tile
    out.append(make("half group 64 M66 tn", 66, 70, 17, layout="tn", gemm_tile=64, tile=64, vec=True, split=False))
    out.append(make("half group 64 N66 tn", 61, 66, 33, batch=2, layout="tn", gemm_tile=64, tile=64, vec=True, split=False))
    out.append(make("half group 64 N2 nn", 5, 2, 16, layout="nn", gemm_tile=64, tile=64, vec=True, split=False))
    out.append(make("half group 64 split tn", 66, 66, 2051, layout="tn", gemm_tile=64, tile=64, vec=True, split=True))
    return out


def _split_count_cases():
    """split counts below 8, a multiple of 8, and above 8 with a remainder (the reduction adds batches of 8 partials, then a tail), on each tile.
    tile 32 (1024 slots, ranges >= 128): 4 tiles; K = 1027 -> at most 8 ranges of 144 (the last 19 columns), K = 1500 -> 11 of 144 (the last 60);
    200 tiles -> 5 ranges of 208.  tiles 64 / 128 (1024 / 512 slots, ranges >= 512): K = 2051 -> 4 of 528 (the last 467), K = 4099 -> 8 of 528 (403),
    K = 5700 -> 11 of 528 (420)."""
    out = []
    out.append(make("splits 32 x8", 40, 40, 1027, layout="nt", gemm_tile=32, kscale=True, tile=32, vec=True, split=True, ksplit=8))
    out.append(make("splits 32 x11", 40, 40, 1500, layout="tn", gemm_tile=32, tile=32, vec=True, split=True, ksplit=11))
    out.append(make("splits 32 x5", 33, 40, 1027, batch=50, layout="nn", gemm_tile=32, strides="odd", bcast="ab", kscale=True, tile=32, vec=False, split=True, ksplit=5))
    for gt in (64, 128):
        out.append(make("splits %d x4" % gt, gt + 2, gt + 1, 2051, layout="tt", gemm_tile=gt, strides="odd", tile=gt, vec=False, split=True, ksplit=4))
        out.append(make("splits %d x8" % gt, gt + 2, gt, 4099, layout="nn", gemm_tile=gt, tile=gt, vec=True, split=True, ksplit=8))
        out.append(make("splits %d x11" % gt, gt, gt + 2, 5700, batch=2, layout="nt", gemm_tile=gt, bcast="ab", kscale=True, tile=gt, vec=True, split=True,
                        ksplit=11))
    return out


def _epilogue_cases():
    """each epilogue on each tile, direct and behind split-k, batch 2; the split cases broadcast B over the batch.  Lower-triangular results take 3 x 3 tiles,
    so that the compact grid's index arithmetic sees an inner row."""
    # the layout of each epilogue's case, the same on every tile: direct and split differ, and every layout serves several epilogues
    layouts = {False: dict(alpha="tn", accumulate="nt", colscale="tt", kscale="nn", sub="tn", phi="nt", lower_rect="tt", mirror_rect="nn", lower_compact="tn",
                           mirror_compact="nt", all_scales="tt"),
               True: dict(alpha="nn", accumulate="tn", colscale="nt", kscale="tt", sub="nn", phi="tn", lower_compact="nt", mirror_compact="tt", all_scales="nn")}
    out = []
    for gt in TILES:
        for split in (False, True):
            K = SPLIT_MIN_K[gt] + 5 if split else 33
            sw = dict(batch=2, gemm_tile=gt, bcast="b" if split else "", tile=gt, split=split)
            tag = "%d %s" % (gt, "split" if split else "direct")
            lay = layouts[split]
            M, N, S = gt + 5, gt - 3, 2 * gt + 3      # rectangular results M x N (phi: M x M), triangular ones S x S
            out.append(make("alpha " + tag, M, N, K, layout=lay["alpha"], alpha=-0.5, vec=True, **sw))
            out.append(make("accumulate " + tag, M, N, K, layout=lay["accumulate"], accumulate=True, vec=True, **sw))
            out.append(make("colscale " + tag, M, N, K, layout=lay["colscale"], colscale=True, vec=True, **sw))
            out.append(make("kscale " + tag, M, N, K, layout=lay["kscale"], kscale=True, vec=True, **sw))
            out.append(make("sub " + tag, M, N, K, layout=lay["sub"], sub=True, alpha=2.0, vec=True, **sw))
            out.append(make("phi " + tag, M, M, K, layout=lay["phi"], phi=True, strides="odd", vec=False, **sw))
            if not split:
                out.append(make("lower rect " + tag, S, S, K, layout=lay["lower_rect"], lower=True, vec=True, compact=False, **sw))
                out.append(make("mirror rect " + tag, S, S, K, layout=lay["mirror_rect"], lower=True, mirror=True, strides="odd", vec=False, compact=False, **sw))
            out.append(make("lower compact " + tag, S, S, K, layout=lay["lower_compact"], lower=True, accumulate=not split, vec=True, compact=True, **sw))
            # mirror with accumulate: the lower triangle accumulates, the upper one is its mirror image
            out.append(make("mirror compact " + tag, S, S, K, layout=lay["mirror_compact"], lower=True, mirror=True, accumulate=True, alpha=-1.0, vec=True,
                            compact=True, **sw))
            out.append(make("mirror sym " + tag, S, S, K, layout="nt", sym=True, lower=True, mirror=True, kscale=True, interleave=True, compact=split, **sw))
            out.append(make("all scales " + tag, M, N, K, layout=lay["all_scales"], alpha=4.0, accumulate=True, colscale=True, kscale=True, strides="odd",
                            interleave=True, vec=False, **sw))
    return out


def _rounding_cases():
    """standard-normal operands, one per tile, direct and split: the derived rounding bound of tests/test_gpu_gemm.py instead of equality.
    (GT + 3) x (GT + 1); direct K = 97 with every scale, layouts nn / tn / nt for tiles 32 / 64 / 128; split K = threshold + 7 with the sub correction,
    layouts tn / nt / tt."""
    out = []
    for i, gt in enumerate(TILES):
        out.append(make("rounding %d direct" % gt, gt + 3, gt + 1, 97, layout=LAYOUTS[i], gemm_tile=gt, kind="rounding", alpha=0.7, accumulate=True, colscale=True,
                        kscale=True, tile=gt, vec=True, split=False))
        out.append(make("rounding %d split" % gt, gt + 3, gt + 1, SPLIT_MIN_K[gt] + 7, layout=LAYOUTS[i + 1], gemm_tile=gt, kind="rounding", alpha=-1.3, sub=True,
                        tile=gt, vec=True, split=True))
    return out


def _natural_cases():
    """gemm_tile = 0: the dispatch of gemm_gen() itself reaching the 64 and 128 tiles, and one pair on either side of each of its thresholds.  Operands are
    broadcast over the batch, the scales of k included (bcast 'k'), so the large batches cost only their results."""
    nat = dict(gemm_tile=0, bcast="abk", colscale=True)      # (what differs from output to output is the column scale and the previous content)
    out = [
        make("natural 64", 200, 200, 40, batch=30, layout="nn", tile=64, vec=True, split=False, **nat),
        make("natural 64 split", 66, 200, 2100, batch=20, layout="tn", kscale=True, tile=64, vec=True, split=True, **nat),
        make("natural 128 split", 130, 130, 8192, batch=8, layout="nt", kscale=True, tile=128, vec=True, split=True, **nat),
        make("natural 128 lower compact", 130, 130, 8192, batch=16, layout="nt", lower=True, kscale=True, tile=128, vec=True, split=True, compact=True, **nat),
        # the 128 tile's fill condition: 4 tiles of 128 x batch x (K / 512) >= 512, K >= 4096, M and N >= 128
        make("fill 128: batch 16", 130, 130, 4096, batch=16, layout="nn", tile=128, vec=True, split=True, **nat),
        make("fill 128: batch 15", 130, 130, 4096, batch=15, layout="nn", tile=64, vec=True, split=True, **nat),
        make("fill 128: K 4096", 130, 130, 4096, batch=19, layout="tt", tile=128, vec=True, split=True, **nat),
        make("fill 128: K 4095", 130, 130, 4095, batch=19, layout="tt", strides="odd", tile=64, vec=False, split=True, **nat),
        make("fill 128: M 128", 128, 130, 4096, batch=32, layout="nn", tile=128, vec=True, split=True, **nat),
        make("fill 128: M 127", 127, 130, 4096, batch=32, layout="nn", strides="odd", tile=64, vec=False, split=True, **nat),
        # what the 64 tile could launch, split included: <= 256 workgroups take the 32 tile
        make("small 32: 4 x 64", 65, 65, 20, batch=64, layout="nt", tile=32, vec=True, split=False, **nat),
        make("small 64: 4 x 65", 65, 65, 20, batch=65, layout="nt", tile=64, vec=True, split=False, **nat),
        make("small 32: 64 x 4 ranges", 64, 64, 2048, batch=64, layout="tn", kscale=True, tile=32, vec=True, split=True, **nat),
        make("small 64: 65 x 4 ranges", 64, 64, 2048, batch=65, layout="tn", kscale=True, tile=64, vec=True, split=True, **nat),
        # the split thresholds: K = 1024 on the 32 tile, 2048 on the 64 tile; on the 128 tile (K >= 4096 always) the tiles that leave room for two ranges
        make("split 32: K 1023", 40, 40, 1023, batch=2, layout="nn", strides="odd", kscale=True, tile=32, vec=False, split=False, gemm_tile=0),
        make("split 32: K 1024", 40, 40, 1024, batch=2, layout="nn", kscale=True, tile=32, vec=True, split=True, gemm_tile=0),
        make("split 64: K 2047", 66, 66, 2047, batch=70, layout="nt", strides="odd", tile=64, vec=False, split=False, **nat),
        make("split 64: K 2048", 66, 66, 2048, batch=70, layout="nt", tile=64, vec=True, split=True, **nat),
        make("split 128: 256 tiles", 130, 130, 4096, batch=64, layout="tn", kscale=True, tile=128, vec=True, split=True, ksplit=2, **nat),
        make("split 128: 260 tiles", 130, 130, 4096, batch=65, layout="tn", kscale=True, tile=128, vec=True, split=False, **nat),
    ]
    return out


def _syrk_case(M, K, batch, a_ld, route, name=None, **kw):
    """A diag(ks_b) A^T, lower triangle mirrored: the reverse pass's W_r.  A is shared by the batch (batch stride 0), the scales differ per batch."""
    e = dict(route=route)
    if route == GENERAL:
        e.update(tile=kw.pop("tile"), split=True, compact=True)
    return make(name or "syrk M%d K%d b%d ld+%d" % (M, K, batch, a_ld - K), M, M, K, batch=batch, layout="nt", sym=True, a_ld=a_ld, kscale=True,
                lower=True, mirror=True, alpha=2.0, **dict(dict(bcast="ab"), **dict(kw, **e)))


def _syrk_cases():
    """M in {129, 130, 200, 255, 256}, K in {8192, 8193, 8222, 11520}, batch in {1, 3}; the row stride K itself where K is even, otherwise and besides K + 2 or
    K + 6 (K = 8193 is odd, and the kernel's 16-byte loads need an even stride: K + 3 and K + 7 there), the gap NaN; the scales of three outputs interleaved as grad.hip passes them, or one vector behind the other.  Not the full product: every value of
    every factor, each K with a tight (where it can be) and a padded row, three outputs at the smallest and the largest M.  Then the neighbours just outside the kernel's range."""
    out = [_syrk_case(M, K, b, K + pad, SYRK, interleave=(b > 1 and M != 130)) for M, K, b, pad in (
        (129, 8192, 3, 0), (130, 8193, 3, 3), (200, 8222, 1, 2), (255, 11520, 1, 6), (256, 8192, 3, 2), (256, 8222, 1, 0), (200, 8193, 1, 7),
        (130, 8192, 1, 6), (256, 11520, 1, 0), (129, 11520, 3, 2), (255, 8222, 1, 6))]
    # every output with an A of its own (the reverse pass shares one A between the outputs: batch stride 0, as above)
    out.append(_syrk_case(129, 8192, 3, 8194, SYRK, name="syrk M129 K8192 b3 ld+2 own A", bcast="", interleave=True))
    out += [
        _syrk_case(128, 8192, 1, 8192, GENERAL, name="not syrk: M 128", tile=32),
        _syrk_case(130, 8191, 1, 8192, GENERAL, name="not syrk: K 8191", tile=32),
        _syrk_case(130, 8192, 1, 8193, GENERAL, name="not syrk: odd row stride", strides="odd", tile=32),
        _syrk_case(130, 8192, 65, 8192, GENERAL, name="not syrk: batch 65", bcast="abk", accumulate=True, tile=128),
        _syrk_case(130, 8192, 3, 8194, GENERAL, name="not syrk: no_syrk", no_syrk=1, tile=32),
    ]
    return out


def _legacy(name, M, N, K, batch=1, ksplit=1, **kw):
    """a run(...) of the two older kernel-level tests of tests/test_gpu_ops.py: contiguous operands, whatever parity the extents give"""
    c = make(name, M, N, K, batch=batch, tile=32, split=ksplit > 1, ksplit=ksplit, **kw)
    lay = c["layout"]
    c.update(a_ld=c["a_minor"], b_ld=c["b_minor"], a_bs=M * K, b_bs=K * N)
    c["a_rs"], c["a_cs"] = (1, M) if lay[0] == "t" else (K, 1)
    c["b_rs"], c["b_cs"] = (1, K) if lay[1] == "t" else (N, 1)
    return c


def legacy_cases():
    """test_strided_gemm_layouts_edges_and_epilogues (every layout) and test_strided_gemm_adjoint_epilogues with the configuration each run takes today:
    the 32 tile throughout, since the narrow long contractions were moved to it"""
    out = []
    for lay in LAYOUTS:
        t = "layouts[%s] " % lay
        out += [_legacy(t + "1,1,1", 1, 1, 1, layout=lay), _legacy(t + "37,53,19", 37, 53, 19, batch=3, layout=lay, alpha=-0.5),
                _legacy(t + "64,64,16", 64, 64, 16, layout=lay, accumulate=True),
                _legacy(t + "65,129,33", 65, 129, 33, layout=lay, colscale=True, kscale=True),
                _legacy(t + "96,96,40 lower", 96, 96, 40, batch=2, layout=lay, lower=True, compact=False),
                _legacy(t + "96,96,40 lower acc", 96, 96, 40, batch=2, layout=lay, lower=True, accumulate=True, compact=True),
                _legacy(t + "20,7,5000", 20, 7, 5000, layout=lay, kscale=True, ksplit=35),
                _legacy(t + "130,130,4100 lower", 130, 130, 4100, batch=2, layout=lay, lower=True, alpha=2.0, ksplit=29, compact=True),
                _legacy(t + "256,25,9000", 256, 25, 9000, layout=lay, accumulate=True, ksplit=63)]
    t = "adjoint "
    out += [_legacy(t + "37,53,19", 37, 53, 19, batch=2, alpha=0.7, sub=True), _legacy(t + "256,25,9000", 256, 25, 9000, accumulate=True, sub=True, ksplit=63),
            _legacy(t + "70,70,33 phi", 70, 70, 33, batch=3, phi=True), _legacy(t + "40,40,3000 phi", 40, 40, 3000, phi=True, alpha=-1.0, ksplit=21),
            _legacy(t + "96,96,40 mirror", 96, 96, 40, batch=2, lower=True, mirror=True, compact=False),
            _legacy(t + "130,130,4100 mirror", 130, 130, 4100, batch=2, lower=True, mirror=True, alpha=2.0, ksplit=29, compact=True)]
    return out


def all_cases():
    out = _instantiation_cases() + _ragged_cases() + _split_count_cases() + _epilogue_cases() + _rounding_cases() + _natural_cases() + _syrk_cases()
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return out


CASES = all_cases()


def forced(tile, layout):
    """the cases of one (tile, layout) parametrisation of the GPU test"""
    return [c for c in CASES if c["gemm_tile"] == tile and c["layout"] == layout]


def natural():
    return [c for c in CASES if c["gemm_tile"] == 0 and not c["name"].startswith(("syrk", "not syrk"))]


def syrk():
    return [c for c in CASES if c["name"].startswith(("syrk", "not syrk"))]

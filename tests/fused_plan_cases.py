"""The layer kernel's launch plan seen from Python (csrc/fused_plan.h through dcgp_debug_plan_layer_launch): the flat field orders of include/dcgp.h, a query
built from a layer's geometry the way csrc/layer_impl.h builds it, and the queries of the recorded table (tests/fused_plan_table.json)."""
import ctypes as C
import struct

QUERY_FIELDS = ("Mp", "M", "R", "Rp", "Kc", "P", "HWC", "L", "Lp", "Lz", "f", "C", "n_mod", "rep", "base", "has_G", "keeps_state", "has_trace", "n_cus",
                "fused_shape", "fused_large", "fused_split", "fused_persist", "fused_pre", "fused_parts", "fused_rep_share", "fused_wgs", "fused_stagger",
                "sweep_no_rows")
OPTION_DEFAULTS = dict(fused_shape=-1, fused_large=0, fused_split=-1, fused_persist=-1, fused_pre=-1, fused_parts=-1, fused_rep_share=-1, fused_wgs=0,
                       fused_stagger=-1, sweep_no_rows=0)
PLAN_FIELDS = ("ok", "shape", "lds", "lds_main", "lds_img", "grid", "persist", "n_strips", "n_items", "deal", "split_first", "split_q", "pre_n", "pre_first",
               "pre_sq", "pre_D", "pre_whole", "pre_stride", "stagger", "cu_slots", "patch_rows", "units_plain", "units_ahead", "units_shared")
UNITS = ("units_plain", "units_ahead", "units_shared")     # doubles, bit-cast into their int64 slot
BASES = {"rbf": 0, "acos": 1, "matern32": 2, "matern52": 3}


def _up(x, m):
    return (x + m - 1) // m * m


def layer_query(hwc, f, s, M, R, rows, n_mod, n_cus, base="rbf", has_G=1, keeps_state=0, has_trace=0, rep=1, **options):
    """The query of a conv layer with an f x f filter at stride s over `rows` images of shape hwc, of which n_mod are distinct"""
    H, W, Cc = hwc
    P = ((H - f) // s + 1) * ((W - f) // s + 1)
    L = f * f * Cc
    q = dict(OPTION_DEFAULTS)
    assert set(options) <= set(q), options
    q.update(options)
    q.update(Mp=_up(M, 16), M=M, R=R, Rp=_up(R, 16), Kc=min(rows * P, 0x7fffffff), P=P, HWC=H * W * Cc, L=L, Lp=_up(L, 4), Lz=_up(L + 2, 4), f=f, C=Cc,
             n_mod=n_mod, rep=rep, base=BASES[base], has_G=has_G, keeps_state=keeps_state, has_trace=has_trace, n_cus=n_cus)
    return [int(q[k]) for k in QUERY_FIELDS]


def plan(query):
    """dcgp_debug_plan_layer_launch's answer as a dict"""
    from deepcgp_amd import device as dev
    qa = (C.c_longlong * len(query))(*query)
    pa = (C.c_longlong * len(PLAN_FIELDS))()
    rc = dev.lib().dcgp_debug_plan_layer_launch(qa, len(query), pa, len(PLAN_FIELDS))
    assert rc == 0, rc
    out = dict(zip(PLAN_FIELDS, pa))
    for k in UNITS:
        out[k] = struct.unpack("<d", struct.pack("<q", out[k]))[0]
    return out


def debug_plan_of(p):
    """what dcgp_debug_fused_plan reports for a launch dealt by plan p"""
    return (p["persist"], p["n_items"] if p["persist"] else 0, p["pre_n"], p["pre_D"])


def ctx_query(ctx, hwc, f, s, M, R, rows, n_mod, **kw):
    """layer_query for a launch on the ctx's device under the ctx's options of the moment"""
    return layer_query(hwc, f, s, M, R, rows, n_mod, ctx.get_option("n_cus"), **dict({k: ctx.get_option(k) for k in OPTION_DEFAULTS}, **kw))


def last_launch(ctx):
    """dcgp_debug_fused_plan: (workgroups, items, hand-over slots, distinct strips D of the shared plan or 0) of the ctx's most recent layer-kernel launch"""
    from deepcgp_amd import device as dev
    out = (C.c_int * 4)()
    assert dev.lib().dcgp_debug_fused_plan(ctx.handle, out) == 0
    return tuple(out)


MNIST = (28, 28, 1)
SMALL = (12, 12, 1)        # tests/test_gpu_fused_rep_share.py: f = 5, s = 2 gives 16 patches per image

# every parametrisation of tests/test_gpu_fused_rep_share.py: (M, R, N, S, fused_shape, fused_wgs, expected D)
REP_SHARE_CASES = [
    (32, 3, 4, 3, 6, 4, 4), (32, 3, 4, 3, 6, 5, 4), (256, 10, 4, 3, 6, 4, 4), (256, 3, 4, 3, 6, 5, 4), (256, 10, 8, 3, 0, 2, 2), (32, 10, 8, 6, 0, 4, 2),
    (32, 3, 8, 3, 6, 3, 8), (256, 3, 8, 4, 6, 3, 8), (32, 3, 4, 5, 0, 2, 1), (256, 10, 4, 6, 0, 2, 1),
    (32, 3, 3, 4, 0, 2, 0), (256, 10, 3, 4, 0, 2, 0), (32, 3, 5, 3, 0, 3, 0), (256, 10, 5, 3, 0, 2, 0),
    (256, 10, 8, 4, 0, 3, 0), (32, 10, 4, 4, 0, 3, 0),
    (32, 3, 12, 1, 6, 4, 0),
    (32, 3, 4, 3, 6, 4, 4), (32, 3, 4, 5, 0, 2, 1),
]


def rep_share_query(M, R, N, S, shape, wgs, n_cus=256, base="rbf", **options):
    return layer_query(SMALL, 5, 2, M, R, N * S, N, n_cus, base=base, fused_shape=shape, fused_persist=1, fused_wgs=wgs, **options)


def table_cases():
    """(name, query) of the recorded table"""
    out = []
    cfg2 = dict(hwc=MNIST, f=5, s=1, M=256, R=10, rows=80, n_mod=8, n_cus=256)     # P = 576, Kc = 46 080: 720 strips of 64 columns
    out.append(("cfg2", layer_query(**cfg2)))
    out.append(("cfg2 at stride 2", layer_query(MNIST, 5, 2, 256, 10, 320, 32, 256)))     # the same column count from 32 images, 10 samples, 144 patches
    out.append(("cfg2 keeps_state", layer_query(keeps_state=1, **cfg2)))
    out.append(("cfg2 trace", layer_query(has_trace=1, **cfg2)))
    for opt, vals in (("fused_rep_share", (0,)), ("fused_pre", (0, 3, 9)), ("fused_persist", (0, 1, 2))):
        for v in vals:
            out.append(("cfg2 %s=%d" % (opt, v), layer_query(**dict(cfg2, **{opt: v}))))
    for s in (1, 2):           # the shards of that batch, and of the same batch at stride 2 (P = 144: 90 strips of 64 columns at 4 images)
        for n in (4, 8, 16):
            for shape in (-1, 0):
                for parts in (-1, -2, 2, 5):
                    out.append(("shard s=%d n=%d shape=%d parts=%d" % (s, n, shape, parts),
                                layer_query(MNIST, 5, s, 256, 10, 10 * n, n, 256, fused_shape=shape, fused_parts=parts)))
            out.append(("shard s=%d n=%d split=0" % (s, n), layer_query(MNIST, 5, s, 256, 10, 10 * n, n, 256, fused_split=0)))
            out.append(("shard s=%d n=%d split=3" % (s, n), layer_query(MNIST, 5, s, 256, 10, 10 * n, n, 256, fused_split=3)))
    for large in (0, 1):
        for M in (384, 1024):
            out.append(("M=%d fused_large=%d" % (M, large), layer_query(MNIST, 5, 1, M, 10, 80, 8, 256, fused_large=large)))
    out.append(("Kc=1<<23", layer_query(SMALL, 5, 2, 32, 3, 1 << 19, 1 << 19, 256)))
    out.append(("Kc=(1<<23)-16", layer_query(SMALL, 5, 2, 32, 3, (1 << 19) - 1, (1 << 19) - 1, 256)))
    out.append(("long patches", layer_query((12, 12, 10), 5, 1, 256, 10, 80, 8, 256)))
    out.append(("long patches sweep_no_rows", layer_query((12, 12, 10), 5, 1, 256, 10, 80, 8, 256, sweep_no_rows=1)))
    out.append(("no q_sqrt", layer_query(MNIST, 5, 2, 256, 10, 40, 4, 256, has_G=0)))
    out.append(("two per CU persist", layer_query(MNIST, 5, 1, 32, 10, 400, 40, 256, fused_shape=2, fused_persist=1)))
    out.append(("two per CU stagger=0", layer_query(MNIST, 5, 1, 32, 10, 400, 40, 256, fused_shape=2, fused_persist=1, fused_stagger=0)))
    out.append(("104 CUs", layer_query(MNIST, 5, 1, 256, 10, 80, 8, 104)))
    out.append(("rep=10", layer_query(MNIST, 5, 1, 256, 10, 80, 8, 256, rep=10)))
    for i, (M, R, N, S, shape, wgs, D) in enumerate(REP_SHARE_CASES):
        for share in (-1, 0):
            out.append(("rep_share %d share=%d" % (i, share), rep_share_query(M, R, N, S, shape, wgs, fused_rep_share=share)))
    for base in ("matern32", "matern52", "acos"):
        for M, R, N, S, shape, wgs in ((32, 3, 4, 3, 6, 5), (256, 10, 8, 3, 0, 2)):
            out.append(("rep_share %s M=%d" % (base, M), rep_share_query(M, R, N, S, shape, wgs, base=base)))
    # the rows of the simulated deal quoted with the plans: strips / workgroups / R (16-column strips, one image each)
    for strips, wgs, R, n_mod in ((12, 4, 3, 4), (9, 4, 3, 3), (10, 4, 2, 5), (17, 4, 10, 17)):
        out.append(("deal %d/%d R=%d" % (strips, wgs, R), layer_query(SMALL, 5, 2, 32, R, strips, n_mod, 256, fused_shape=6, fused_persist=1, fused_wgs=wgs)))
    return out

"""The cases of the factorisation chain's operator tests (csrc/chol_fused.hip through dcgp_debug_factor_chain) and what each DECLARES it reaches.

A batch is a list of entries, one per matrix: what rides on that matrix's chain (csrc/common.h, ChainRhs).  A case is a batch at a size M (Mp = M rounded up
to 16).  tests/test_host_chain_plan.py holds every declaration against csrc/chain_plan.h (through dcgp_debug_plan_chain: the launch arithmetic and the
decodes the library itself runs) and enumerates the planner; tests/test_gpu_chain.py runs the cases against tests/chain_ref.py.  The declarations are
written down from the shapes, never read back from the planning function."""
import ctypes as C

import numpy as np

QUERY_FIELDS = ("Mp", "batch", "jp", "has_inv", "rides", "max_R", "alone", "no_iso")
PLAN_FIELDS = ("np", "j", "nt", "nT", "nct", "la_idx", "has_xla", "has_xin", "has_xnext", "has_xself", "has_rhs", "rhs_p", "rhs_last", "rhs_nt", "rhs_tpw",
               "rhs_ng", "rhs_nq", "rhs_base", "gx", "iso_per", "grid_x", "grid_y", "iso", "n_wgs")
EXIT, TRAILING, INVERSE, LOOKAHEAD, DIAG_ONLY, RHS = range(6)      # kinds of a workgroup (include/dcgp.h, dcgp_debug_plan_chain)
MAX_RIDE_MP = 256                                                  # kChainRhsMaxMp


def round_up(x, m):
    return (x + m - 1) // m * m


def plan(Mp, batch, jp, has_inv=1, rides=0, max_R=0, alone=1, no_iso=0, R_of=None, want_wgs=False):
    """dcgp_debug_plan_chain's answer: the plan as a dict and, with want_wgs, the [workgroups][8] table {b, bx, kind, q / rt, ct, g, final_only, first row tile}"""
    from deepcgp_amd import device as dev
    q = [Mp, batch, jp, has_inv, rides, max_R, alone, no_iso]
    qa = (C.c_longlong * len(q))(*[int(v) for v in q])
    pa = (C.c_longlong * len(PLAN_FIELDS))()
    ra = (C.c_longlong * batch)(*[int(r) for r in R_of]) if R_of is not None else None
    L = dev.lib()
    rc = L.dcgp_debug_plan_chain(qa, len(q), ra, batch if ra is not None else 0, pa, len(PLAN_FIELDS), None, 0)
    assert rc == 0, (rc, q)
    p = dict(zip(PLAN_FIELDS, pa))
    if not want_wgs:
        return p
    wgs = np.zeros((p["n_wgs"], 8), np.int64)
    rc = L.dcgp_debug_plan_chain(qa, len(q), ra, batch if ra is not None else 0, pa, len(PLAN_FIELDS), wgs.ctypes.data, p["n_wgs"])
    assert rc == 0, (rc, q)
    return p, wgs


# ---- batches ----------------------------------------------------------------------------------------------------------------------------------------
def entry(R, Lq=True, qmu=True, G=True, alpha=True, Rp=None, share=None):
    """One matrix of a batch: R right-hand sides Lq_r (Lq) and q_mu (qmu) ride its chain; G / alpha: the results are stored (False: sums only).
    share = i: Lq and q_mu are entry i's buffers (a prior's chain carries the layer's own right-hand sides)."""
    return dict(R=R, Rp=Rp if Rp is not None else round_up(R, 16), Lq=Lq, qmu=qmu, G=G and Lq, alpha=alpha and qmu, share=share)


def nothing(R=10):
    return entry(R, Lq=False, qmu=False)


def carries(e):
    return e["Lq"] or e["qmu"]


BATCHES = {
    "a": [entry(1)],                                                            # one matrix, R = 1
    "b": [entry(10), entry(10, G=False, alpha=False, share=0), nothing()],      # riding in full; a prior's entry (sums only); nothing
    "c": [entry(3, Lq=False)],                                                  # only alpha rides
    "d6": [entry(10) for _ in range(6)],                                        # two row tiles per workgroup: six riding matrices, R = 10
    "d2": [entry(32), entry(32)],                                               # ... two at R = 32, Rp = 32
    # ... and on every launch from the first lagged panel on, where four row tiles make two groups of two (the cases above take two tiles per workgroup
    # only from three tiles down, where the second group has one): the batch's largest R sizes the launch, the matrices of smaller R leave slots idle
    "d4": [entry(1), entry(32), entry(3), entry(1)],
    "e": [entry(3), entry(10), entry(1)],                                       # matrices differing in R, the largest not first
    "plain": [nothing(0)],                                                      # no right-hand sides (with or without the inverse)
}
RIDE_SIZES = (16, 32, 41, 48, 64, 96, 128, 144, 176, 200, 240, 256)             # M; 41 -> Mp 48 and 200 -> Mp 208 through padding; 1 .. 8 panels


def case_id(batch, M):
    return "%s@%d" % (batch, M)


# (batch, M, inverse formed) of every GPU case
RIDE_CASES = [(b, M) for b in ("a", "b", "c", "e") for M in RIDE_SIZES] + [("d6", 256), ("d2", 256), ("d2", 240), ("d4", 256)]
LARGE_CASES = [("plain", 384), ("plain", 1000)]                                 # no right-hand sides, with the inverse (1000 -> Mp 1008: a ragged last panel)
PLAIN_FACTOR_CASE = ("plain", 144)                                              # Linv == NULL: the last launch has gx == 0
STATUS_MP = 144                                                                 # status-word cases: batch "b", five panels, the last ragged (16 columns)
STATUS_COLUMNS = {"panel 0": 5, "middle panel": 70, "ragged last panel": 133, "first column of a panel": 64}      # 0-based column of the -1

# What the cases declare (tests/test_host_chain_plan.py holds the planner to it).  Launches jp whose right-hand sides take two row tiles per workgroup:
# batch (max_R jp + 1) rhs_nt > 400 with rhs_nt = ceil((Mp - 32 jp) / 64).
#   d6@256: 6 (10 jp + 1) nt = 264, 378, 558, 492, 612, 366, 426 for jp = 1 .. 7 (nt = 4, 3, 3, 2, 2, 1, 1)
#   d2@256, d2@240: 2 (32 jp + 1) nt = 264, 390, 582, 516, 644, 386, 450 (the same nt: 240 - 32 jp rounds up to the same tiles)
#   d4@256: 4 (32 jp + 1) nt = 528, 780, 1164, 1032, 1288, 772, 900: every launch that carries right-hand sides, the first with nt = 4
#   every other case stays below: the largest is e@256 / b@256 at jp = 5, 3 (10 * 5 + 1) 2 = 306
TPW2_LAUNCHES = {"d6@256": {3, 4, 5, 7}, "d2@256": {3, 4, 5, 7}, "d2@240": {3, 4, 5, 7}, "d4@256": {1, 2, 3, 4, 5, 6, 7}}
TPW2_ROW_TILES = {1, 2, 3, 4}      # counts of row tiles that the cases' two-tiles-per-workgroup launches see between them


def declared(batch, M, has_inv=True):
    """What a case declares: panels, launches with two row tiles per workgroup, whether right-hand sides ride, whether the look-ahead workgroups exist."""
    Mp = round_up(M, 16)
    ents = BATCHES[batch]
    rides = any(carries(e) for e in ents)
    np_ = (Mp + 31) // 32
    return dict(Mp=Mp, np=np_, rides=rides, max_R=max([e["R"] for e in ents if carries(e)], default=0), tpw2=TPW2_LAUNCHES.get(case_id(batch, M), set()),
                lookahead=has_inv and np_ > 1, one_panel=np_ == 1, ragged=Mp % 32 != 0)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------
_KUU = {}


def realistic_kuu(M, seed):
    """Kuu of the realistic ill-conditioned inducing patches of synthetic.make_spec (tests/test_gpu_ops.py, test_kuu_potrf_trtri_realistic_large_M): RBF
    variance 5, lengthscale 5, jitter 1e-3"""
    if (M, seed) not in _KUU:
        from deepcgp_amd import synthetic as syn
        Z = syn.make_spec((28, 28, 1), [(5, 2, 10)], (5, 1), M=M, S=1, seed=seed)["convs"][0]["Z"]
        Zs = Z / 5.0
        d = np.sum(Zs * Zs, 1)[:, None] + np.sum(Zs * Zs, 1)[None, :] - 2.0 * Zs @ Zs.T
        K = 5.0 * np.exp(-0.5 * np.maximum(d, 0.0))
        K = 0.5 * (K + K.T) + 1e-3 * np.eye(M)
        _KUU[(M, seed)] = K
    return _KUU[(M, seed)].copy()


def random_spd(rng, M):
    W = rng.standard_normal((M, M + 8))
    return W @ W.T / (M + 8) + np.eye(M)


def pad_spd(K, Mp):
    """as the library pads: the identity on the padded diagonal"""
    M = K.shape[0]
    out = np.eye(Mp)
    out[:M, :M] = K
    return out


def build(batch, M, seed=0):
    """Host inputs of a case, padded as the library pads them: A [batch][Mp][Mp] (matrix 0 and every third one the realistic Kuu, the others random
    well-conditioned SPD), and per entry Lq [R][Mp][Mp] (lower triangular, unit-ish diagonal, as rand_spd_inputs of tests/test_gpu_ops.py) and qmu [Mp][Rp],
    zero in the padded rows and columns."""
    ents = BATCHES[batch]
    Mp = round_up(M, 16)
    rng = np.random.default_rng(1000 * M + 7 * len(ents) + seed)
    A = np.stack([pad_spd(realistic_kuu(M, 77 + i) if i % 3 == 0 else random_spd(rng, M), Mp) for i in range(len(ents))])
    Lq, qmu = [], []
    for i, e in enumerate(ents):
        lq = np.zeros((e["R"], Mp, Mp))
        lq[:, :M, :M] = np.tril(rng.standard_normal((e["R"], M, M))) * 0.5 + np.eye(M)[None]
        mu = np.zeros((Mp, e["Rp"]))
        mu[:M, :e["R"]] = rng.standard_normal((M, e["R"]))
        if e["share"] is not None:
            lq, mu = Lq[e["share"]], qmu[e["share"]]
        Lq.append(lq if e["Lq"] else None)
        qmu.append(mu if e["qmu"] else None)
    return dict(batch=batch, ents=ents, M=M, Mp=Mp, A=A, Lq=Lq, qmu=qmu)


def subset(inp, idx, full=False):
    """the case of matrices idx of inp alone, each with right-hand sides of its own (a shared entry gets its source's); full: every entry also stores the
    G / alpha of what rides on it"""
    ents = [dict(inp["ents"][i], share=None) for i in idx]
    if full:
        ents = [dict(e, G=e["Lq"], alpha=e["qmu"]) for e in ents]
    return dict(batch=inp["batch"], ents=ents, M=inp["M"], Mp=inp["Mp"], A=inp["A"][list(idx)].copy(), Lq=[inp["Lq"][i] for i in idx], qmu=[inp["qmu"][i] for i in idx])


# ---- one call of the chain --------------------------------------------------------------------------------------------------------------------------
def n_slots(Mp):
    np_ = (Mp + 31) // 32
    return np_ * (np_ + 1) // 2


def written_slots(e, Mp):
    """mask [R + 1][ns] of the sums slots the chain writes for an entry: every slot of the rows r < R where Lq rides, the first np of row R where q_mu does"""
    mask = np.zeros((e["R"] + 1, n_slots(Mp)), bool)
    mask[:e["R"]] = bool(e["Lq"])
    mask[e["R"], :(Mp + 31) // 32] = bool(e["qmu"])
    return mask


def run(ctx, inp, alone=True, defer=False, may_ride=True, inverse=True, transpose=True, A_again=None, snapshot=False):
    """dcgp_debug_factor_chain on the inputs of build(): every output buffer and the sums filled with NaN before the call.  Returns a dict: info [batch]
    (with A_again [2][batch]), L, Linv, LinvT [batch][Mp][Mp] (None where not formed), and per entry G [R][Mp][Mp], alpha [Mp][Rp], sums [R + 1][ns] (None
    where the entry has none); with snapshot also "before": the same buffers as they were between run() and finish()."""
    from deepcgp_amd import device as dev
    ents, Mp, nb = inp["ents"], inp["Mp"], len(inp["ents"])
    nan = np.nan
    keep = []                                   # device arrays of the call

    def dev_arr(host):
        keep.append(ctx.to_device(host))
        return keep[-1]
    dA = dev_arr(inp["A"])
    dLinv = dev_arr(np.full((nb, Mp, Mp), nan)) if inverse else None
    dLinvT = dev_arr(np.full((nb, Mp, Mp), nan)) if inverse and transpose else None
    rides = any(carries(e) for e in ents)
    desc, dG, dal, dsums, dLq, dmu = [], [], [], [], [], []
    for i, e in enumerate(ents):
        src = e["share"]
        dLq.append(None if not e["Lq"] else dLq[src] if src is not None else dev_arr(inp["Lq"][i]))
        dmu.append(None if not e["qmu"] else dmu[src] if src is not None else dev_arr(inp["qmu"][i]))
        dG.append(dev_arr(np.full((e["R"], Mp, Mp), nan)) if e["G"] else None)
        dal.append(dev_arr(np.full((Mp, e["Rp"]), nan)) if e["alpha"] else None)
        dsums.append(dev_arr(np.full((e["R"] + 1, n_slots(Mp)), nan)) if carries(e) else None)
        desc += [e["R"], e["Rp"]] + [a.ptr if a is not None else 0 for a in (dLq[i], dmu[i], dG[i], dal[i], dsums[i])]
    outs = {"L": dA, "Linv": dLinv, "LinvT": dLinvT}
    per = {"G": dG, "alpha": dal, "sums": dsums}
    snap, copies = [], {}
    if snapshot:
        for name, a in list(outs.items()) + [("%s/%d" % (k, i), a) for k, v in per.items() for i, a in enumerate(v)]:
            if a is not None:
                copies[name] = dev_arr(np.full(a.shape, nan))
                snap += [copies[name].ptr, a.ptr, a.nbytes]
    da = (C.c_longlong * len(desc))(*desc) if rides else None
    sa = (C.c_longlong * len(snap))(*snap) if snap else None
    dAgain = dev_arr(A_again) if A_again is not None else None
    info = np.full((2 if A_again is not None else 1, nb), -99, np.int32)
    flags = int(bool(alone)) | int(bool(may_ride)) << 1 | int(bool(defer)) << 2
    ctx._check(dev.lib().dcgp_debug_factor_chain(ctx.handle, dA.ptr, dLinv.ptr if dLinv is not None else None, dLinvT.ptr if dLinvT is not None else None, nb, Mp,
                                                 da, len(desc) if rides else 0, flags, sa, len(snap), dAgain.ptr if dAgain is not None else None,
                                                 info.ctypes.data))
    res = {k: (a.numpy() if a is not None else None) for k, a in outs.items()}
    res.update({k: [a.numpy() if a is not None else None for a in v] for k, v in per.items()})
    res["info"] = info if A_again is not None else info[0]
    if snapshot:
        before = {k: (copies[k].numpy() if k in copies else None) for k in outs}
        before.update({k: [copies["%s/%d" % (k, i)].numpy() if "%s/%d" % (k, i) in copies else None for i in range(nb)] for k in per})
        res["before"] = before
    for a in keep:
        a.free()
    return res

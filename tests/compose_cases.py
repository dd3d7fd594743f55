"""Test helper: the covering table of feature combinations (tests/test_host_compose.py, tests/test_gpu_compose.py).

Five factors -- the stack, the likelihood, the conv layers' base kernel, their mean function, whitening -- and a small greedy generator that
picks cases until every pair of levels of two different factors occurs in one of them, except the pairs in ``EXCLUDED``, which the library
refuses by design (each with the text of its refusal).  Every case runs under both ``dedup_layer0`` settings; N = 3, S = 2, explicit noise, as
in tests/conv_mean_ref.py.  Test infrastructure only."""
import itertools
import random

import numpy as np

from deepcgp_amd import synthetic as syn
import conv_mean_ref as cmr
import live_specs as ls
import padding_ref as pr
import stack_specs as ss

N, S, SEED = 3, 2, 7

# stack -> stack_specs.stack_spec arguments: convs [(f, s, R, pad, dil)], head (f, s, pad), one M per layer
#   ch_res, valid2, even_s2, wide_R   conv_mean_ref.CASES
#   small3_20_40_24, ch_72_264         the geometry and the Ms of that live_specs.CASES_MIXED entry (Mp 32 / 48 / 32; the head at M > 256)
#   ch_264_72                          padding_ref.STACKS: the conv layer at M = 264 (sweep + GEMM route), padded by 2
#   narrow_R1                          8 x 8 x 1, f3 s1 R1, M = 4: a conv layer of width 1 takes the R < 2 branches of csrc/fused_plan.h
_KEYS = ("hwc", "convs", "head", "Ms")


def _unpadded(k):
    return dict(hwc=k["hwc"], convs=[c + (0, 1) for c in k["convs"]], head=k["head"] + (0,), Ms=k["Ms"])


STACKS = {
    "ch_res": {k: cmr.CASES["ch_res"][k] for k in _KEYS},
    "valid2": {k: cmr.CASES["valid2"][k] for k in _KEYS},
    "even_s2": {k: cmr.CASES["even_s2"][k] for k in _KEYS},
    "wide_R": {k: cmr.CASES["wide_R"][k] for k in _KEYS},
    "small3_20_40_24": _unpadded(ls.CASES_MIXED["small3_20_40_24"]),
    "ch_264_72": {k: pr.STACKS["ch_264_72"][k] for k in _KEYS},
    "ch_72_264": _unpadded(ls.CASES_MIXED["ch_72_264"]),
    "narrow_R1": dict(hwc=(8, 8, 1), convs=[(3, 1, 1, 0, 1)], head=(3, 1, 0), Ms=4),
}

# likelihood -> (compose_ref tuple, head width D)
LIKELIHOODS = {
    "multiclass3": (("robustmax", 3), 3),
    "softmax3": (("softmax", 3, 100, 3), 3),
    "gaussian3": (("gaussian", 0.7), 3),
    "gaussian1": (("gaussian", 0.7), 1),
    "bernoulli1": (("bernoulli",), 1),
    "studentt3": (("studentt", 0.7, 4.5), 3),
    "poisson1": (("poisson", 2.5), 1),
}
# live_specs' lengthscale constant c (lengthscale = c * rms |Z_i|), 1 unless named: behind a random mean filter and whitened layers the samples
# that reach small3's second layer and head lie outside c = 1's lengthscale and three gradient groups fall under LIVE_MAX (1.0e-4, 8.7e-5,
# 1.8e-5 against 1e-3); at c = 2 every group of every case of that stack is live (tests/test_host_compose.py)
LENGTHSCALE_C = {"small3_20_40_24": 2.0}
ACOS = (1.7, 0.8, 0.5)            # (variance, weight_variances, bias_variance): none of them gpflow's default 1

FACTORS = {
    "stack": list(STACKS),
    "likelihood": list(LIKELIHOODS),
    "base": ["rbf", "matern32", "matern52", "acos"],
    "mean": ["none", "conv2d", "filter"],            # no mean function, Conv2dMean, a trainable random LinearConv2dMean filter
    "white": ["none", "all", "alternate"],          # alternate: layers 0, 2, ... whitened
}
NAMES = list(FACTORS)

# Pairs the library refuses by design: ((factor, level), (factor, level), the text of the refusal).  Conv2dMean copies a patch's centre pixel;
# dcgp_model_add_conv_layer refuses it on a layer with an even filter (even_s2: f4; small3_20_40_24: its second conv layer is f4).  The
# refusal comes from the device model's first call, so tests/test_gpu_compose.py asserts it.
EXCLUDED = [
    (("stack", "even_s2"), ("mean", "conv2d"), "Conv2dMean supports odd filter sizes only"),
    (("stack", "small3_20_40_24"), ("mean", "conv2d"), "Conv2dMean supports odd filter sizes only"),
]


def _pairs(case):
    items = [(f, case[f]) for f in NAMES]
    return set(itertools.combinations(items, 2))


def excluded_pairs():
    return {(a, b) for a, b, _ in EXCLUDED}


def all_pairs():
    """Every pair of levels of two different factors, as ((factor, level), (factor, level)) in FACTORS' order."""
    out = set()
    for fa, fb in itertools.combinations(NAMES, 2):
        out |= {((fa, a), (fb, b)) for a in FACTORS[fa] for b in FACTORS[fb]}
    return out


def generate(seed=0):
    """Greedy pairwise cover: of all combinations that hold no excluded pair, take the one that covers the most pairs not yet covered (ties:
    a seeded draw), until none is left.  Deterministic: plain Python, ``random.Random(seed)``."""
    rng = random.Random(seed)
    banned = excluded_pairs()
    todo = all_pairs() - banned
    pool = [dict(zip(NAMES, combo)) for combo in itertools.product(*FACTORS.values())]
    pool = [(c, _pairs(c)) for c in pool]
    pool = [(c, p) for c, p in pool if not (p & banned)]
    cases = []
    while todo:
        gains = [len(p & todo) for _, p in pool]
        best = max(gains)
        assert best > 0, sorted(todo)
        c, p = pool[rng.choice([i for i, g in enumerate(gains) if g == best])]
        cases.append(c)
        todo -= p
    return cases


CASES = generate()


def case_id(case):
    return "-".join(case[f] for f in NAMES)


IDS = [case_id(c) for c in CASES]
BY_ID = dict(zip(IDS, CASES))


def whites(case, layers):
    return {"none": [False] * layers, "all": [True] * layers, "alternate": [i % 2 == 0 for i in range(layers)]}[case["white"]]


def targets(lik, D, Ylab, seed=SEED):
    """Targets of a likelihood for the images whose labels are Ylab: labels mod 3; standard normal floats (StudentT: one entry at 3.0);
    {0, 1} with both values present; small counts with a zero among them."""
    n = len(Ylab)
    rng = np.random.default_rng(300 + seed)
    kind = lik[0]
    if kind in ("robustmax", "softmax"):
        return (np.asarray(Ylab) % D).astype(np.int32)
    if kind in ("gaussian", "studentt"):
        Y = rng.standard_normal((n, D))
        if kind == "studentt":
            Y[n // 2, D // 2] = 3.0
        return Y
    if kind == "bernoulli":
        Y = (rng.random((n, D)) < 0.5).astype(np.float64)
        Y[0], Y[-1] = 1.0, 0.0
        return Y
    Y = rng.poisson(2.5, (n, D)).astype(np.float64)
    Y[0, 0] = 0.0
    return Y


def make_spec(case, trainable=True):
    """(spec, likelihood tuple) of a case: stack_specs.stack_spec (live_specs' recipe, c = LENGTHSCALE_C, a = 0.1) with the head cut to the likelihood's
    width, the base kernel and the mean put on every conv layer as tests/conv_mean_ref.py::make_case does."""
    k = STACKS[case["stack"]]
    lik, D = LIKELIHOODS[case["likelihood"]]
    nl = len(k["convs"]) + 1
    spec = ss.stack_spec(whites=whites(case, nl), S=S, seed=SEED, c=LENGTHSCALE_C.get(case["stack"], 1.0), **k)
    h = spec["head"]
    h["R"], h["q_mu"], h["q_sqrt"] = D, np.array(h["q_mu"][:, :D]), np.array(h["q_sqrt"][:D])
    for c in spec["convs"]:
        if case["base"] != "rbf":
            c["base"] = case["base"]
        if case["base"] == "acos":
            c["acos"], c["variance"] = ACOS, ACOS[0]
        if case["mean"] == "conv2d":
            c["mean_function"] = "conv2d"
    if case["mean"] == "filter":
        cmr.add_filters(spec, "random", trainable=trainable, seed=SEED)
    return spec, lik


def make_case(case, n=N, seed=SEED):
    """(spec, X, Y, zs, likelihood tuple) of a case; ``n`` images."""
    spec, lik = make_spec(case)
    X, Ylab = syn.make_batch(STACKS[case["stack"]]["hwc"], n, seed=seed)
    return spec, X, targets(lik, spec["head"]["R"], Ylab, seed), ss.make_noise(spec, n, seed=seed), lik

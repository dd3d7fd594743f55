"""Test helper: model specs whose EVERY gradient group is live (CASES: M > 256, CASES_M256: M <= 256 and the model variants), and the measures
the entry-wise gradient tests share.

``syn.make_config`` is right for timing and for the forward, but its deep specs are degenerate for gradients: the inducing patches of a deeper
layer are cut from images pushed through the identity convolution, which SUMS the input channels (10 equal maps: values 10 x the image, 30 x at
the CIFAR head), while the data that reaches that layer is mean + noise of order one.  With one lengthscale of 5 everywhere K_uf underflows and
nothing flows back (|dZ|max 1e-30 for both conv layers of cfg3 / cfg4).  ``live_spec`` keeps ``make_spec``'s geometry, seeds and inducing
patches and edits the dicts:

* per-layer lengthscale  c * rms_i |Z_i|  (the root-mean-square norm of that layer's own inducing patches: c * sqrt(patch length) for
  patches of unit-variance pixels, 10 x / 30 x that where the identity convolution has scaled them);
* q_mu scaled by ``a``; conv q_sqrt = 0.3 * chol(K_uu) at the NEW lengthscale (identity when whitened), the head's chol(K_uu);
* head patch weights 0.5 + U(0, 1).

``mixed_live_spec`` builds the heterogeneous stacks of CASES_MIXED from it: one M and one white flag per layer.

Used by tests/test_host_grad_large_m.py, tests/test_host_grad_m256.py and tests/test_host_mixed_layers.py (liveness of the torch reference,
no GPU) and by tests/test_gpu_grad_large_m.py, tests/test_gpu_grad_m256.py and tests/test_gpu_mixed_layers.py."""
import numpy as np

from deepcgp_amd import synthetic as syn

LIVE_MAX = 1e-3          # every group: |want|max >= LIVE_MAX
LIVE_MEDIAN = 1e-6       # Z, q_mu, patch_weights: median |want| >= LIVE_MEDIAN * |want|max
ENTRY_FLOOR = 1e-6       # entry-wise measure: over the entries with |want| >= ENTRY_FLOOR * |want|max
LEFT_OUT_CAP = 0.5       # ... which may leave out at most this share of Z, q_mu, patch_weights and tril(q_sqrt)
MEDIAN_GROUPS = ("Z", "q_mu", "patch_weights")
CAPPED_GROUPS = MEDIAN_GROUPS + ("q_sqrt",)

# name -> geometry, M, images, and the two constants of live_spec.  S = 2 and seed 7 everywhere.
CASES = {
    "ch_M1024": dict(hwc=(28, 28, 1), convs=[(5, 2, 10)], head=(5, 1), M=1024, N=4, c=0.7, a=0.1),
    "ch_M1000": dict(hwc=(28, 28, 1), convs=[(5, 2, 10)], head=(5, 1), M=1000, N=3, c=0.7, a=0.1),
    "h_M1024": dict(hwc=(28, 28, 1), convs=[], head=(5, 1), M=1024, N=4, c=0.5, a=0.3),
    "cifar3_M384": dict(hwc=(32, 32, 3), convs=[(4, 2, 10), (5, 1, 10)], head=(5, 1), M=384, N=2, c=1.0, a=0.1),
    "mnist3_M320": dict(hwc=(28, 28, 1), convs=[(4, 2, 10), (5, 1, 10)], head=(5, 1), M=320, N=3, c=1.0, a=0.1),
    "ch_white_M384": dict(hwc=(28, 28, 1), convs=[(5, 2, 10)], head=(5, 1), M=384, N=4, c=1.0, a=0.1, white=True),
    "ch_M384": dict(hwc=(28, 28, 1), convs=[(5, 2, 10)], head=(5, 1), M=384, N=4, c=1.0, a=0.1),
}

# The M <= 256 route (tests/test_host_grad_m256.py, tests/test_gpu_grad_m256.py).  Kept apart: the large-M host test asserts M > 256 on every
# entry of CASES.  S = 2 unless a case says otherwise: the two ch cases run S = 4, 15 x 4 x 144 = 8640 columns in the conv layer, past the 4096
# of the strip kernel and the 8192 of syrk_kscale_kernel.  The last three are the model variants (`head_kernel`, `additive`, `conv2d_mean`).
_MNIST, _MNIST3, _SMALL3 = dict(hwc=(28, 28, 1), head=(5, 1)), [(4, 2, 10), (5, 1, 10)], [(3, 1, 3), (4, 2, 2)]
CASES_M256 = {
    "ch_M256": dict(_MNIST, convs=[(5, 2, 10)], M=256, N=15, c=1.0, a=0.1, S=4),
    "ch_M200": dict(_MNIST, convs=[(5, 2, 10)], M=200, N=15, c=1.0, a=0.1, S=4),
    "ch_white_M256": dict(_MNIST, convs=[(5, 2, 10)], M=256, N=15, c=1.0, a=0.1, white=True),
    "h_M256": dict(_MNIST, convs=[], M=256, N=8, c=0.5, a=0.3),
    "mnist3_M256": dict(_MNIST, convs=_MNIST3, M=256, N=3, c=1.0, a=0.1),
    "mnist3_M72": dict(_MNIST, convs=_MNIST3, M=72, N=3, c=1.0, a=0.1),
    "small3_M20": dict(hwc=(14, 14, 1), convs=_SMALL3, head=(3, 1), M=20, N=3, c=1.0, a=0.1),
    "small3_white_M20": dict(hwc=(14, 14, 1), convs=_SMALL3, head=(3, 1), M=20, N=3, c=1.0, a=0.1, white=True),
    "small3_M12": dict(hwc=(12, 12, 1), convs=_SMALL3, head=(3, 1), M=12, N=4, c=1.0, a=0.1),     # M <= 16: one row chunk in the K_uf adjoint
    "odd_M33": dict(hwc=(13, 13, 2), convs=[(4, 3, 13)], head=(2, 1), M=33, N=5, c=1.0, a=0.1),
    "additive_M24": dict(hwc=(12, 12, 1), convs=[(3, 1, 3)], head=(3, 1), M=24, N=3, c=1.0, a=0.1, additive=True),
    "dense_ard_M24": dict(hwc=(12, 12, 1), convs=[(3, 1, 3)], head=(3, 1), M=24, N=3, c=1.0, a=0.1, head_kernel="rbf"),
    "conv2d_mean_M24": dict(hwc=(12, 12, 1), convs=[(3, 1, 3)], head=(3, 1), M=24, N=3, c=1.0, a=0.1, conv2d_mean=True),
}


def live_spec(hwc, convs, head, M, c, a, S=2, seed=7, white=False, num_data=60000, conv_q_sqrt_scale=0.3, head_kernel="conv", additive=False,
              conv2d_mean=False):
    """``head_kernel="rbf"``: the dense RBF(ARD) head, its lengthscales make_spec's 0.8 - 1.2 spread around c * rms_i |Z_i|; ``additive``: the
    AdditivePatchKernel head; ``conv2d_mean``: Conv2dMean on every conv layer (odd filters)."""
    spec = syn.make_spec(hwc, convs, head, M, S=S, num_data=num_data, seed=seed, white=white, conv_q_sqrt_scale=conv_q_sqrt_scale,
                         head_kernel=head_kernel)
    rng = np.random.default_rng(seed)
    layers = spec["convs"] + [spec["head"]]
    for li, l in enumerate(layers):
        Z = np.asarray(l["Z"], np.float64)
        ls_old = l["ls"]
        l["ls"] = float(c * np.sqrt(np.mean(np.sum(Z * Z, 1))))
        l["q_mu"] = a * np.asarray(l["q_mu"], np.float64)
        if "ls_ard" in l:
            l["ls_ard"] = np.asarray(l["ls_ard"], np.float64) * (l["ls"] / ls_old)
        if not white:
            Ku = syn._rbf(Z / l["ls_ard"], Z / l["ls_ard"], l["variance"], 1.0) if "ls_ard" in l else syn._rbf(Z, Z, l["variance"], l["ls"])
            Lu = np.linalg.cholesky(Ku + syn.JITTER * np.eye(M))
            l["q_sqrt"] = np.tile(Lu[None], [l["R"], 1, 1]) * (1.0 if l is spec["head"] else conv_q_sqrt_scale)
    if head_kernel != "rbf":
        spec["head"]["w"] = 0.5 + rng.random(spec["head"]["w"].shape)
    if additive:
        spec["head"]["kernel"] = "add"
    if conv2d_mean:
        for l in spec["convs"]:
            l["mean_function"] = "conv2d"
    return spec


def mixed_live_spec(hwc, convs, head, Ms, c, a, whites=None, **kw):
    """A live spec whose layers differ in M (``Ms``: one count per layer, the head last, as the reference's ``-M 384,64``) and in whitening
    (``whites``: one flag per layer, default all False): ``live_spec`` once per layer with that layer's M and white, layer i kept from call i.
    A layer's inducing patches are cut from images that depend on the geometry and the seed alone, and its lengthscale edit and q_sqrt on its
    own Z: nothing in layer i of call i depends on the M another layer would have had.  ``kw`` goes to ``live_spec`` (S, seed, ...)."""
    nl = len(convs) + 1
    whites = [False] * nl if whites is None else list(whites)
    assert len(Ms) == nl and len(whites) == nl, (Ms, whites, nl)
    each = [live_spec(hwc, convs, head, M, c, a, white=w, **kw) for M, w in zip(Ms, whites)]
    return {"S": each[0]["S"], "num_data": each[0]["num_data"], "convs": [each[i]["convs"][i] for i in range(nl - 1)], "head": each[-1]["head"]}


# Heterogeneous stacks (tests/test_host_mixed_layers.py, tests/test_gpu_mixed_layers.py): one M per layer, Mp = round_up(M, 16) in brackets, one
# white flag per layer where given.  S = 2, seed 7, N = 3.  The library keeps one factor group per distinct Mp (csrc/model.hip, build_groups).
_CH = dict(hwc=(28, 28, 1), convs=[(5, 2, 10)], head=(5, 1))
_SMALL = dict(hwc=(14, 14, 1), convs=_SMALL3, head=(3, 1))
CASES_MIXED = {
    # two groups (32: layers 0 and 2 with layer 0's prior, 48: layer 1 and its prior); no deferred factor copy, the in-tail KL reads K / Kp
    "small3_20_40_24": dict(_SMALL, Ms=(20, 40, 24), N=3, c=1.0, a=0.1),                                         # Mp 32, 48, 32
    # group 32 holds a riding matrix pair (layer 1) and a whitened head that does not ride; a whitened layer moves the KL out of the tail launch
    "small3_mixwhite": dict(_SMALL, Ms=(40, 20, 24), N=3, c=1.0, a=0.1, whites=(True, False, True)),             # Mp 48, 32, 32
    # one group, the deferred copy on, three different true M inside it
    "small3_sameMp": dict(_SMALL, Ms=(20, 24, 30), N=3, c=1.0, a=0.1),                                           # Mp 32, 32, 32
    # the conv layer on the M > 256 route, the head on the M <= 256 route, and the reverse
    "ch_264_72": dict(_CH, Ms=(264, 72), N=3, c=1.0, a=0.1),                                                     # Mp 272, 80
    "ch_72_264": dict(_CH, Ms=(72, 264), N=3, c=1.0, a=0.1),                                                     # Mp 80, 272
    # 33 feature maps, Rp = 48: the widest conv layer of the suite (13 elsewhere), beside a head with Rp = 16 in the same group.  Its right-hand sides
    # cannot ride (Rp > 32) -- and nor do the head's here: a conv layer with Rp != 16 is not one launch (fused_plan.h, plan_layer_launch), and a chain beside
    # a first layer's sweep carries no right-hand sides at all (plan_step: may_ride).  Mixed riding in one group is small3_mixwhite's
    "wide_R33": dict(hwc=(12, 12, 1), convs=[(3, 1, 33)], head=(3, 1), Ms=(24, 24), N=3, c=1.0, a=0.1),          # Mp 32, 32
}


# What each CASES_MIXED entry is claimed to reach.  Per layer (the head last): Mp, whether the layer takes the M > 256 route, white, Rp =
# round_up(R, 16).  `groups`: the factor groups in the order build_groups makes them, (Mp, matrices, riding): an unwhitened conv layer brings
# Kuu(Z) and the prior's Kuu(Z0), a whitened conv layer and the head one matrix each; `riding` = how many of them carry G / alpha (the prior:
# the KL's sums) on the chain in an ELBO step -- the layer unwhitened, Mp <= 256 and Rp <= 32, and only where the chain may carry any: a first layer
# that is one launch behind the chain (a conv layer with Mp <= 256 and R <= 16), not one that opens with a sweep beside it.  None: not claimed.
EXPECT_MIXED = {
    "small3_20_40_24": dict(Mp=(32, 48, 32), large=(False, False, False), white=(False, False, False), Rp=(16, 16, 16),
                            groups=[(32, 3, 3), (48, 2, 2)]),
    "small3_mixwhite": dict(Mp=(48, 32, 32), large=(False, False, False), white=(True, False, True), Rp=(16, 16, 16),
                            groups=[(48, 1, 0), (32, 3, 2)]),
    "small3_sameMp": dict(Mp=(32, 32, 32), large=(False, False, False), white=(False, False, False), Rp=(16, 16, 16), groups=[(32, 5, 5)]),
    "ch_264_72": dict(Mp=(272, 80), large=(True, False), white=(False, False), Rp=(16, 16), groups=[(272, 2, None), (80, 1, None)]),
    "ch_72_264": dict(Mp=(80, 272), large=(False, True), white=(False, False), Rp=(16, 16), groups=[(80, 2, None), (272, 1, 0)]),
    "wide_R33": dict(Mp=(32, 32), large=(False, False), white=(False, False), Rp=(48, 16), groups=[(32, 3, 0)]),
}


def round_up(n, k):
    return (n + k - 1) // k * k


def host_groups(spec):
    """[(Mp, matrices, riding)] of a spec as build_groups makes them: layers in order, a group per distinct Mp in order of first appearance;
    riding as EXPECT_MIXED defines it (never None; conv-first specs)."""
    groups = []
    layers = spec["convs"] + [spec["head"]]
    may_ride = bool(spec["convs"]) and round_up(layers[0]["M"], 16) <= 256 and layers[0]["R"] <= 16       # the first layer is one launch
    for li, l in enumerate(layers):
        n = 2 if (li < len(layers) - 1 and not l["white"]) else 1
        Mp = round_up(l["M"], 16)
        ride = n if (may_ride and not l["white"] and Mp <= 256 and round_up(l["R"], 16) <= 32) else 0
        at = [i for i, g in enumerate(groups) if g[0] == Mp]
        if at:
            groups[at[0]] = (Mp, groups[at[0]][1] + n, groups[at[0]][2] + ride)
        else:
            groups.append((Mp, n, ride))
    return groups


def make_case(name):
    """(spec, X, Y, zs) of CASES[name], CASES_M256[name] or CASES_MIXED[name]."""
    if name in CASES_MIXED:
        k = dict(CASES_MIXED[name])
        N = k.pop("N")
        spec = mixed_live_spec(**k)
        X, Y = syn.make_batch(k["hwc"], N, seed=7)
        return spec, X, Y, syn.make_noise(spec, N, seed=7)
    k = dict(CASES[name] if name in CASES else CASES_M256[name])
    N = k.pop("N")
    spec = live_spec(**k)
    X, Y = syn.make_batch(k["hwc"], N, seed=7)
    return spec, X, Y, syn.make_noise(spec, N, seed=7)


def torch_reference(spec, X, Y, zs):
    """(ELBO, [per-layer {group: gradient}]) by torch autograd of tests/test_oracle_autograd.py's forward, float64 on the CPU; q_sqrt's
    gradient is cut to the lower triangle (the parameter)."""
    import torch
    from test_oracle_autograd import _torch_elbo
    e_t, leaves = _torch_elbo(spec, X, Y, zs)
    flat = [(li, k, t) for li, p in enumerate(leaves) for k, t in p.items()]
    tg = torch.autograd.grad(e_t, [t for _, _, t in flat])
    want = [{} for _ in leaves]
    for (li, k, _), g in zip(flat, tg):
        want[li][k] = np.tril(g.numpy()) if k == "q_sqrt" else g.numpy().copy()
    return e_t.item(), want


SPEC_KEY = {"Z": "Z", "q_mu": "q_mu", "q_sqrt": "q_sqrt", "variance": "variance", "lengthscales": "ls", "patch_weights": "w",
            "weight_variances": "weight_variances", "bias_variance": "bias_variance"}      # (the last two: tests/acos_ref.py's flattened specs)
POSITIVE = ("variance", "lengthscales", "weight_variances", "bias_variance")      # softplus + 1e-6 in gpflow's unconstrained space


def softplus_inv(x):
    return np.log(np.expm1(x - 1e-6))


def adam_numpy_step(spec, grads, state, lr, t, b1=0.9, b2=0.999, eps=1e-8):
    """tf.train.AdamOptimizer's update (ascent on the ELBO) of every value of `spec` in place, from `grads` as torch_reference returns them;
    `state` {(layer, group): [m, v]} is filled on the first call.  The scheme of test_adam_steps_match_numpy_on_oracle_gradients."""
    lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    for li, l in enumerate(spec["convs"] + [spec["head"]]):
        for name, g in grads[li].items():
            x = np.array(l[SPEC_KEY[name]], np.float64)
            g = -np.asarray(g, np.float64)
            u = softplus_inv(x) if name in POSITIVE else x
            if name in POSITIVE:
                g = g * (1.0 - np.exp(-(x - 1e-6)))
            m, v = state.setdefault((li, name), [np.zeros_like(x), np.zeros_like(x)])
            m[...] = b1 * m + (1 - b1) * g
            v[...] = b2 * v + (1 - b2) * g * g
            u = u - lr_t * m / (np.sqrt(v) + eps)
            new = np.log1p(np.exp(u)) + 1e-6 if name in POSITIVE else u
            l[SPEC_KEY[name]] = float(new) if np.ndim(new) == 0 else new


def model_values(model):
    """[per-layer {group: value}] of a device model's Python-side parameters (after pull_parameters), under the gradient's names."""
    out = []
    for li, l in enumerate(model.layers):
        head = li == len(model.layers) - 1
        kern = l.kern.base_kernel if head else l.base_kernel
        d = dict(Z=np.array(l.feature.Z), q_mu=np.array(l.q_mu), q_sqrt=np.array(l.q_sqrt), variance=float(kern.variance))
        if hasattr(kern, "lengthscales"):
            d["lengthscales"] = float(kern.lengthscales)
        else:                                             # ArcCosine(order 0)
            d["weight_variances"], d["bias_variance"] = float(kern.weight_variances), float(kern.bias_variance)
        if head:
            d["patch_weights"] = np.array(l.kern.patch_weights)
        out.append(d)
    return out


def _entries(name, g):
    """The entries of a group that are parameters: the lower triangle of every q_sqrt[r], everything otherwise."""
    g = np.asarray(g, np.float64)
    if name == "q_sqrt":
        return g[:, np.tril(np.ones(g.shape[1:], bool))]
    return g.reshape(-1)


def liveness(want):
    """[(layer, group, |want|max, median |want| / |want|max, share of entries below ENTRY_FLOOR * |want|max)] of a reference gradient."""
    rows = []
    for li, groups in enumerate(want):
        for name, g in groups.items():
            v = np.abs(_entries(name, g))
            top = float(v.max())
            rows.append((li, name, top, float(np.median(v)) / top if top > 0 else 0.0, float(np.mean(v < ENTRY_FLOOR * top))))
    return rows


def assert_live(case, want):
    """The liveness condition of a case, on the reference alone."""
    for li, name, top, med, left_out in liveness(want):
        assert top >= LIVE_MAX, (case, li, name, "max", top)
        if name in MEDIAN_GROUPS:
            assert med >= LIVE_MEDIAN, (case, li, name, "median / max", med)
        if name in CAPPED_GROUPS:
            assert left_out <= LEFT_OUT_CAP, (case, li, name, "share below the entry floor", left_out)


def errors(name, got, want):
    """(group-wise |got - want|max / |want|max, entry-wise max |got - want| / |want| over the entries at or above the floor)."""
    g, w = _entries(name, got), _entries(name, want)
    top = np.abs(w).max()
    keep = np.abs(w) >= ENTRY_FLOOR * top
    d = np.abs(g - w)
    return float(d.max() / top), float((d[keep] / np.abs(w[keep])).max())

"""No GPU: the covering table of tests/compose_cases.py and the composed torch reference of tests/compose_ref.py, before anything runs on a device.

* the table covers every pair of levels of two different factors, or names the pair in ``EXCLUDED``, in at most 60 cases;
* under RobustMax the composed reference is tests/torch_ref.py's forward with its own tail (tests/test_host_torch_ref.py pins that forward to
  the per-feature copies it replaced);
* each likelihood rule on the plain stack agrees with the reference its own test file uses, to 1e-12 relative: float64 restatements of one
  formula.  Seen on the CPU: quad_ref.torch_elbo 0 (StudentT), 0 (Poisson); _torch_softmax_elbo 0; _torch_gauss 0; bernoulli_ref.elbo 4.4e-16
  (the NumPy oracle's forward under a SciPy tail: the only one that is not the same torch operations in the same order);
* the reference gradient of every case is live by tests/live_specs.py's measures (LIVE_MAX, LIVE_MEDIAN, LEFT_OUT_CAP), and where a case
  has a mean function, taking it off moves the input gradient by more than 1e-3 of its maximum (smallest seen: 1.6e-1,
  wide_R-studentt3-matern32-filter-none)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import compose_cases as cc          # noqa: E402
import compose_ref as cr            # noqa: E402
import conv_mean_ref as cmr         # noqa: E402
import live_specs as ls             # noqa: E402

RULE_RTOL = 1e-12


# ---- 1. the table -------------------------------------------------------------------------------------------------------------------
def test_every_pair_is_covered_or_excluded():
    covered = set()
    for case in cc.CASES:
        assert set(case) == set(cc.NAMES) and all(case[f] in cc.FACTORS[f] for f in cc.NAMES), case
        covered |= cc._pairs(case)
    missing = cc.all_pairs() - covered
    print("%d cases, %d pairs, %d covered, %d excluded" % (len(cc.CASES), len(cc.all_pairs()), len(covered), len(missing)))
    assert len(cc.CASES) <= 60
    assert len(set(cc.IDS)) == len(cc.IDS)
    assert missing == cc.excluded_pairs(), sorted(missing ^ cc.excluded_pairs())      # no pair dropped silently, none excluded that is covered
    assert cc.generate() == cc.CASES                                                  # the generator is deterministic


def test_excluded_pairs_are_the_ones_the_library_refuses():
    """Both refusals come from dcgp_model_add_conv_layer (``Conv2dMean supports odd filter sizes only``), a device call: the raise itself is
    asserted in tests/test_gpu_compose.py (building the layers already factors K_uu on the device, so no call without a GPU can know).
    Here: each excluded stack does hold a conv layer with an even filter, and no other stack does -- so no other (stack, conv2d) pair
    belongs in the list -- and the spec of such a case does ask for Conv2dMean on that layer."""
    even = {name for name, k in cc.STACKS.items() if any(f % 2 == 0 for f, *_ in k["convs"])}
    assert even == {a[1] for a, b, _ in cc.EXCLUDED} and all(b == ("mean", "conv2d") for _, b, _ in cc.EXCLUDED)
    for (_, stack), _, text in cc.EXCLUDED:
        assert text == "Conv2dMean supports odd filter sizes only"
        spec, _ = cc.make_spec(dict(stack=stack, likelihood="multiclass3", base="rbf", mean="conv2d", white="none"))
        assert any(c["f"] % 2 == 0 and c["mean_function"] == "conv2d" for c in spec["convs"])


# ---- 2. the likelihood rules on the plain stack -----------------------------------------------------------------------------------------
def _leaf_grads(e, leaves, extra=()):
    flat = [t for p in leaves for t in p.values()] + [t for t in extra if t is not None]
    return [g.numpy() for g in torch.autograd.grad(e, flat)]


def _agree(tag, got, want):
    err = abs(got - want) / abs(want)
    print("%s: composed %.15e reference %.15e rel %.3e" % (tag, got, want, err))
    assert err <= RULE_RTOL, (tag, err)


@pytest.mark.parametrize("lik", [("studentt", 0.7, 4.5), ("poisson", 2.5)], ids=["studentt", "poisson"])
def test_quadrature_rules_match_quad_ref(lik):
    import quad_ref as qr
    import test_gpu_quadrature as tq
    spec, X, Ylab, Y, zs = tq.make_case(lik, "conv", 3, N=3, S=2, seed=11)
    e, leaves, scale = qr.torch_elbo(lik, spec, X, Ylab, Y, zs)
    parts, want, dlik = cr.torch_reference(spec, X, Y, zs, lik)
    _agree(lik[0], parts[0], e.item())
    ref = _leaf_grads(e, leaves, (scale,))
    got = [want[li][k] for li, p in enumerate(leaves) for k in p] + ([dlik] if scale is not None else [])
    for g, w in zip(got, ref):
        w = np.tril(w) if w.ndim == 3 else w
        assert np.abs(g - w).max() <= RULE_RTOL * max(1.0, np.abs(w).max())      # (the same torch operations: the gradients agree as the values do)


def test_softmax_rule_matches_its_test_files_reference():
    import test_gpu_softmax as tsm
    lik = ("softmax", 3, 100, 3)
    spec, X, Y, zs = tsm.make_case("conv", 3, N=3, S=2, seed=11)
    e, _ = tsm._torch_softmax_elbo(spec, X, Y, zs, cr.softmax_nodes(lik))
    _agree("softmax", cr.torch_reference(spec, X, Y, zs, lik)[0][0], e.item())


def test_gaussian_rule_matches_its_test_files_reference():
    import test_gpu_gaussian as tg
    spec, X, Ylab, Y, zs = tg.make_case("conv", 3, N=3, S=2, seed=11)
    e, leaves, s2t = tg._torch_gauss(spec, X, Ylab, Y, zs, 0.6)
    parts, _, dlik = cr.torch_reference(spec, X, Y, zs, ("gaussian", 0.6))
    _agree("gaussian", parts[0], e.item())
    (ds2,) = torch.autograd.grad(e, [s2t])
    _agree("gaussian d / d variance", float(dlik), ds2.item())


@pytest.mark.parametrize("D,white", [(1, False), (3, True)])
def test_bernoulli_rule_matches_bernoulli_ref(D, white):
    import bernoulli_ref as br
    import test_gpu_bernoulli as tb
    spec, X, Ylab, Y, zs = tb.make_case("conv", D, white, N=3, S=2, seed=11)
    want = br.elbo(spec, X, Ylab, Y, zs)
    parts, _, _ = cr.torch_reference(spec, X, Y, zs, ("bernoulli",))
    for what, g, w in zip(("elbo", "data", "kl"), parts, want):
        _agree("bernoulli D=%d %s" % (D, what), g, w)


# ---- 3. liveness of every case ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(cid):
    spec, X, Y, zs, lik = cc.make_case(cc.BY_ID[cid])
    return cr.reference(spec, X, Y, zs, lik)


@pytest.mark.parametrize("cid", cc.IDS)
def test_reference_gradient_is_live(cid):
    ref = reference(cid)
    assert all(np.isfinite(p) for p in ref["parts"])
    case = cc.BY_ID[cid]
    n_conv = len(cc.STACKS[case["stack"]]["convs"])
    assert all(("mean_filter" in g) == (case["mean"] == "filter") for g in ref["want"][:n_conv]) and "mean_filter" not in ref["want"][-1]
    lik = cc.LIKELIHOODS[case["likelihood"]][0]
    assert (cr.LIK_PARAM.get(lik[0]) in ref["want"][-1]) == (lik[0] in cr.LIK_PARAM)
    ls.assert_live(cid, ref["want"])
    assert np.abs(ref["dX"]).max() > 0 and np.all(np.isfinite(ref["dX"]))


@pytest.mark.parametrize("cid", [i for i in cc.IDS if cc.BY_ID[i]["mean"] != "none"])
def test_the_mean_function_is_live_in_the_input_gradient(cid):
    """The measure of tests/test_gpu_conv_mean.py: without its mean functions the case's input gradient moves by more than 1e-3 |dX|max, so a
    device that dropped the mean's term (Conv2dMean has no gradient group that could show it) cannot meet the input gradient's bound."""
    spec, X, Y, zs, lik = cc.make_case(cc.BY_ID[cid])
    plain = cmr.without_filters(spec)
    for c in plain["convs"]:
        c.pop("mean_function", None)
    _, without = cr.torch_input_gradient(plain, X, Y, zs, lik)
    want = reference(cid)["dX"]
    share = np.abs(want - without).max() / np.abs(want).max()
    print("%s: the mean's share of dX %.3e" % (cid, share))
    assert share > 1e-3

"""The heterogeneous stacks of tests/live_specs.py (CASES_MIXED: layers that differ in M, whitening and width), on the CPU: what each case is
claimed to reach, the liveness of its torch reference gradient, and the two CPU references against each other.

tests/test_gpu_mixed_layers.py runs the device on these cases.  The library keeps one factor group per distinct padded size
Mp = round_up(M, 16) (csrc/model.hip, build_groups), lets a layer's right-hand sides ride the factorisation chain only where it is unwhitened,
Mp <= 256 and Rp = round_up(R, 16) <= 32, and sends each layer down the M <= 256 or the M > 256 route on its own; live_specs.EXPECT_MIXED
writes out, per case, the per-layer Mp / route / white flag / Rp and the groups that follow from them, so that a later edit of the table
cannot fold a case back into one group unnoticed.

The reference's figures, smallest over the layers of a case (group maximum | median / max of Z, q_mu, patch_weights | largest share of
tril(q_sqrt) below the entry floor), and the oracle's ELBO against the torch forward.  S = 2, seed 7, N = 3, c = 1.0, a = 0.1 everywhere (the
two cases nobody had run before this module, small3_sameMp and wide_R33, are live at the same constants):

    case              Ms           min group max              min median / max    q_sqrt below floor   ELBO (torch)      oracle vs torch
    small3_20_40_24   20, 40, 24   6.9e-01 (L0 variance)      2.4e-02 (L1 Z)      0.001 (L1)           -493210.094001    3.5e-16
    small3_mixwhite   40, 20, 24   2.3e-01 (L2 variance)      2.4e-02 (L1 Z)      0.002 (L1)           -494925.699543    0
    small3_sameMp     20, 24, 30   1.5e+01 (L1 q_sqrt)        5.2e-03 (L2 Z)      0.000 (L0)           -492839.859374    4.7e-16
    ch_264_72         264, 72      2.1e+00 (L1 variance)      2.3e-02 (L1 q_mu)   0.002 (L0)           -494965.524861    2.4e-16
    ch_72_264         72, 264      3.8e+01 (L1 lengthscales)  1.3e-03 (L1 Z)      0.010 (L1)           -493817.724036    1.3e-14
    wide_R33          24, 24       6.8e+00 (L1 variance)      1.2e-02 (L1 q_mu)   0.001 (L1)           -493150.140716    0

Every figure is printed by the last test of this module (run with -s).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import live_specs as ls                           # noqa: E402
from oracle_build import oracle_model             # noqa: E402

ELBO_RTOL = 1e-10        # oracle ELBO against the torch forward: the bound of test_hand_written_gradient_matches_torch_autograd

EXPECT = ls.EXPECT_MIXED
round_up, host_groups = ls.round_up, ls.host_groups


def test_every_case_has_its_expectation():
    assert set(EXPECT) == set(ls.CASES_MIXED)
    for k in ls.CASES_MIXED.values():
        assert k["N"] == 3 and "S" not in k and "seed" not in k          # S = 2 and seed 7: live_spec's defaults


@pytest.mark.parametrize("case", list(ls.CASES_MIXED))
def test_the_built_spec_reaches_what_the_table_claims(case):
    """Per-layer M, Mp, route, white flag and Rp of the built spec, the shapes of its parameters, and the factor groups that follow."""
    spec, X, Y, zs = ls.make_case(case)
    k, want = ls.CASES_MIXED[case], EXPECT[case]
    layers = spec["convs"] + [spec["head"]]
    assert spec["S"] == 2 and X.shape[0] == 3 and len(layers) == len(k["Ms"])
    assert tuple(l["M"] for l in layers) == tuple(k["Ms"])
    assert tuple(round_up(l["M"], 16) for l in layers) == want["Mp"]
    assert tuple(l["M"] > 256 for l in layers) == want["large"]
    assert tuple(bool(l["white"]) for l in layers) == want["white"] == tuple(k.get("whites", (False,) * len(layers)))
    assert tuple(round_up(l["R"], 16) for l in layers) == want["Rp"]
    for l in layers:
        M, R = l["M"], l["R"]
        assert np.shape(l["Z"])[0] == M and np.shape(l["q_mu"]) == (M, R) and np.shape(l["q_sqrt"]) == (R, M, M)
        if l["white"]:
            assert np.array_equal(l["q_sqrt"], np.tile(np.eye(M)[None], [R, 1, 1]))
    got = host_groups(spec)
    assert [g[:2] for g in got] == [g[:2] for g in want["groups"]]
    assert all(w[2] is None or w[2] == g[2] for g, w in zip(got, want["groups"])), (got, want["groups"])
    assert len(want["groups"]) == len(set(want["Mp"]))


def test_a_layer_is_the_one_its_own_single_M_spec_has():
    """mixed_live_spec keeps layer i from the live_spec call with Ms[i] and whites[i]: every value of it, and nothing of the other calls."""
    k = dict(ls.CASES_MIXED["small3_mixwhite"])
    k.pop("N")
    spec = ls.mixed_live_spec(**k)
    layers = spec["convs"] + [spec["head"]]
    for i, (M, w) in enumerate(zip(k["Ms"], k["whites"])):
        one = ls.live_spec(k["hwc"], k["convs"], k["head"], M, k["c"], k["a"], white=w)
        src = (one["convs"] + [one["head"]])[i]
        assert set(src) == set(layers[i])
        for key, val in src.items():
            assert np.array_equal(layers[i][key], val), (i, key)
    assert spec["S"] == one["S"] and spec["num_data"] == one["num_data"]


@pytest.mark.parametrize("case", list(ls.CASES_MIXED))
def test_every_gradient_group_is_live_and_the_references_agree(case):
    spec, X, Y, zs = ls.make_case(case)
    e, want = ls.torch_reference(spec, X, Y, zs)
    assert np.isfinite(e)
    for row in ls.liveness(want):
        print("%s L%d %-14s max %.3e  median/max %.3e  below the entry floor %.4f" % ((case,) + row))
    ls.assert_live(case, want)
    for groups in want:        # the reference's own q_sqrt gradient: nothing above the diagonal
        assert not np.triu(groups["q_sqrt"], 1).any()
    e_o = oracle_model(spec, X, Y).compute_log_likelihood(X, Y, zs=zs)
    print("%s ELBO torch %.6f  oracle %.6f  rel %.3e" % (case, e, e_o, abs(e - e_o) / abs(e_o)))
    assert abs(e - e_o) <= ELBO_RTOL * abs(e_o), (case, e, e_o)

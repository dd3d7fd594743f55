"""Models whose layers differ in M, whitening and width (tests/live_specs.py, CASES_MIXED) on the device, against torch autograd of the textbook
forward (tests/test_oracle_autograd.py) and the oracle.

The reference takes ``-M`` as a list, one count per layer.  The library has code of its own for that which no single-M spec reaches: one factor
group per distinct padded size Mp = round_up(M, 16) (csrc/model.hip, build_groups), with right-hand sides that ride the chain only for
unwhitened layers with Mp <= 256 and Rp <= 32 -- so one group can hold riding and non-riding matrices; the deferred factor copy only with a
single group (plan_step), the in-tail KL reading K / Kp without it (place_kl) and leaving the tail launch as soon as one layer is whitened;
status words walked over several groups (fill_status, first_bad_pivot); and each layer on the M <= 256 or the M > 256 route on its own,
forward and reverse.  What each case reaches is live_specs.EXPECT_MIXED; tests/test_host_mixed_layers.py checks that table and the liveness
of every reference gradient without a GPU.

Every bound is the one the single-M tests use for the same quantity: RTOL of tests/test_gpu_model.py (ELBO, data term, KL against the oracle;
the same 1e-9 is the ELBO's bound against torch in the gradient modules) and of tests/test_gpu_ops.py (layer outputs), TOL_GROUP / TOL_E of
tests/test_gpu_grad_large_m.py for a case with a layer above 256 and of tests/test_gpu_grad_m256.py otherwise, the Adam bounds of
test_adam_one_call_steps_match_numpy_on_torch_gradients_at_M200 / _at_M384, the kl_side bounds of
test_kl_pieces_in_the_tail_launch_match_the_kl_launches, the no_rhs_ride bound of test_chain_rhs_riding_matches_their_own_launch.

The factor groups a device model ran are read back from it (DGP_Base.factor_groups: Mp, matrices, matrices whose right-hand sides rode the
chain in the step) and compared with live_specs.EXPECT_MIXED, so a case that quietly folds into one group fails.  Every figure -- the groups,
the error of the ELBO and its parts, of every gradient group, of every Adam-stepped value, of every layer's outputs, the reported pivots -- is
printed before it is asserted (run with -s).  No device figure is recorded here: this module was written without access to an MI355X.
"""
import copy
import functools

import numpy as np
import pytest

from deepcgp_amd import synthetic as syn
from deepcgp_amd.models import build_from_spec
import live_specs as ls
from oracle_build import oracle_model, spec_from_model
import test_gpu_grad_large_m as large_m
import test_gpu_grad_m256 as m256
from test_gpu_model import RTOL
from test_gpu_ops import RTOL as RTOL_OPS

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]   # a hung launch ends the run instead of holding the device

CASES = list(ls.CASES_MIXED)
# the bounds of the Adam tests of the two gradient modules (three steps: the step's ELBO, variance / lengthscale, everything else)
ADAM_ELBO, ADAM_POSITIVE, ADAM_OTHER = 1e-8, 1e-8, 1e-7
KL_SIDE_RTOL = 1e-12     # test_kl_pieces_in_the_tail_launch_match_the_kl_launches: KL and ELBO; the data term to the bit
NO_RIDE_RTOL = 1e-11     # test_chain_rhs_riding_matches_their_own_launch


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def grad_bounds(spec):
    """(TOL_GROUP, TOL_E): the large-M module's where any layer is above 256, the M <= 256 module's otherwise."""
    mod = large_m if any(l["M"] > 256 for l in spec["convs"] + [spec["head"]]) else m256
    return mod.TOL_GROUP, mod.TOL_E


@functools.lru_cache(maxsize=None)
def _case(name):
    """(spec, X, Y, zs, e_t, want): the case and its torch reference, computed once per process; liveness asserted before anything else."""
    pytest.importorskip("torch")
    spec, X, Y, zs = ls.make_case(name)
    e_t, want = ls.torch_reference(spec, X, Y, zs)
    ls.assert_live(name, want)
    return spec, X, Y, zs, e_t, want


@functools.lru_cache(maxsize=None)
def _parts(name):
    """ELBO, data term and KL of a case by both CPU references, and the oracle's layer means and variances: computed once.  The torch forward
    returns the ELBO only: with num_data = 0 it is -KL, and the data term is what is left of the ELBO, over num_data / N."""
    import torch
    from test_oracle_autograd import _torch_elbo
    spec, X, Y, zs, e_t, _ = _case(name)
    kl_only = copy.deepcopy(spec)
    kl_only["num_data"] = 0
    with torch.no_grad():
        kl_t = -_torch_elbo(kl_only, X, Y, zs)[0].item()
    data_t = (e_t + kl_t) / (spec["num_data"] / X.shape[0])
    ref = oracle_model(spec, X, Y)
    _, om, ov = ref.propagate(X, S=spec["S"], zs=zs)
    return dict(torch=(e_t, data_t, kl_t), oracle=(ref.compute_log_likelihood(X, Y, zs=zs), ref.data_term(X, Y, zs=zs), ref.KL()), Fm=om, Fv=ov)


def check_groups(case, model):
    """The groups the device model built are the ones the case is there for (None: the riding count is not claimed)."""
    got, want = model.factor_groups(), ls.EXPECT_MIXED[case]["groups"]
    print("%s factor groups (Mp, matrices, riding): %s" % (case, got))
    assert [g[:2] for g in got] == [w[:2] for w in want], (case, got, want)
    for g, w in zip(got, want):
        assert w[2] is None or g[2] == w[2], (case, got, want)


@pytest.mark.parametrize("dedup", [False, True], ids=["tiled", "dedup"])
@pytest.mark.parametrize("case", CASES)
def test_elbo_and_its_parts_match_torch_and_the_oracle(ctx, case, dedup):
    spec, X, Y, zs, _, _ = _case(case)
    p = _parts(case)
    model = build_from_spec(spec, X, Y)
    assert model.factor_groups() == []
    model.dedup_layer0 = dedup
    got = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    check_groups(case, model)
    for src in ("torch", "oracle"):
        for what, g, w in zip(("elbo", "data", "kl"), got, p[src]):
            print("%s%s %-6s %-4s device %.9f  rel %.3e" % (case, "-dedup" if dedup else "", src, what, g, abs(g - w) / max(abs(w), 1.0)))
    for src in ("torch", "oracle"):
        e, data, kl = p[src]
        assert abs(got[0] - e) <= RTOL * abs(e), (case, src, "elbo", got[0], e)
        assert abs(got[1] - data) <= RTOL * abs(data), (case, src, "data", got[1], data)
        assert abs(got[2] - kl) <= RTOL * max(abs(kl), 1.0), (case, src, "kl", got[2], kl)
    assert model.compute_log_likelihood(X, Y, zs=zs, return_parts=True) == got          # the other bank: the same bits
    assert abs(model.KL() - got[2]) <= 1e-10 * abs(got[2])                               # the operator API, layer by layer (test_golden_vectors)
    model.close()


GRAD = [(c, False) for c in CASES] + [("small3_20_40_24", True), ("ch_72_264", True)]


@pytest.mark.parametrize("case,dedup", GRAD, ids=["%s%s" % (c, "-dedup" if d else "") for c, d in GRAD])
def test_gradient_matches_torch_autograd_entry_by_entry(ctx, case, dedup):
    """ELBO to 1e-9, every group of every layer group-wise and entry-wise over the floor, q_sqrt's gradient zero above the diagonal, the same
    bits when the step is repeated."""
    spec, X, Y, zs, e_t, want = _case(case)
    tol_group, tol_e = grad_bounds(spec)
    tag = case + ("-dedup" if dedup else "")
    model = build_from_spec(spec, X, Y)
    model.dedup_layer0 = dedup
    e, grads = model.compute_gradients(X, Y, zs=zs)
    e2, grads2 = model.compute_gradients(X, Y, zs=zs)
    assert [g[:2] for g in model.factor_groups()] == [w[:2] for w in ls.EXPECT_MIXED[case]["groups"]]
    rows = []
    for li, groups in enumerate(want):
        assert set(groups) == set(grads[li]), (tag, li)
        for name, w in groups.items():
            got = np.asarray(grads[li][name], np.float64)
            assert got.shape == np.shape(w), (tag, li, name)
            rows.append((li, name) + ls.errors(name, got, w))
            print("%s L%d %-14s group %.3e  entry %.3e  |want|max %.3e" % ((tag,) + rows[-1] + (np.abs(w).max(),)))
    print("%s elbo rel %.3e  WORST group %.3e entry %.3e" % (tag, abs(e - e_t) / abs(e), max(r[2] for r in rows), max(r[3] for r in rows)))
    assert abs(e - e_t) <= RTOL * abs(e), (tag, e, e_t)
    for li, name, err_g, err_e in rows:
        assert err_g <= tol_group, (tag, li, name, "group-wise", err_g)
        assert err_e <= tol_e, (tag, li, name, "entry-wise", err_e)
    for li, g in enumerate(grads):
        assert not np.triu(g["q_sqrt"], 1).any(), (tag, li, "q_sqrt above the diagonal")
    assert e == e2
    for li, (a, b) in enumerate(zip(grads, grads2)):
        for name in a:
            assert np.array_equal(a[name], b[name]), (tag, li, name, "repeat")
    model.close()


@pytest.mark.parametrize("case", CASES)
def test_three_adam_steps_match_numpy_on_torch_gradients(ctx, case):
    """Three one-call training steps against NumPy Adam on torch gradients recomputed after every step; the values read back with
    pull_parameters."""
    spec = copy.deepcopy(_case(case)[0])
    _, X, Y, _, _, _ = _case(case)
    N, lr, state = X.shape[0], 0.05, {}
    model = build_from_spec(spec, X, Y)
    for t in range(1, 4):
        z = syn.make_noise(spec, N, seed=100 + t)
        e = model.train_step(X, Y, lr, zs=z, t=t)
        e_t, g = ls.torch_reference(spec, X, Y, z)
        print("%s adam t%d elbo rel %.3e" % (case, t, abs(e - e_t) / abs(e_t)))
        assert abs(e - e_t) <= ADAM_ELBO * abs(e_t), (case, t, e, e_t)
        ls.adam_numpy_step(spec, g, state, lr, t)
    model.pull_parameters()
    rows = []
    for li, (l, now) in enumerate(zip(spec["convs"] + [spec["head"]], ls.model_values(model))):
        for name in now:
            rows.append((li, name, rel(now[name], l[ls.SPEC_KEY[name]])))
            print("%s adam L%d %-14s rel %.3e" % ((case,) + rows[-1]))
    for li, name, err in rows:
        assert err < (ADAM_POSITIVE if name in ls.POSITIVE else ADAM_OTHER), (case, li, name, err)
    model.close()


@pytest.mark.parametrize("case", CASES)
def test_kl_placement_and_riding_do_not_change_the_numbers(ctx, case):
    """ctx option kl_side (the KL pieces by their own launches on the side stream, wherever the default puts them): the same data term to
    the bit, KL and ELBO to 1e-12.  ctx option no_rhs_ride (G / alpha of every layer by their own launch, where the default lets some matrices
    of a group ride the chain and others not): equal to 1e-11, and no matrix rides."""
    spec, X, Y, zs, _, _ = _case(case)
    model = build_from_spec(spec, X, Y)
    e, data, kl = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    with ctx.options(kl_side=1):
        e2, data2, kl2 = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    print("%s kl_side: kl rel %.3e  elbo rel %.3e  data equal %s" % (case, abs(kl2 - kl) / abs(kl), abs(e2 - e) / abs(e), data2 == data))
    assert data2 == data and abs(kl2 - kl) <= KL_SIDE_RTOL * abs(kl) and abs(e2 - e) <= KL_SIDE_RTOL * abs(e)
    with ctx.options(no_rhs_ride=1):
        off = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
        assert all(g[2] == 0 for g in model.factor_groups()), model.factor_groups()
    print("%s no_rhs_ride: rel %.3e %.3e %.3e" % ((case,) + tuple(abs(a - b) / abs(b) for a, b in zip(off, (e, data, kl)))))
    np.testing.assert_allclose(off, (e, data, kl), rtol=NO_RIDE_RTOL, atol=0)
    assert model.compute_log_likelihood(X, Y, zs=zs, return_parts=True) == (e, data, kl)
    model.close()


@pytest.mark.parametrize("case", ["small3_20_40_24", "ch_72_264"])
def test_factor_reuse_and_steps_in_flight_give_the_same_bits(ctx, case):
    """A step at unchanged parameters that reuses the chain of the step before it (set_factor_reuse, mode 2) is bit-identical to the step
    that ran it, for the ELBO and for propagate; two steps in flight on different batches hand back the synchronous values."""
    spec, X, Y, zs, _, _ = _case(case)
    p = _parts(case)
    S = spec["S"]
    model = build_from_spec(spec, X, Y)
    with ctx.options(no_factor_reuse=1):
        first = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
        _, Fm0, Fv0 = model.propagate(X, S=S, zs=zs)
        again = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    assert model.chain_skips == 0 and again == first
    model.set_factor_reuse(2)
    reused = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)       # same kind of chain as the step before it
    assert model.chain_skips == 1 and reused == first
    zs2 = [z[:, :2] for z in zs]
    short = model.compute_log_likelihood(X[:2], Y[:2], zs=zs2, return_parts=True)   # another batch, same parameters
    assert model.chain_skips == 2
    _, Fm1, Fv1 = model.propagate(X, S=S, zs=zs)       # a chain without KL pieces is another kind: it runs ...
    _, Fm2, Fv2 = model.propagate(X, S=S, zs=zs)       # ... and is reused here
    assert model.chain_skips == 3
    for i in range(len(Fm0)):
        assert np.array_equal(Fm1[i], Fm0[i]) and np.array_equal(Fv1[i], Fv0[i]), i
        assert np.array_equal(Fm2[i], Fm0[i]) and np.array_equal(Fv2[i], Fv0[i]), i
    assert rel(Fm2[-1], p["Fm"][-1]) < RTOL and rel(Fv2[-1], p["Fv"][-1]) < RTOL
    model.set_factor_reuse(1)
    with ctx.options(no_factor_reuse=1):
        short0 = model.compute_log_likelihood(X[:2], Y[:2], zs=zs2, return_parts=True)
    assert short == short0
    for _ in range(2):
        tickets = [model.enqueue_log_likelihood(X, Y, zs=zs), model.enqueue_log_likelihood(X[:2], Y[:2], zs=zs2)]
        assert [model.collect_log_likelihood(t, return_parts=True) for t in tickets] == [first, short0]
    assert model.compute_log_likelihood(X, Y, zs=zs, return_parts=True) == first
    model.close()


@pytest.mark.parametrize("case", ["small3_20_40_24", "ch_264_72"])
def test_layer_outputs_match_the_oracle(ctx, case):
    """propagate: the means and variances of every layer against the oracle's propagate."""
    spec, X, Y, zs, _, _ = _case(case)
    p = _parts(case)
    model = build_from_spec(spec, X, Y)
    _, Fm, Fv = model.propagate(X, S=spec["S"], zs=zs)
    assert len(Fm) == len(p["Fm"]) == len(spec["convs"]) + 1
    for i in range(len(Fm)):
        print("%s layer %d mean rel %.3e  var rel %.3e" % (case, i, rel(Fm[i], p["Fm"][i]), rel(Fv[i], p["Fv"][i])))
    for i in range(len(Fm)):
        assert Fm[i].shape == p["Fm"][i].shape
        assert rel(Fm[i], p["Fm"][i]) < RTOL_OPS and rel(Fv[i], p["Fv"][i]) < RTOL_OPS, i
    model.close()


@pytest.mark.parametrize("which", ["Z", "Z_prior"])
def test_failed_factorisation_in_the_second_group_is_reported(ctx, which):
    """small3_20_40_24: layer 1 (Mp = 48) is alone in the SECOND factor group, its Kuu(Z) that group's first matrix and the prior's Kuu(Z0)
    its second.  One NaN row of Z (of the prior's Z0) makes that one matrix fail at the row's column -- in the second panel of its chain --
    while every matrix of the first group is healthy.  The synchronous and the enqueued step both raise NotPositiveDefinite with the column
    _potrf reports for that matrix alone; a following step with healthy parameters is clean and gives the value from before."""
    from deepcgp_amd.device import NotPositiveDefinite
    from deepcgp_amd.layers import _potrf
    case, li, row = "small3_20_40_24", 1, 35
    spec, X, Y, zs, e_t, _ = _case(case)
    assert ls.EXPECT_MIXED[case]["Mp"][li] == ls.EXPECT_MIXED[case]["groups"][1][0] != ls.EXPECT_MIXED[case]["groups"][0][0]
    model = build_from_spec(spec, X, Y)
    good = model.compute_log_likelihood(X, Y, zs=zs, return_parts=True)
    layer = model.layers[li]
    keep = np.array(layer.feature.Z if which == "Z" else layer.Z_prior)
    bad = keep.copy()
    bad[row] = np.nan
    c = spec["convs"][li]
    with pytest.raises(NotPositiveDefinite) as alone:
        _potrf(syn._rbf(bad, bad, c["variance"], c["ls"]) + syn.JITTER * np.eye(c["M"]))
    assert 0 < alone.value.column <= row + 1, alone.value.column       # (the NaN row's own pivot at the latest)
    if which == "Z":
        layer.feature.Z = bad
    else:
        layer.Z_prior = bad
    model.sync_parameters()
    with pytest.raises(NotPositiveDefinite) as sync:
        model.compute_log_likelihood(X, Y, zs=zs)
    t = model.enqueue_log_likelihood(X, Y, zs=zs)
    with pytest.raises(NotPositiveDefinite) as flight:
        model.collect_log_likelihood(t)
    print("%s NaN row %d of layer %d's %s: column alone %d  synchronous %d  in flight %d" % (case, row, li, which, alone.value.column,
                                                                                      sync.value.column, flight.value.column))
    assert sync.value.column == alone.value.column and flight.value.column == alone.value.column
    if which == "Z":
        layer.feature.Z = keep
    else:
        layer.Z_prior = keep
    model.sync_parameters()
    assert model.compute_log_likelihood(X, Y, zs=zs, return_parts=True) == good
    t = model.enqueue_log_likelihood(X, Y, zs=zs)
    assert model.collect_log_likelihood(t, return_parts=True) == good
    assert abs(good[0] - e_t) <= RTOL * abs(e_t)
    model.close()


def test_model_builder_with_two_groups_from_flags(ctx):
    """ModelBuilder with ``-M 20,40`` (Mp 32 and 48: two factor groups): the ELBO at explicit noise against the oracle built from the same
    parameters, and the reference's training loop for three steps: finite, and every parameter group of every layer moves."""
    from deepcgp_amd.arguments import default_parser
    from deepcgp_amd.models import ModelBuilder, train
    rng = np.random.default_rng(0)
    np.random.seed(0)
    X = rng.standard_normal((40, 12, 12, 1))
    Y = rng.integers(0, 10, (40, 1))
    flags = default_parser().parse_args(['--name', 't', '-M', '20,40', '--feature-maps', '3', '--filter-sizes', '3,3', '--strides', '2,1',
                                         '--num-samples', '2', '--batch-size', '8'])
    model = ModelBuilder(flags, X, Y).build()
    conv, head = model.layers
    assert conv.feature.Z.shape == (20, 9) and head.feature.Z.shape == (40, 27)
    spec = spec_from_model(model)
    Xb, Yb = X[:8].reshape(8, -1), Y[:8].reshape(-1)
    zs = syn.make_noise(spec, 8, seed=3)
    e = model.compute_log_likelihood(Xb, Yb, zs=zs)
    assert [g[:2] for g in model.factor_groups()] == [(32, 2), (48, 1)], model.factor_groups()
    ref = oracle_model(spec, Xb, Yb).compute_log_likelihood(Xb, Yb, zs=zs)
    print("-M 20,40: ELBO %.9f oracle %.9f rel %.3e  groups %s" % (e, ref, abs(e - ref) / abs(ref), model.factor_groups()))
    assert abs(e - ref) <= 1e-9 * abs(ref), (e, ref)
    before = ls.model_values(model)
    hist = train(model, 3)
    assert len(hist) == 3 and np.all(np.isfinite(hist)), hist
    for li, (b, now) in enumerate(zip(before, ls.model_values(model))):
        for name in b:
            assert np.all(np.isfinite(now[name])), (li, name)
            assert not np.array_equal(now[name], b[name]), (li, name, "did not move")
    model.close()

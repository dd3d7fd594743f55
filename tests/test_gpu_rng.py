"""The device-drawn layer noise (``seed=``: csrc/rng.h's philox_normal at the counters of model.hip / layer_impl.h, drawn by conv_fused.hip's
phase 4 and cond.hip's finalize_kernel) against the host Philox reference of tests/rng_ref.py (checked without a GPU in
tests/test_host_rng.py).

The comparison is device against device: the same model once with ``seed=s`` and once with ``zs=rng_ref.device_noise(..., s)``.  The
explicit-noise path of every stack below is tied to torch or the oracle by the file that owns the stack, so this closes the chain for the
path every training step takes.  No tolerance is this file's own -- the host's log / cos and the device's log / cospi differ by a few ulp
in z:

    layer samples, means, variances              RTOL of tests/test_gpu_ops.py (1e-9)
    ELBO, data term, KL                          RTOL of tests/test_gpu_model.py (1e-9)
    gradient of every group, entry by entry      TOL_GROUP / TOL_E of tests/test_gpu_grad_m256.py, of tests/test_gpu_grad_large_m.py where a
                                                 layer has M > 256 (test_gpu_padding.grad_bounds, tests/live_specs.py: errors)
    evaluate: log density, class probabilities   RTOL of tests/test_gpu_evaluate.py (1e-9)

The stacks, each the smallest of its helper that takes the route (N = 3, S = 2; plain: N = 4, S = 3):

    plain          the 14 x 14 two-layer spec of test_gpu_model.py::test_gradient_with_device_rng_matches_explicit_noise: the one-launch kernel
    res3           padding_ref: two conv layers whose counters run over the same range -- they must not draw the same noise
    ch_264_72      padding_ref: M = 264, the sweep + GEMM route and finalize_kernel
    mix_a_3_5, mix_m264   mixing_ref: 3 latent GPs into 5 (10) maps -- the noise is G wide, not Rout
    dil2_odd, dil3_pad, ch_264_72_d2   dilation_ref: phase layout with phantom positions, padding, the sweep + GEMM route
    mean_ch_res    conv_mean_ref: the mean filter's pass behind the launch

``propagate`` always tiles its batch, so the layer outputs are compared once per stack and seed; the ELBO and the gradient run under both
``dedup_layer0`` settings (a de-duplicated first layer draws per replica: shared noise between replicas moves the ELBO).  Every figure is
printed before it is asserted (run with -s; lines that start with RNG), the largest per quantity again at the end of the module.

Largest figure seen per quantity on an MI355X, with the case that came closest to its bound:

    quantity                              largest     bound     closest case
    layer sample / mean                   2.1e-14     1e-9      ch_264_72_d2, seed 77: the head behind layer 0's device draw
    layer variance                        1.4e-15     1e-9      plain, seed 77: the head behind layer 1's device draw
    ELBO / data term                      2.4e-16 / 1.4e-16  1e-9   mix_a_3_5 (dedup), seed 77;  KL: the same bits (it sees no noise)
    gradient, group-wise                  1.8e-11     1e-7      ch_264_72_d2, seed (9 << 32) | 5, layer 0 variance
    gradient, entry-wise, M <= 256        2.4e-11     5.3e-6    mean_ch_res, seed (9 << 32) | 5, layer 0 Z
    gradient, entry-wise, a layer M > 256 1.9e-8      7.6e-6    ch_264_72 (dedup), seed (9 << 32) | 5, layer 0 Z
    evaluate: log density / p_mean        1.9e-16 / 4.2e-16  1e-9   plain, seed 77
    train_step: ELBO                      the same bits; parameters behind the step: at most 8.9e-16 apart (dedup; tiled 2.5e-16)
    shards of worlds 2 and 3, chunks      bit-identical with the rows of the un-sharded / un-chunked seed run, every layer's sample, mean, variance

The closest any quantity came to its bound is the entry-wise gradient with a layer at M > 256: 0.26 % of TOL_E, on entries of Z near the
entry floor, where that route's own rounding (the floor TOL_E was derived from) multiplies the few ulp by which the two z differ; nothing
came within two orders of its bound.  All 97 cases passed and no counter was found wrong: the library's map is the one rng_ref.py states.
The only library change is the ctx option fwd_chunk_rows, which lets the chunked route run on a small batch.

Three mutations of the library made by hand (not committed), each run against this file and against test_gpu_model.py, test_gpu_train_run.py,
test_gpu_evaluate.py, test_gpu_dilation.py, test_gpu_mixing.py and test_gpu_fused_rep_share.py as they were:

    every layer on stream 1 (``li + 1`` -> ``1``)       34 cases here fail: layer outputs, ELBO, gradient of the three stacks with two conv
                                                        layers (plain, res3, mean_ch_res), evaluate[plain], train_step, the shard test;
                                                        none of the older files noticed
    ``s * rep_stride`` dropped from the noise index     37 cases here fail: ELBO and gradient of every stack under dedup, train_step[dedup];
                                                        of the older tests test_gradients_are_bitwise_reproducible_at_full_size noticed
                                                        (its tiled-against-dedup comparison under one seed)
    ``col0`` dropped from finalize_kernel's noise index both chunk tests here fail; of the older tests test_oversized_operand_slab noticed
                                                        (on its 2.36 GB slab)
"""
import copy
import functools

import numpy as np
import pytest

from deepcgp_amd import synthetic as syn
from deepcgp_amd.dist import shard_range
from deepcgp_amd.models import build_from_spec
import conv_mean_ref as cmr
import dilation_ref as dr
import live_specs as ls
import mixing_ref as mr
import padding_ref as pr
import rng_ref as rr
from test_gpu_evaluate import RTOL as RTOL_EVAL
from test_gpu_model import RTOL
from test_gpu_ops import RTOL as RTOL_OPS
from test_gpu_padding import grad_bounds

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120, method="thread")]   # a hung launch ends the run instead of holding the device

SEEDS = [77, (9 << 32) | 5]
SEED = pytest.mark.parametrize("seed", SEEDS, ids=["seed77", "seedhigh"])
DEDUP = pytest.mark.parametrize("dedup", [False, True], ids=["tiled", "dedup"])
PLAIN_HWC = (14, 14, 1)


def _plain(N=4):
    spec = syn.make_spec(PLAIN_HWC, [(3, 1, 3), (4, 2, 2)], (3, 1), 20, S=3, num_data=500, seed=12, conv_q_sqrt_scale=0.3, variance=2.0, ls=1.5)
    return (spec,) + syn.make_batch(PLAIN_HWC, N, seed=12)


CASES = {
    "plain": _plain,
    "res3": lambda: pr.make_stack("res3")[:3],
    "ch_264_72": lambda: pr.make_stack("ch_264_72")[:3],
    "mix_a_3_5": lambda: mr.make_case("a_3_5")[:3],
    "mix_m264": lambda: mr.make_case("m264")[:3],
    "dil2_odd": lambda: dr.make_stack("dil2_odd")[:3],
    "dil3_pad": lambda: dr.make_stack("dil3_pad")[:3],
    "ch_264_72_d2": lambda: dr.make_stack("ch_264_72_d2", N=3)[:3],
    "mean_ch_res": lambda: cmr.make_case("ch_res")[:3],
}
CASE = pytest.mark.parametrize("name", list(CASES))
WORST = {}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def figure(what, value, bound, tag):
    print("RNG %-26s %.3e  bound %.1e  %s" % (what, value, bound, tag))
    if value / bound >= WORST.get(what, (0.0, 0.0, -1.0, ""))[2]:
        WORST[what] = (value, bound, value / bound, tag)
    return value


@pytest.fixture(scope="module", autouse=True)
def _largest_figures():
    yield
    for what, (value, bound, share, tag) in sorted(WORST.items()):
        print("\nRNG LARGEST %-26s %.3e  bound %.1e  share %.1e  %s" % (what, value, bound, share, tag), end="")
    print()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(spec, X, Y) of a stack, once per process; never written to."""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def _ref(name, seed):
    """The host reference of the noise the stack's model draws under ``seed``, computed once; never written to."""
    spec, X, _ = _case(name)
    return rr.device_noise(spec, X.shape[0], spec["S"], seed)


def _model(name, dedup=False):
    spec, X, Y = _case(name)
    model = build_from_spec(copy.deepcopy(spec), X.copy(), Y.copy())
    model.dedup_layer0 = dedup
    return model


def _layer_figures(tag, got, want):
    """rel of every layer's (sample, mean, variance); printed, returned for the assertions."""
    out = []
    for li in range(len(want[0])):
        for what, g, w in zip(("sample", "mean", "variance"), (got[0][li], got[1][li], got[2][li]), (want[0][li], want[1][li], want[2][li])):
            assert g.shape == w.shape, (tag, li, what)
            out.append((li, what, figure("layer " + what, rel(g, w), RTOL_OPS, "%s L%d" % (tag, li))))
    return out


# ---- 1. layer outputs ---------------------------------------------------------------------------------------------------------------------
@SEED
@CASE
def test_layer_outputs_under_a_seed_are_those_of_the_reference_noise(ctx, name, seed):
    """``propagate(seed=s)`` against ``propagate(zs=reference)``, every layer's sample, mean and variance; then one layer at a time on the
    device draw (its ``zs`` entry None, the others from the reference), so that a layer with a wrong counter names itself."""
    spec, X, Y = _case(name)
    S, zs = spec["S"], _ref(name, seed)
    tag = "%s seed %#x" % (name, seed)
    model = _model(name)
    want = model.propagate(X, S=S, zs=zs)
    rows = _layer_figures(tag + " all layers drawn", model.propagate(X, S=S, seed=seed), want)
    for li in range(len(zs) - 1):
        one = list(zs)
        one[li] = None
        rows += [(li,) + r for r in _layer_figures(tag + " only L%d drawn" % li, model.propagate(X, S=S, zs=one, seed=seed), want)]
    model.close()
    assert [z.shape for z in zs[:-1]] == [(S, X.shape[0], d) for d in model._out_dims()[:-1]]
    for r in rows:
        assert r[-1] < RTOL_OPS, (tag, r)
    assert not np.array_equal(want[0][0][0], want[0][0][1])      # (the samples of an image differ: the noise is live in what was compared)


# ---- 2. ELBO ------------------------------------------------------------------------------------------------------------------------------
@DEDUP
@SEED
@CASE
def test_elbo_under_a_seed_is_that_of_the_reference_noise(ctx, name, seed, dedup):
    spec, X, Y = _case(name)
    tag = "%s%s seed %#x" % (name, "-dedup" if dedup else "", seed)
    model = _model(name, dedup)
    got = model.compute_log_likelihood(X, Y, seed=seed, return_parts=True)
    want = model.compute_log_likelihood(X, Y, zs=_ref(name, seed), return_parts=True)
    other = model.compute_log_likelihood(X, Y, seed=seed + 1, return_parts=True)
    model.close()
    figs = [figure(what, abs(g - w) / max(abs(w), 1.0 if what == "KL" else 1e-300), RTOL, tag) for what, g, w in zip(("ELBO", "data term", "KL"), got, want)]
    assert max(figs) <= RTOL, (tag, got, want)
    assert abs(other[1] - got[1]) > 1e3 * RTOL * abs(got[1]), (tag, "the data term does not see the seed", got, other)


# ---- 3. gradient --------------------------------------------------------------------------------------------------------------------------
@DEDUP
@SEED
@CASE
def test_gradient_under_a_seed_is_that_of_the_reference_noise(ctx, name, seed, dedup):
    """Every group of every layer, group-wise and entry-wise (tests/live_specs.py: errors): the reverse pass recovers the noise the forward
    pass drew, on every route."""
    spec, X, Y = _case(name)
    tol_group, tol_e = grad_bounds(spec)
    tag = "%s%s seed %#x" % (name, "-dedup" if dedup else "", seed)
    model = _model(name, dedup)
    e, grads = model.compute_gradients(X, Y, seed=seed)
    e_w, want = model.compute_gradients(X, Y, zs=_ref(name, seed))
    model.close()
    figure("ELBO (gradient step)", abs(e - e_w) / abs(e_w), RTOL, tag)
    rows = []
    bound = "M > 256" if any(l["M"] > 256 for l in spec["convs"] + [spec["head"]]) else "M <= 256"
    for li, groups in enumerate(want):
        assert set(groups) == set(grads[li]), (tag, li)
        for gname, w in groups.items():
            err_g, err_e = ls.errors(gname, grads[li][gname], w)
            rows.append((li, gname, figure("gradient group-wise", err_g, tol_group, "%s L%d %s" % (tag, li, gname)),
                         figure("gradient entry-wise " + bound, err_e, tol_e, "%s L%d %s" % (tag, li, gname))))
    assert abs(e - e_w) <= RTOL * abs(e_w), (tag, e, e_w)
    for li, gname, err_g, err_e in rows:
        assert err_g <= tol_group, (tag, li, gname, "group-wise", err_g)
        assert err_e <= tol_e, (tag, li, gname, "entry-wise", err_e)


# ---- 4. shards ----------------------------------------------------------------------------------------------------------------------------
def test_a_shard_draws_the_rows_of_the_unsharded_batch(ctx):
    """``set_shard(lo, 7)`` for the ranks of worlds 2 and 3: the layer outputs of a shard's images under a seed are rows lo .. hi of the
    un-sharded seed run, bit for bit (the counter of an element is its position in the global batch); and they are those of the reference's
    sharded noise."""
    spec, X, Y = _plain(N=7)
    S, Ng, seed = spec["S"], 7, SEEDS[1]
    model = build_from_spec(spec, X, Y)
    full = model.predict_all_layers(X, S, seed=seed)
    rows = _layer_figures("plain N = 7 un-sharded", full, model.predict_all_layers(X, S, zs=rr.device_noise(spec, Ng, S, seed)))
    equal = []
    for world in (2, 3):
        for r in range(world):
            lo, hi = shard_range(Ng, r, world)
            model.set_shard(lo, Ng)
            part = model.predict_all_layers(X[lo:hi], S, seed=seed)
            tag = "plain shard %d of %d, images %d .. %d" % (r, world, lo, hi - 1)
            rows += _layer_figures(tag, part, model.predict_all_layers(X[lo:hi], S, zs=rr.device_noise(spec, hi - lo, S, seed, rank=r, shard=(lo, Ng))))
            for k, what in enumerate(("sample", "mean", "variance")):
                for li in range(len(model.layers)):
                    same = np.array_equal(part[k][li], full[k][li][:, lo:hi])
                    print("RNG %s L%d %s bit-identical with the un-sharded rows: %s (rel %.3e)" % (tag, li, what, same, rel(part[k][li], full[k][li][:, lo:hi])))
                    equal.append((tag, li, what, same))
    model.set_shard(0, 0)
    again = model.predict_all_layers(X, S, seed=seed)
    model.close()
    for r in rows:
        assert r[-1] < RTOL_OPS, r
    assert all(e[-1] for e in equal), [e for e in equal if not e[-1]]
    assert all(np.array_equal(a, b) for k in range(3) for a, b in zip(again[k], full[k]))      # the shard is taken off again


# ---- 5. the chunked route -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_rows", [1, 4])
def test_a_chunk_of_the_sweep_gemm_route_draws_at_its_global_column(ctx, chunk_rows):
    """ch_264_72 (M = 264) with the forward pass cut into chunks of whole images (ctx option fwd_chunk_rows: 6 rows in chunks of 1, and of 4 + 2),
    the route a batch above the 2 GiB operand slab takes: a chunk's outputs and counters are those of its columns in the whole batch
    (finalize_kernel's col0), so the chunked seed run equals the un-chunked run on the reference noise.  The number of finalize launches
    shows that the chunks were taken."""
    name, seed = "ch_264_72", SEEDS[1]
    spec, X, Y = _case(name)
    S, zs = spec["S"], _ref(name, seed)
    n_chunks = -(-S * X.shape[0] // chunk_rows)
    model = _model(name)
    want = model.propagate(X, S=S, zs=zs)
    ctx.timing_reset()
    ctx.timing_enable(1)
    try:
        whole = model.propagate(X, S=S, seed=seed)
        n_whole = ctx.timing().get("finalize", (0, 0.0))[0]
        ctx.timing_reset()
        with ctx.options(fwd_chunk_rows=chunk_rows):
            got = model.propagate(X, S=S, seed=seed)
            got_z = model.propagate(X, S=S, zs=zs)
        n_chunked = ctx.timing().get("finalize", (0, 0.0))[0]
    finally:
        ctx.timing_enable(0)
        ctx.timing_reset()
    model.close()
    print("RNG finalize launches: %d un-chunked, %d for two passes in chunks of %d rows" % (n_whole, n_chunked, chunk_rows))
    rows = _layer_figures("%s chunks of %d, seed" % (name, chunk_rows), got, want)
    rows += _layer_figures("%s chunks of %d, reference noise" % (name, chunk_rows), got_z, want)
    print("RNG chunked seed run bit-identical with the un-chunked seed run: %s" % all(np.array_equal(a, b) for k in range(3) for a, b in zip(got[k], whole[k])))
    assert n_whole >= 1 and n_chunked - 2 * n_whole == 2 * (n_chunks - 1), (n_whole, n_chunked, n_chunks)    # one more launch per further chunk
    for r in rows:
        assert r[-1] < RTOL_OPS, r


# ---- 6. evaluate --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "ch_264_72"])
def test_evaluate_draws_batch_b_under_seed_plus_b(ctx, name):
    """``evaluate(batch_size=2, seed=s)`` on three images: batch b (2 + 1 images, each starting at row 0 of its own forward pass) draws under
    s + b, so it equals ``evaluate(zs=...)`` with batch b's noise from the reference at seed s + b."""
    spec, X, Y = _case(name)
    X, Y = X[:3], Y[:3]
    S, bs = spec["S"], 2
    model = _model(name)
    for seed in SEEDS:
        parts = [rr.device_noise(spec, min(bs, 3 - lo), S, seed + b) for b, lo in enumerate(range(0, 3, bs))]
        zs = [np.concatenate([p[li] for p in parts], axis=1) for li in range(len(spec["convs"]))] + [None]
        got = model.evaluate(X, Y, S=S, batch_size=bs, seed=seed, per_image=True)
        want = model.evaluate(X, Y, S=S, batch_size=bs, zs=zs, per_image=True)
        same_seed = model.evaluate(X, Y, S=S, batch_size=bs, zs=rr.device_noise(spec, 3, S, seed), per_image=True)
        tag = "%s seed %#x" % (name, seed)
        a = figure("evaluate log density", rel(got["log_density"], want["log_density"]), RTOL_EVAL, tag)
        b = figure("evaluate p_mean", rel(got["p_mean"], want["p_mean"]), RTOL_EVAL, tag)
        c = figure("evaluate mean log density", abs(got["mean_log_density"] - want["mean_log_density"]) / abs(want["mean_log_density"]), RTOL_EVAL, tag)
        assert max(a, b, c) < RTOL_EVAL and got["accuracy"] == want["accuracy"], tag
        assert rel(got["log_density"][bs:], same_seed["log_density"][bs:]) > 1e3 * RTOL_EVAL, (tag, "the second batch does not see its seed")
    model.close()


# ---- 7. train_step ------------------------------------------------------------------------------------------------------------------------
@DEDUP
def test_train_step_under_a_seed_is_the_step_on_the_reference_noise(ctx, dedup):
    """One Adam step of the plain stack under a seed against the step on the reference noise: the ELBO within RTOL.  The parameters behind
    the step are compared and printed; they need not be bit-equal (the first Adam step is lr g / (|g| + 1e-8): where |g| is of the order of
    1e-8 a difference in the last bits of g is a visible share of the step), but no parameter of either model moved by more than lr in its
    unconstrained form, so 2 lr bounds the difference of every constrained value (softplus and the identity have slope <= 1)."""
    name, seed, lr = "plain", SEEDS[1], 0.01
    spec, X, Y = _case(name)
    a, b = _model(name, dedup), _model(name, dedup)
    ea = a.train_step(X, Y, lr, seed=seed)
    eb = b.train_step(X, Y, lr, zs=_ref(name, seed))
    tag = "plain%s" % ("-dedup" if dedup else "")
    f = figure("train_step ELBO", abs(ea - eb) / abs(eb), RTOL, tag)
    for m in (a, b):
        m.pull_parameters()
    start = build_from_spec(copy.deepcopy(spec), X, Y)
    worst, moved = 0.0, 0
    for pa, pb, p0 in zip(a.parameters, b.parameters, start.parameters):
        va, vb, v0 = (np.asarray(p.value, np.float64) for p in (pa, pb, p0))
        assert pa.pathname == pb.pathname == p0.pathname
        d = float(np.max(np.abs(va - vb))) if va.size else 0.0
        worst, moved = max(worst, d), moved + int(not np.array_equal(vb, v0))
        print("RNG %s %-50s |seed - reference|max %.3e  |step|max %.3e  bit-equal %s" % (tag, pa.pathname, d, float(np.max(np.abs(vb - v0))) if vb.size else 0.0,
                                                                                  np.array_equal(va, vb)))
        assert d <= 2.0 * lr, (tag, pa.pathname, d)
    a.close(), b.close()
    print("RNG %s parameters after the step: largest difference %.3e (lr %.0e), %d of %d moved" % (tag, worst, lr, moved, len(b.parameters)))
    assert f <= RTOL, (tag, ea, eb)
    assert moved >= len(b.parameters) - 1, (tag, moved)

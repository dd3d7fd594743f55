"""The host reference of the device-drawn layer noise (tests/rng_ref.py), without a GPU: its words are Philox4x32-10's, its normals are
normal and uncorrelated where the library relies on it, and its counter map keeps layers, ranks, replicas and shards apart.  The device is
held to this reference in tests/test_gpu_rng.py.

The distribution checks are conditions on fixed inputs, n = 2^20 draws at three (seed, stream) pairs: every raw moment within 4 standard
errors of the normal's (1 / sqrt n, sqrt(2 / n), sqrt(15 / n), sqrt(96 / n)), Kolmogorov-Smirnov p >= 0.01, correlations within 4 / sqrt n.
A plain scalar mirror of csrc/rng.h run on a CPU for exactly these inputs gave moments within about 2 standard errors, KS p of 0.18, 0.25 and
0.61 and a largest correlation of 1.5 / sqrt n."""
import numpy as np
import pytest

from deepcgp_amd import augment
import dilation_ref as dr
import padding_ref as pr
import rng_ref as rr
import stack_specs as ss

N_DRAWS = 1 << 20
PAIRS = [(1, 1), (77, 2), ((5 << 32) | 3, 65)]


def test_words_are_the_augmentation_mirrors_philox():
    """rng_ref.philox_words against deepcgp_amd.augment.philox4x32_10 (held to Random123's known-answer vectors in tests/test_host_augment.py)
    on random counters and keys, idx and seed with their high halves set among them."""
    rng = np.random.default_rng(0)
    idx = np.concatenate([np.arange(64, dtype=np.uint64), rng.integers(0, 1 << 63, 4096, dtype=np.uint64) * np.uint64(2) + np.uint64(1)])
    assert (idx >> np.uint64(32)).max() > 0
    for seed in [0, 1, 77, (9 << 32) | 5, 0xFFFFFFFFFFFFFFFF] + [int(s) for s in rng.integers(0, 1 << 63, 4, dtype=np.uint64)]:
        for stream in (0, 1, 65, 0xFFFFFFFF):
            got = rr.philox_words(seed, stream, idx)
            want = augment.philox4x32_10(seed, idx & np.uint64(0xFFFFFFFF), idx >> np.uint64(32), stream, rr.TAG)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (seed, stream)
    a, b = rr.philox_words(5, 1, idx), rr.philox_words((9 << 32) | 5, 1, idx)       # the key's high half is read
    assert not np.array_equal(a[0], b[0])


def test_cosine_is_reduced_exactly():
    k = np.array([0, 1 << 30, 1 << 31, 3 << 30, 1 << 32, 5 << 30, 3 << 31, 7 << 30, (1 << 33) - 1, 1, (1 << 31) + 1], np.int64)
    got = rr.cospi_dyadic(k)
    r = np.sqrt(0.5)
    assert np.array_equal(got[[0, 2, 4, 6]], [1.0, 0.0, -1.0, 0.0])                 # the zeros are exact zeros, as cospi's are
    assert np.allclose(got[[1, 3, 5, 7]], [r, -r, -r, r], rtol=0, atol=2.3e-16)
    kk = np.random.default_rng(1).integers(0, 1 << 33, 100000).astype(np.int64) | 1
    assert np.max(np.abs(rr.cospi_dyadic(kk) - np.cos(np.pi * (kk / 4294967296.0)))) < 2e-15     # libm on the rounded argument: |x| < 2 pi
    assert abs(got[10] + np.sin(np.pi / 4294967296.0)) < 1e-24 and got[10] < 0      # next to a zero: relative, not absolute, accuracy


@pytest.fixture(scope="module")
def draws():
    idx = np.arange(N_DRAWS, dtype=np.uint64)
    return {p: rr.philox_normal(p[0], p[1], idx) for p in PAIRS + [(1, 2), (2, 1), (1 | (1 << 32), 1)]}


@pytest.mark.parametrize("pair", PAIRS, ids=["seed1-stream1", "seed77-stream2", "seed-high-stream65"])
def test_reference_draws_are_standard_normal(draws, pair):
    from scipy import stats
    z, n = draws[pair], float(N_DRAWS)
    assert np.all(np.isfinite(z))
    for k, want, se in [(1, 0.0, 1.0 / np.sqrt(n)), (2, 1.0, np.sqrt(2.0 / n)), (3, 0.0, np.sqrt(15.0 / n)), (4, 3.0, np.sqrt(96.0 / n))]:
        m = np.mean(z ** k)
        print("%r moment %d: %.6f, %.2f standard errors from %.0f" % (pair, k, m, (m - want) / se, want))
        assert abs(m - want) <= 4.0 * se, (pair, k, m)
    p = stats.kstest(z, "norm").pvalue
    print("%r KS p %.3f" % (pair, p))
    assert p >= 0.01, (pair, p)


def test_streams_seeds_and_neighbours_are_uncorrelated(draws):
    bound = 4.0 / np.sqrt(N_DRAWS)
    z = draws[(1, 1)]
    for what, a, b in [("stream 1 | stream 2", z, draws[(1, 2)]), ("seed 1 | seed 2", z, draws[(2, 1)]),
                       ("seed 1 | seed 1 + 2^32", z, draws[(1 | (1 << 32), 1)]), ("lag 1", z[:-1], z[1:])]:
        c = np.corrcoef(a, b)[0, 1]
        print("%-24s correlation %.2f / sqrt n" % (what, c * np.sqrt(N_DRAWS)))
        assert abs(c) <= bound, (what, c)


def test_counters_are_disjoint_across_layers_ranks_and_the_augmentation():
    """No two elements of a step share (stream, idx): not two layers (res3's run over the same idx range), not two ranks, not two replicas of a
    de-duplicated first layer; and word 3 keeps every one of them off the augmentation's draws."""
    assert rr.TAG != augment.AUG_TAG
    spec, _, _, _ = pr.make_stack("res3")
    N, S, seen = 3, 2, set()
    for rank in range(4):
        for li, (stream, idx) in enumerate(rr.layer_counters(spec, N, S, rank=rank)):
            assert stream == li + 1 + 64 * rank and stream not in seen and li < 63
            seen.add(stream)
            assert np.unique(idx).size == idx.size == S * N * ss.output_dims(spec)[li][0]
            assert np.array_equal(idx.reshape(-1), np.arange(idx.size, dtype=np.uint64))      # the element's offset in [S, N, P G]
    zs = rr.device_noise(spec, N, S, 5)
    assert zs[-1] is None and [z.shape for z in zs[:-1]] == [(S, N, d) for d, _ in ss.output_dims(spec)[:-1]]
    assert not np.array_equal(zs[0][0], zs[0][1])                                   # the replicas of an image draw their own noise
    assert not np.array_equal(zs[0].reshape(-1)[:zs[1].size], zs[1].reshape(-1))    # two layers at the same idx
    assert not np.array_equal(zs[0], rr.device_noise(spec, N, S, 5, rank=1)[0])
    with_shard = rr.layer_counters(spec, N, S, rank=2, shard=(0, N))                # a declared shard: one stream per layer on every rank
    assert [s for s, _ in with_shard] == [1, 2]


@pytest.mark.parametrize("world", [2, 3])
def test_shards_concatenate_to_the_unsharded_noise(world):
    from deepcgp_amd.dist import shard_range
    spec, _, _, _ = pr.make_stack("res3")
    Ng, S, seed = 7, 3, (9 << 32) | 5
    full = rr.device_noise(spec, Ng, S, seed)
    parts = []
    for r in range(world):
        lo, hi = shard_range(Ng, r, world)
        parts.append(rr.device_noise(spec, hi - lo, S, seed, rank=r, shard=(lo, Ng)))
    for li in range(len(spec["convs"])):
        assert np.array_equal(np.concatenate([p[li] for p in parts], axis=1), full[li]), li
    assert all(p[-1] is None for p in parts)


def test_dilated_layer_draws_in_phase_layout_and_drops_the_phantoms():
    """dil2_odd: 9 x 7 x 3 under f3 d2 gives a 5 x 3 output, whose phases are 3 x 2 sub-images with phantom positions in both axes.  Element
    (oh, ow) of phase (oh % d, ow % d) sits at (oh // d, ow // d) of its sub-image; the counters not used are exactly the phantoms'."""
    spec, _, _, _ = dr.make_stack("dil2_odd")
    N, S = 3, 2
    (stream, idx), = rr.layer_counters(spec, N, S)
    ho, wo, G, d = rr.layer_geometry(spec["convs"][0])
    assert (ho, wo, G, d) == (5, 3, 2, 2) and stream == 1
    hs, ws = 3, 2
    idx5 = idx.reshape(S, N, ho, wo, G).astype(np.int64)
    used = set()
    for s in range(S):
        for n in range(N):
            for oh in range(ho):
                for ow in range(wo):
                    for g in range(G):
                        o = (((s * N + n) * d * d + (oh % d) * d + ow % d) * hs * ws + (oh // d) * ws + ow // d) * G + g
                        assert idx5[s, n, oh, ow, g] == o
                        used.add(o)
    phantoms = set()
    for row in range(S * N):
        for a in range(d):
            for b in range(d):
                for i in range(hs):
                    for j in range(ws):
                        if a + d * i >= ho or b + d * j >= wo:
                            phantoms.update((((row * d + a) * d + b) * hs * ws + i * ws + j) * G + g for g in range(G))
    assert len(phantoms) == S * N * (d * d * hs * ws - ho * wo) * G > 0
    assert used | phantoms == set(range(S * N * d * d * hs * ws * G)) and not used & phantoms
    z = rr.device_noise(spec, N, S, 77)[0]
    assert np.array_equal(z, rr.philox_normal(77, 1, idx))

"""Test helper for the device-drawn layer noise (tests/test_host_rng.py, tests/test_gpu_rng.py): csrc/rng.h's ``philox_normal`` in NumPy, and
the counter every output element of a model draws at, as the library implements it today.

The generator.  Philox4x32-10 under the key (seed lo, seed hi) on the counter (idx lo, idx hi, stream, 0x5eed5eed); of the four output words

    u1 = ((w0 << 21 ^ w1 >> 11) + 1) / 2^53         in (0, 1]
    u2 = (w2 + 0.5) / 2^32                          in (0, 1)
    z  = sqrt(-2 ln u1) cos(2 pi u2)

The device evaluates the cosine with ``cospi(2 u2)``.  2 u2 = (2 w2 + 1) / 2^32 is an exact dyadic number, so the mirror takes off the nearest
multiple of 1/2 in integers and calls np.cos / np.sin on pi t with |t| <= 1/4: no argument reduction of a rounded 2 pi u2 is left to libm.

The counter map, read from model.hip (``run_layer``, ``run_dilated_layer``), layer_impl.h (``conv_forward``) and the two kernels that draw
(conv_fused.hip phase 4, cond.hip ``finalize_kernel``: both ``o = s * rep_stride + (col0 + j) * R + r``).  Conv layer li of a model, N images (of
this rank), S samples, P patches per image, G latent GPs (the layer's GP count -- of a mixed layer NOT the Rout maps it emits), Wd = P G:

    what                          value
    key                           the step's seed (``evaluate``: seed + batch number), both halves
    counter word 3                0x5eed5eed (the augmentation draws carry DCGP_AUG_TAG there)
    counter word 2, the stream    li + 1 + 64 * rank; with a shard declared (``set_shard(lo, Ng)``): li + 1 on every rank
    counter words 0, 1, the idx   o = (s * N + n) * Wd + p * G + g: the element's offset in the layer's [S, N, P, G] noise table, whether the
                                  first layer is tiled (S N rows) or de-duplicated (S replicas, rep_stride = N Wd), and whichever chunk of the
                                  sweep + GEMM route writes it (col0 is the chunk's first column of the whole batch)
    ... with a shard (lo, Ng)     (s * Ng + lo + n) * Wd + p * G + g: the same element's offset in the un-sharded batch (``rng_index``)
    ... a dilated layer (d > 1)   the layer runs on N d^2 phase sub-images of P' patches, phantoms included, and draws in that layout:
                                  o = ((s * N + n) * d^2 + a * d + b) * P' G + p' * G + g for phase (a, b); batch-to-space (dilation_ref.b2s)
                                  brings the draws into image order and drops the phantom positions.  (A sharded model takes no dilated layer.)
    the head                      draws nothing (its entry of ``zs`` is None)

Layers (fewer than 64) and ranks therefore never share a stream, and ``device_noise`` returns per layer what the explicit-noise API takes:
image order, [S, N, P G].  Test infrastructure only."""
import numpy as np

import dilation_ref as dr
import stack_specs as ss

TAG = 0x5eed5eed
_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox_words(seed, stream, idx):
    """The four output words (uint64 arrays of 32-bit values) of the counter (idx lo, idx hi, stream, TAG) under ``seed``."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    idx = np.asarray(idx, np.uint64)
    c = [idx & _MASK, idx >> np.uint64(32), np.full(idx.shape, int(stream) & 0xFFFFFFFF, np.uint64), np.full(idx.shape, TAG, np.uint64)]
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]          # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return tuple(c)


def cospi_dyadic(k):
    """cos(pi k / 2^32) for integers 0 <= k < 2^34 (int64 array): k / 2^32 = n / 2 + t with |t| <= 1/4, both exact."""
    k = np.asarray(k, np.int64)
    n = (k + (1 << 30)) >> 31                                  # nearest multiple of 1/2, in halves
    t = (k - (n << 31)).astype(np.float64) / 4294967296.0      # |k - n 2^31| <= 2^30: exact
    c, s = np.cos(np.pi * t), np.sin(np.pi * t)
    return np.choose(n & 3, [c, -s, -c, s])


def philox_normal(seed, stream, idx):
    """rng.h's philox_normal, vectorised over ``idx`` (any shape, values below 2^64)."""
    w0, w1, w2, _ = philox_words(seed, stream, idx)
    bits = (w0 << np.uint64(21)) ^ (w1 >> np.uint64(11))        # < 2^53
    u1 = (bits.astype(np.float64) + 1.0) * (1.0 / 9007199254740992.0)
    return np.sqrt(-2.0 * np.log(u1)) * cospi_dyadic(2 * w2.astype(np.int64) + 1)


def layer_geometry(c):
    """(Ho, Wo, G, d) of a conv entry of a spec: its output image, latent GP count and dilation."""
    ho, wo = ss.out_size(c["H"], c["W"], c["f"], c["s"], c.get("pad", 0), c.get("dil", 1))
    return ho, wo, int(c["R"]), int(c.get("dil", 1))


def layer_counters(spec, N, S, rank=0, shard=None):
    """[(stream, idx)] per conv layer: idx a uint64 array [S, N, P G] in image order, the counter words 0, 1 of every element (module docstring).
    ``shard`` = (lo, Ng): the N images are [lo, lo + N) of a declared global batch of Ng."""
    out = []
    for li, c in enumerate(spec["convs"]):
        ho, wo, G, d = layer_geometry(c)
        if d > 1:
            assert shard is None, "a sharded model takes no dilated layer"
            hs, ws = -(-ho // d), -(-wo // d)                  # the sub-images' VALID output: ceil((H + 2 pad) / d) - f + 1
            sub = np.arange(S * N * d * d * hs * ws * G, dtype=np.float64).reshape(S * N * d * d, hs, ws, G)     # < 2^53: exact in a double
            idx = dr.b2s(sub, d, ho, wo).reshape(S, N, ho * wo * G).astype(np.uint64)
            out.append((li + 1 + 64 * rank, idx))
            continue
        Wd = ho * wo * G
        lo, Ng = (0, N) if shard is None else shard
        assert 0 <= lo and lo + N <= Ng, (lo, N, Ng)
        s = np.arange(S, dtype=np.int64)[:, None, None]
        n = np.arange(N, dtype=np.int64)[None, :, None]
        w = np.arange(Wd, dtype=np.int64)[None, None, :]
        idx = ((s * Ng + lo + n) * Wd + w).astype(np.uint64)
        out.append((li + 1 + (0 if shard is not None else 64 * rank), idx))
    return out


def device_noise(spec, N, S, seed, rank=0, shard=None):
    """The noise a model of ``spec`` draws under ``seed``: per layer [S, N, P * (the layer's GPs)] in image order, the head None."""
    return [philox_normal(seed, stream, idx) for stream, idx in layer_counters(spec, N, S, rank, shard)] + [None]

"""Training-time augmentation, the host mirror in NumPy of csrc/augment_map.h: a random shift by (dy, dx) in [-t, t]^2 with zero fill ("pad by
t and random-crop") and a random horizontal flip per image.

    F[y][x][c]   = I[y][W - 1 - x if flip else x][c]
    out[y][x][c] = F[y - dy][x - dx][c]  where 0 <= y - dy < H and 0 <= x - dx < W,  0.0 everywhere else

The device draws (dy, dx, flip) itself (dcgp_model_set_augmentation, dcgp_augment_images): Philox4x32-10 under the step's seed at counter
(position, stream word, tag word); ``draw`` is the same arithmetic, so ``apply(X, *draw(seed, len(X), t, hflip))`` is what the device writes,
to the bit -- the transform only moves values.  Nothing here touches the device."""
import numpy as np

AUG_STREAM, AUG_TAG = 0x0a095eed, 0xa0951f7b        # counter words 2 and 3 (csrc/augment_map.h); the layers' noise has 0x5eed5eed in word 3
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW, _32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(seed, c0, c1, c2, c3):
    """The four output words (uint64 arrays holding 32-bit values) of Philox4x32-10 with key ``seed`` (its low and high half) on the
    counters (c0, c1, c2, c3), arrays or scalars of 32-bit values; the high halves of the products are taken through uint64 products."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, np.uint64) for c in (c0, c1, c2, c3)])
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2             # < 2^64: both factors are below 2^32
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ np.uint64(k0), p1 & _LOW, (p0 >> _32) ^ c3 ^ np.uint64(k1), p0 & _LOW
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def draw(seed, n, max_shift, hflip):
    """(dy, dx, flip), int64 arrays of length n: the draws of batch positions 0 .. n - 1 under ``seed``.  dy, dx = a word modulo
    2 max_shift + 1, minus max_shift (modulo bias about (2 max_shift + 1) / 2^32); flip = the lowest bit of a third word, 0 without hflip."""
    t = int(max_shift)
    if t < 0:
        raise ValueError("max_shift must be >= 0, got %d" % t)
    pos = np.arange(int(n), dtype=np.uint64)
    w0, w1, w2, _ = philox4x32_10(seed, pos & _LOW, pos >> _32, AUG_STREAM, AUG_TAG)
    span = np.uint64(2 * t + 1)
    dy = (w0 % span).astype(np.int64) - t
    dx = (w1 % span).astype(np.int64) - t
    flip = (w2 & np.uint64(1)).astype(np.int64) if hflip else np.zeros(int(n), np.int64)
    return dy, dx, flip


def apply(X_nhwc, dy, dx, flip):
    """The transform on a batch [N, H, W, C] with one (dy, dx, flip) per image; a new array of X's shape and dtype."""
    X = np.asarray(X_nhwc)
    if X.ndim != 4:
        raise ValueError("apply: images must be [N, H, W, C], got %r" % (X.shape,))
    N, H, W, _ = X.shape
    dy, dx, flip = (np.broadcast_to(np.asarray(a), (N,)) for a in (dy, dx, flip))
    out = np.zeros_like(X)
    for b in range(N):
        F = X[b, :, ::-1] if flip[b] else X[b]
        y, x = int(dy[b]), int(dx[b])
        if abs(y) >= H or abs(x) >= W:
            continue
        out[b, max(y, 0):H + min(y, 0), max(x, 0):W + min(x, 0)] = F[max(-y, 0):H + min(-y, 0), max(-x, 0):W + min(-x, 0)]
    return out


class Augmentation(object):
    """What to do to every training image: a shift of up to ``max_shift`` pixels either way along both axes, and a horizontal flip with
    probability one half when ``hflip``.  False when it does nothing."""

    def __init__(self, max_shift=0, hflip=False):
        self.max_shift, self.hflip = int(max_shift), bool(hflip)
        if self.max_shift < 0:
            raise ValueError("Augmentation: max_shift must be >= 0, got %d" % self.max_shift)

    def __bool__(self):
        return self.max_shift > 0 or self.hflip

    def __repr__(self):
        return "Augmentation(max_shift=%d, hflip=%r)" % (self.max_shift, self.hflip)

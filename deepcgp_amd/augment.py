"""Augmentation, the host mirror in NumPy of csrc/augment_map.h: a random shift by (dy, dx) in [-t, t]^2 with zero fill ("pad by
t and random-crop") and a random horizontal flip per image.

    F[y][x][c]   = I[y][W - 1 - x if flip else x][c]
    out[y][x][c] = F[y - dy][x - dx][c]  where 0 <= y - dy < H and 0 <= x - dx < W,  0.0 everywhere else

The device draws (dy, dx, flip) itself (dcgp_model_set_augmentation, dcgp_augment_images): Philox4x32-10 under the step's seed at counter
(position, stream word, tag word); ``draw`` is the same arithmetic, so ``apply(X, *draw(seed, len(X), t, hflip))`` is what the device writes,
to the bit -- the transform only moves values.

Test-time augmentation uses the same transform with a fixed table in place of the draw: ``views`` lists (dy, dx, flip) triples, ``apply_views``
is the mirror of the device's view gather (dcgp_view_images, and inside ``DGP_Base.evaluate(views=...)``).  Nothing here touches the device."""
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


VIEW_PATTERNS = ("cross", "grid")


def views(max_shift=0, hflip=False, pattern="cross"):
    """The views of test-time augmentation, an int32 array [V, 3] of (dy, dx, flip): the identity first, no duplicates.  ``pattern`` "cross":
    (0, 0), (+-t, 0), (0, +-t) with t = ``max_shift`` -- 5 views; "grid": all (2t + 1)^2 shifts of [-t, t]^2.  ``hflip`` doubles the list: the
    unflipped views first, then the same shifts of the mirrored image.  t = 0 without ``hflip`` is [(0, 0, 0)], which evaluates as no views do."""
    t = int(max_shift)
    if t < 0:
        raise ValueError("views: max_shift must be >= 0, got %d" % t)
    if pattern not in VIEW_PATTERNS:
        raise ValueError("views: pattern must be one of %s, got %r" % (" | ".join(VIEW_PATTERNS), pattern))
    if pattern == "cross":
        shifts = [(0, 0), (-t, 0), (t, 0), (0, -t), (0, t)]
    else:
        shifts = [(0, 0)] + [(dy, dx) for dy in range(-t, t + 1) for dx in range(-t, t + 1)]
    seen, out = set(), []
    for s in shifts:
        if s not in seen:
            seen.add(s)
            out.append(s)
    rows = [(dy, dx, f) for f in ((0, 1) if hflip else (0,)) for dy, dx in out]
    return np.array(rows, np.int32).reshape(-1, 3)


def check_views(views, H, W, per_axis=False):
    """``views`` as an int32 array [V, 3], checked against H x W images: V >= 1, integer entries, |dy| and |dx| < min(H, W), flip in {0, 1}.
    ValueError otherwise -- the checks of dcgp_model_set_eval_views, made before anything reaches the device.  ``per_axis``: the bound of the
    gather alone (dcgp_view_images, ``apply_views``), |dy| < H and |dx| < W -- a view may keep a single row or column."""
    a = np.asarray(views)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("views: expected an array [V, 3] of (dy, dx, flip), got shape %r" % (a.shape,))
    if a.shape[0] == 0:
        raise ValueError("views: the list is empty (pass views=None for none)")
    if a.dtype.kind not in "iu":
        if a.dtype.kind != "f" or not np.all(a == np.round(a)):
            raise ValueError("views: entries must be integers")
    a = a.astype(np.int64)
    m = min(int(H), int(W))
    if per_axis:
        if np.any(np.abs(a[:, 0]) >= int(H)) or np.any(np.abs(a[:, 1]) >= int(W)):
            raise ValueError("views: |dy| must be < H and |dx| < W of the %d x %d images: a larger shift leaves no pixel" % (H, W))
    elif np.any(np.abs(a[:, :2]) >= m):
        raise ValueError("views: |dy| and |dx| must be < min(H, W) = %d of the %d x %d images" % (m, H, W))
    if np.any((a[:, 2] != 0) & (a[:, 2] != 1)):
        raise ValueError("views: flip must be 0 or 1")
    return np.ascontiguousarray(a, np.int32)


def apply_views(X_nhwc, views):
    """The views of a batch [N, H, W, C]: [V * N, H, W, C], view-major -- view v of image i at row v * N + i, ``apply`` per view.  What
    dcgp_view_images writes, to the bit.  A shift may go up to H - 1 rows and W - 1 columns (an evaluation's views: below min(H, W))."""
    X = np.asarray(X_nhwc)
    if X.ndim != 4:
        raise ValueError("apply_views: images must be [N, H, W, C], got %r" % (X.shape,))
    v = check_views(views, X.shape[1], X.shape[2], per_axis=True)
    return np.concatenate([apply(X, int(dy), int(dx), int(f)) for dy, dx, f in v], axis=0)


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

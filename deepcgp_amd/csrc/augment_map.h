// augment_map.h -- training-time augmentation of an image [H][W][C]: a random translation by (dy, dx) in [-t, t]^2 with zero fill ("pad by t and
// random-crop") and a random horizontal flip.  With F[y][x][c] = I[y][flip ? W - 1 - x : x][c]:
//     out[y][x][c] = F[y - dy][x - dx][c]   where 0 <= y - dy < H and 0 <= x - dx < W,   0.0 everywhere else.
// Host and device: augment.hip's two kernels are this draw, this map and a copy; tests/augment_map_check.cc walks both on the CPU against
// deepcgp_amd/augment.py (the NumPy mirror) and an independent np.flip / np.pad / slice formulation.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DCGP_AUG_HD __host__ __device__
#else
#define DCGP_AUG_HD
#endif

// Counter words 2 and 3 of an augmentation draw.  rng.h's philox_normal puts 0x5eed5eed into word 3 of every counter it forms, whatever its
// stream id: a counter whose word 3 differs can never be one of its, under any key.
#define DCGP_AUG_STREAM 0x0a095eedu
#define DCGP_AUG_TAG 0xa0951f7bu

// Philox4x32-10, the raw output words: key = the two halves of seed, the rounds and key schedule of rng.h's philox_normal.  Plain C++ (the high
// halves of the products through 64-bit products), so that the host compiles it as it stands.
DCGP_AUG_HD inline void philox4x32_10(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct AugmentDraw {
  int dy, dx, flip;
};

// The draw of batch position `position` under `seed` (a step's seed: seed0 + step).  t = max_shift >= 0.  dy and dx are a word modulo 2t + 1:
// the values below 2^32 mod (2t + 1) are more likely than the others by 1 part in 2^32 / (2t + 1) -- a bias of about (2t + 1) / 2^32, accepted.
DCGP_AUG_HD inline AugmentDraw augment_draw(uint64_t seed, uint64_t position, int t, int hflip) {
  uint32_t w[4];
  philox4x32_10(seed, (uint32_t)position, (uint32_t)(position >> 32), DCGP_AUG_STREAM, DCGP_AUG_TAG, w);
  const uint32_t span = 2u * (uint32_t)t + 1u;
  AugmentDraw d;
  d.dy = (int)(w[0] % span) - t;
  d.dx = (int)(w[1] % span) - t;
  d.flip = hflip ? (int)(w[2] & 1u) : 0;
  return d;
}

// One image row: offset j in [0, W C) of a destination row -> offset in the source row, or -1 for fill.  An unflipped row is a contiguous
// copy shifted by dx C values; a flipped row reverses the pixels and keeps the C channels of a pixel in order.
DCGP_AUG_HD inline int augment_source_in_row(int j, int W, int C, int dx, int flip) {
  if (!flip) {
    const int s = j - dx * C;
    return (s < 0 || s >= W * C) ? -1 : s;
  }
  const int x = j / C, c = j - x * C, sx = x - dx;
  if (sx < 0 || sx >= W) return -1;
  return (W - 1 - sx) * C + c;
}

// linear index into the destination image [H][W][C] -> linear index into the source image, or -1 for fill
DCGP_AUG_HD inline long augment_source_index(long i, int H, int W, int C, int dy, int dx, int flip) {
  const int WC = W * C;
  const int y = (int)(i / WC), j = (int)(i - (long)y * WC), sy = y - dy;
  if (sy < 0 || sy >= H) return -1;
  const int s = augment_source_in_row(j, W, C, dx, flip);
  return s < 0 ? -1 : (long)sy * WC + s;
}

// ---- Deterministic views (test-time augmentation): a table views [V][3] of (dy, dx, flip) in place of the draw, the same map ----
// Destination row r of a view-major batch [V][n] images: view r / n of source image r % n (n >= 1, 0 <= r < V n).
struct ViewRow {
  int v, i;
};
DCGP_AUG_HD inline ViewRow view_row(long r, int n) {
  ViewRow q;
  q.v = (int)(r / n);
  q.i = (int)(r - (long)q.v * n);
  return q;
}

DCGP_AUG_HD inline AugmentDraw view_draw(const int32_t* views, int v) {
  AugmentDraw d;
  d.dy = views[3 * v]; d.dx = views[3 * v + 1]; d.flip = views[3 * v + 2];
  return d;
}

// nullptr, or what is wrong with a table of V views of H x W images (the geometry itself: augment_geometry_error).  per_axis (the gather on a
// caller's batch): |dy| < H and |dx| < W, a view keeps at least one row and one column of its image.  Otherwise (a model's evaluation): a shift
// of min(H, W) or more along either axis is refused whatever the axis -- the bound of the training-time shift.
inline const char* view_table_error(const int32_t* views, int V, int H, int W, bool per_axis) {
  const int m = H < W ? H : W, my = per_axis ? H : m, mx = per_axis ? W : m;
  for (int v = 0; v < V; ++v) {
    const int32_t dy = views[3 * v], dx = views[3 * v + 1], f = views[3 * v + 2];
    if (dy <= -my || dy >= my || dx <= -mx || dx >= mx)
      return per_axis ? "a view's |dy| must be < H and its |dx| < W: a larger shift leaves no pixel of the image" : "a view's |dy| and |dx| must be < min(H, W)";
    if (f != 0 && f != 1) return "a view's flip must be 0 or 1";
  }
  return nullptr;
}

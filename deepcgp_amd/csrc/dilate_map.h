// dilate_map.h -- the index map of space-to-batch with rate d: an image batch [rows][H][W][C] against its d^2 phase sub-images
// [rows d^2][Hs][Ws][C], Hs = ceil(H / d), Ws = ceil(W / d):  sub[(n d + a) d + b][i][j][c] = x[n][i d + a][j d + b][c], and fill where
// i d + a >= H or j d + b >= W.  A dilated stride-1 layer is an ordinary layer on those sub-images (dilate.hip).
// Host and device: dilate.hip's kernels are this map and a copy; tests/dilate_map_check.cc walks it exhaustively against NumPy slicing on the CPU.
#pragma once

#if defined(__HIPCC__)
#define DCGP_DIL_HD __host__ __device__
#else
#define DCGP_DIL_HD
#endif

DCGP_DIL_HD inline long dilate_ceil_div(long a, long d) { return (a + d - 1) / d; }

// linear index into the phase batch -> linear index into the image batch, or -1 on the fill
DCGP_DIL_HD inline long s2b_source_index(long i, int H, int W, int C, int d) {
  const long Hs = dilate_ceil_div(H, d), Ws = dilate_ceil_div(W, d);
  const long c = i % C;
  long t = i / C;
  const long j = t % Ws;
  t /= Ws;
  const long k = t % Hs;
  t /= Hs;
  const long b = t % d;
  t /= d;
  const long a = t % d, n = t / d;
  const long y = k * d + a, x = j * d + b;
  if (y >= H || x >= W) return -1;
  return ((n * H + y) * W + x) * C + c;
}

// the inverse: linear index into the image batch -> linear index of the same pixel in the phase batch (never a fill entry)
DCGP_DIL_HD inline long s2b_phase_index(long j, int H, int W, int C, int d) {
  const long Hs = dilate_ceil_div(H, d), Ws = dilate_ceil_div(W, d);
  const long c = j % C;
  long t = j / C;
  const long x = t % W;
  t /= W;
  const long y = t % H, n = t / H;
  return ((((n * d + y % d) * d + x % d) * Hs + y / d) * Ws + x / d) * C + c;
}

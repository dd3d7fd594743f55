// pad_map.h -- the index map of symmetric zero padding: an image batch [rows][H][W][C] inside its padded copy [rows][H + 2p][W + 2p][C].
// Host and device: pad.hip's two kernels are this map and a copy; tests/pad_map_check.cc walks it exhaustively against np.pad on the CPU.
#pragma once

#if defined(__HIPCC__)
#define DCGP_PAD_HD __host__ __device__
#else
#define DCGP_PAD_HD
#endif

// linear index into the padded batch -> linear index into the source batch, or -1 on the zero border
DCGP_PAD_HD inline long pad_source_index(long i, int H, int W, int C, int p) {
  const long Hp = (long)H + 2L * p, Wp = (long)W + 2L * p;
  const long c = i % C;
  long t = i / C;
  const long x = t % Wp - p;
  t /= Wp;
  const long y = t % Hp - p, r = t / Hp;
  if (y < 0 || y >= H || x < 0 || x >= W) return -1;
  return ((r * H + y) * W + x) * C + c;
}

// the adjoint's direction: linear index into the source batch -> linear index of the same pixel in the padded batch
DCGP_PAD_HD inline long pad_padded_index(long j, int H, int W, int C, int p) {
  const long Hp = (long)H + 2L * p, Wp = (long)W + 2L * p;
  const long c = j % C;
  long t = j / C;
  const long x = t % W;
  t /= W;
  const long y = t % H, r = t / H;
  return ((r * Hp + y + p) * Wp + x + p) * C + c;
}

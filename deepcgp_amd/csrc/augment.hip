// augment.hip -- training-time augmentation on the device: a random shift with zero fill and a random horizontal flip per image, drawn on the
// device from the step's seed (augment_map.h holds the draw and the index map, host and device).  Two kernels, both "the map and a copy":
// the augmenting sibling of train_run.hip's gather (dcgp_model_set_augmentation switches a run over to it) and the stand-alone form on a
// caller's batch (dcgp_augment_images), which the per-step optimisers and the tests use.  Pure data movement: every output value is an input
// value or 0.0, so both are exact.
#include "model_state.h"
#include "augment_map.h"

namespace {

// dst [H][W][C] <- the augmented src, by one workgroup of four waves: a wave takes every fourth image row, its lanes walk consecutive doubles of
// the destination row (W C of them), and every value of the destination is written -- fill included, the batch buffer is reused.  No division
// on an unflipped row, a 32-bit one per value on a flipped row.
__device__ __forceinline__ void augment_image(const double* __restrict__ src, double* __restrict__ dst, int H, int W, int C, AugmentDraw d) {
  const int WC = W * C, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int y = wave; y < H; y += 4) {
    double* drow = dst + (long)y * WC;
    const int sy = y - d.dy;
    if (sy < 0 || sy >= H) {
      for (int j = lane; j < WC; j += 64) drow[j] = 0.0;
      continue;
    }
    const double* srow = src + (long)sy * WC;
    for (int j = lane; j < WC; j += 64) {
      const int s = augment_source_in_row(j, W, C, d.dx, d.flip);
      drow[j] = s < 0 ? 0.0 : srow[s];
    }
  }
}

// gather_batch_kernel's sibling: row idx[b] of the resident set, augmented with the draw of (seed, b), into row b of the step's batch; the
// target is copied as there.  One workgroup per batch row, one draw per workgroup (uniform: every lane forms the same three values from the
// block index).  The host has checked 0 <= idx < n, H W C == the row length and 0 <= t < min(H, W).
__global__ __launch_bounds__(256) void gather_augment_batch_kernel(const double* __restrict__ X, const int32_t* __restrict__ idx, int batch, long n,
                                                                   double* __restrict__ Xb, const int32_t* __restrict__ y32,
                                                                   const double* __restrict__ yf, int D, int32_t* __restrict__ yb32,
                                                                   double* __restrict__ ybf, int H, int W, int C, int t, int hflip, uint64_t seed) {
  const int b = blockIdx.x;
  if (b >= batch) return;
  const long r = idx[b];
  if (r < 0 || r >= n) return;
  const long len = (long)H * W * C;
  augment_image(X + r * len, Xb + (long)b * len, H, W, C, augment_draw(seed, (uint64_t)b, t, hflip));
  if (D == 0) {
    if (threadIdx.x == 0) yb32[b] = y32[r];
  } else {
    for (int j = threadIdx.x; j < D; j += 256) ybf[(long)b * D + j] = yf[r * D + j];
  }
}

// out [N][H][W][C] <- X with image b augmented by the draw of (seed, b)
__global__ __launch_bounds__(256) void augment_images_kernel(const double* __restrict__ X, int N, int H, int W, int C, int t, int hflip, uint64_t seed,
                                                             double* __restrict__ out) {
  const int b = blockIdx.x;
  if (b >= N) return;
  const long len = (long)H * W * C;
  augment_image(X + (long)b * len, out + (long)b * len, H, W, C, augment_draw(seed, (uint64_t)b, t, hflip));
}

}  // namespace

// what both entry points ask of a geometry: nullptr, or what is wrong with it
const char* augment_geometry_error(int H, int W, int C, int max_shift) {
  if (H < 1 || W < 1 || C < 1) return "H, W and C must be >= 1";
  if ((long)H * W * C > 0x7fffffffL) return "an image of more than 2^31 - 1 values";
  if (max_shift < 0) return "max_shift must be >= 0";
  if (max_shift >= (H < W ? H : W)) return "max_shift must be < min(H, W): a larger shift can leave no pixel of the image";
  return nullptr;
}

int gather_augment_batch(dcgp_model* model, const int32_t* idx_dev, int batch, uint64_t seed, const int32_t* y32, const double* yf, int D,
                         int32_t* yb32, double* ybf) {
  dcgp_ctx* ctx = model->ctx;
  hipLaunchKernelGGL(gather_augment_batch_kernel, dim3(batch), dim3(256), 0, ctx->stream, model->ds_X, idx_dev, batch, model->ds_n, model->run_X, y32,
                     yf, D, yb32, ybf, model->aug_H, model->aug_W, model->aug_C, model->aug_shift, model->aug_hflip, seed);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

extern "C" int dcgp_augment_images(dcgp_ctx* ctx, const double* X, int N, int H, int W, int C, int max_shift, int hflip, uint64_t seed, double* out) {
  if (!ctx) return DCGP_ERR_ARG;
  if (N < 0 || (N > 0 && (!X || !out))) return ctx_fail(ctx, DCGP_ERR_ARG, "augment_images: bad args");
  if (const char* why = augment_geometry_error(H, W, C, max_shift)) return ctx_fail(ctx, DCGP_ERR_ARG, "augment_images: %s (H %d W %d C %d max_shift %d)", why, H, W, C, max_shift);
  if (N == 0) return DCGP_OK;
  const long total = (long)N * H * W * C;
  if (X < out + total && out < X + total) return ctx_fail(ctx, DCGP_ERR_ARG, "augment_images: out may not alias X");
  hipLaunchKernelGGL(augment_images_kernel, dim3(N), dim3(256), 0, ctx->stream, X, N, H, W, C, max_shift, hflip != 0, seed, out);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

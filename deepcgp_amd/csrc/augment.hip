// augment.hip -- augmentation on the device.  Training time: a random shift with zero fill and a random horizontal flip per image, drawn on the
// device from the step's seed (augment_map.h holds the draw and the index map, host and device).  Two kernels, both "the map and a copy":
// the augmenting sibling of train_run.hip's gather (dcgp_model_set_augmentation switches a run over to it) and the stand-alone form on a
// caller's batch (dcgp_augment_images), which the per-step optimisers and the tests use.  Pure data movement: every output value is an input
// value or 0.0, so both are exact.  Test time (the end of the file): the same per-image map under a table of deterministic views, for the
// evaluation's batches (dcgp_model_set_eval_views; model.hip: eval_batches) and on a caller's batch (dcgp_view_images).
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

// out [V][n][H][W][C] <- view v of image i at row v n + i: the draw read from the table views [V][3] in place of augment_draw
__global__ __launch_bounds__(256) void view_images_kernel(const double* __restrict__ X, int n, int H, int W, int C, int V,
                                                          const int32_t* __restrict__ views, double* __restrict__ out) {
  const long r = blockIdx.x;
  if (r >= (long)V * n) return;
  const ViewRow q = view_row(r, n);
  const long len = (long)H * W * C;
  augment_image(X + (long)q.i * len, out + r * len, H, W, C, view_draw(views, q.v));
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

// ---- Test-time augmentation: V deterministic views of every image of an evaluation batch (model.hip: eval_batches) ----

namespace {
// the checks the two entry points share; V >= 1
int view_args_error(dcgp_ctx* ctx, const char* who, int H, int W, int C, int V, const int32_t* views_host, bool per_axis) {
  if (V < 1 || !views_host) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: bad args (V %d)", who, V);
  if (const char* why = augment_geometry_error(H, W, C, 0)) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: %s (H %d W %d C %d)", who, why, H, W, C);
  if (const char* why = view_table_error(views_host, V, H, W, per_axis)) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: %s (H %d W %d, %d views)", who, why, H, W, V);
  return DCGP_OK;
}
}  // namespace

int gather_eval_views(dcgp_model* model, const double* X, int n, double* out) {
  dcgp_ctx* ctx = model->ctx;
  const long rows = (long)model->eval_V * n;
  if (rows > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "evaluate: %d views of %d images are more than 2^31 - 1 rows", model->eval_V, n);
  hipLaunchKernelGGL(view_images_kernel, dim3((unsigned)rows), dim3(256), 0, ctx->stream, X, n, model->ev_H, model->ev_W, model->ev_C, model->eval_V,
                     model->d_eval_views, out);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

extern "C" int dcgp_view_images(dcgp_ctx* ctx, const double* X, int N, int H, int W, int C, int V, const int32_t* views_host, double* out) {
  if (!ctx) return DCGP_ERR_ARG;
  if (N < 0 || (N > 0 && (!X || !out))) return ctx_fail(ctx, DCGP_ERR_ARG, "view_images: bad args");
  DCGP_TRY(view_args_error(ctx, "view_images", H, W, C, V, views_host, true));
  if (N == 0) return DCGP_OK;
  const long rows = (long)V * N, len = (long)H * W * C;
  if (rows > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "view_images: %d views of %d images are more than 2^31 - 1 rows", V, N);
  if (X < out + rows * len && out < X + (long)N * len) return ctx_fail(ctx, DCGP_ERR_ARG, "view_images: out may not alias X");
  int32_t* table = (int32_t*)ws_get(ctx, "view_table", (size_t)V * 3 * sizeof(int32_t));
  if (!table) return DCGP_ERR_ALLOC;
  HIP_TRY(ctx, hipMemcpyAsync(table, views_host, (size_t)V * 3 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(view_images_kernel, dim3((unsigned)rows), dim3(256), 0, ctx->stream, X, N, H, W, C, V, table, out);
  LAUNCH_CHECK(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the table left the caller's memory)
  return DCGP_OK;
}

extern "C" int dcgp_model_set_eval_views(dcgp_model* model, int H, int W, int C, int V, const int32_t* views_host) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (model->enq_seq != model->col_seq) return ctx_fail(ctx, DCGP_ERR_ARG, "set_eval_views: enqueued steps are still to be collected");
  if (V == 0) {   // off: the geometry plays no part
    model->eval_views.clear();
    model->eval_V = model->ev_H = model->ev_W = model->ev_C = 0;
    return DCGP_OK;
  }
  if (!model->has_head || model->layers.empty()) return ctx_fail(ctx, DCGP_ERR_ARG, "set_eval_views: the model has no head layer yet");
  DCGP_TRY(view_args_error(ctx, "set_eval_views", H, W, C, V, views_host, false));
  const LayerState& L0 = *model->layers[0];
  if (model->layers.size() == 1 && (L0.in_scale || (L0.v.H == 1 && L0.v.W == 1)))
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_eval_views: a dense head alone takes feature vectors, not H x W x C images: it has no views");
  const int p = model->pad[0];
  const dcgp_model::Geom g0 = model->geom(0);   // (true size: a dilated first layer's v is its phase geometry)
  if (H != g0.H - 2 * p || W != g0.W - 2 * p || C != L0.v.C)
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_eval_views: %d x %d x %d is not the model's image of %d x %d x %d", H, W, C, g0.H - 2 * p, g0.W - 2 * p, L0.v.C);
  const size_t bytes = (size_t)V * 3 * sizeof(int32_t);
  if (bytes > model->eval_views_cap) {
    dev_free(ctx, model->d_eval_views);
    model->d_eval_views = nullptr; model->eval_views_cap = 0;
    if (dev_alloc(ctx, (void**)&model->d_eval_views, bytes, "eval_views") != hipSuccess) return ctx_fail(ctx, DCGP_ERR_ALLOC, "set_eval_views: allocation failed");
    model->eval_views_cap = bytes;
  }
  // (no evaluation is in flight: each one ends in a stream synchronisation)
  HIP_TRY(ctx, hipMemcpy(model->d_eval_views, views_host, bytes, hipMemcpyHostToDevice));
  model->eval_views.assign(views_host, views_host + 3 * (size_t)V);
  model->eval_V = V; model->ev_H = H; model->ev_W = W; model->ev_C = C;
  return DCGP_OK;
}

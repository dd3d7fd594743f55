// dilate.hip -- space-to-batch and batch-to-space for dilated conv layers (dcgp_model_set_dilation).  A stride-1 layer whose window taps sit d
// pixels apart is an ordinary VALID layer on the d^2 phase sub-images of its input: the sweeps, the fused layer kernel and every reverse kernel see
// an ordinary image.  Both kernels are one fp64 pass with the contiguous channel run innermost across lanes; the index map is dilate_map.h's.
// Each kernel walks its DESTINATION: s2b has to, it writes the fill of a reused workspace on every call; b2s walks the image so that a phantom
// entry (a patch that touched the fill) is never read.  The other side of each is strided by d C doubles.
#include "model_state.h"
#include "dilate_map.h"

namespace {

// dst [rows d^2][Hs][Ws][C] <- src [rows][H][W][C]; the fill is written on every call
__global__ void s2b_images_kernel(const double* __restrict__ src, long n_dst, int H, int W, int C, int d, double* __restrict__ dst) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_dst) return;
  const long j = s2b_source_index(i, H, W, C, d);
  dst[i] = j < 0 ? 0.0 : src[j];
}

// dst [rows][H][W][C] <- src [reps][rows d^2][Hs][Ws][C], summed over the reps replicas in the order 0, 1, ... (reps == 1: the plain inverse)
__global__ void b2s_images_kernel(const double* __restrict__ src, int reps, long n_dst, long rep_stride, int H, int W, int C, int d,
                                  double* __restrict__ dst) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_dst) return;
  const long i = s2b_phase_index(j, H, W, C, d);
  double acc = src[i];
  for (int r = 1; r < reps; ++r) acc += src[(long)r * rep_stride + i];
  dst[j] = acc;
}

// ---- the other way round, for dcgp_debug_dilate_time only: each kernel walking its SOURCE (coalesced reads, writes strided by d C doubles) ----
// s2b from the image's side cannot write the fill: a memset of the destination goes in front of it (two launches)
__global__ void s2b_scatter_kernel(const double* __restrict__ src, long n_src, int H, int W, int C, int d, double* __restrict__ dst) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_src) return;
  dst[s2b_phase_index(j, H, W, C, d)] = src[j];
}
__global__ void b2s_scatter_kernel(const double* __restrict__ src, long n_src, int H, int W, int C, int d, double* __restrict__ dst) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_src) return;
  const long j = s2b_source_index(i, H, W, C, d);
  if (j >= 0) dst[j] = src[i];
}
// the yardstick: n doubles read, n written
__global__ __launch_bounds__(256) void dilate_copy_kernel(const double* __restrict__ src, long n, double* __restrict__ dst) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

}  // namespace

int s2b_images(dcgp_ctx* ctx, hipStream_t stream, const double* src, long rows, int H, int W, int C, int d, double* dst) {
  const long n_dst = rows * d * d * dilate_ceil_div(H, d) * dilate_ceil_div(W, d) * C;
  if (n_dst <= 0) return DCGP_OK;
  if ((n_dst + 255) / 256 > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "dilate: %ld values exceed one launch", n_dst);
  hipLaunchKernelGGL(s2b_images_kernel, dim3((unsigned)((n_dst + 255) / 256)), dim3(256), 0, stream, src, n_dst, H, W, C, d, dst);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int b2s_images(dcgp_ctx* ctx, hipStream_t stream, const double* src, int reps, long rows, int H, int W, int C, int d, double* dst) {
  const long n_dst = rows * H * W * C;
  if (n_dst <= 0 || reps < 1) return DCGP_OK;
  if ((n_dst + 255) / 256 > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "dilate: %ld values exceed one launch", n_dst);
  const long rep_stride = rows * d * d * dilate_ceil_div(H, d) * dilate_ceil_div(W, d) * C;
  hipLaunchKernelGGL(b2s_images_kernel, dim3((unsigned)((n_dst + 255) / 256)), dim3(256), 0, stream, src, reps, n_dst, rep_stride, H, W, C, d, dst);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// Measurement aid (tools/dilation_time.py): the two relayout kernels alone on `rows` images H x W x C at rate d, each beside the same relayout
// walking its source instead of its destination (s2b: a memset of the destination plus the scatter) and beside a copy kernel of the same traffic.
// `iters` launches between two events behind a warm-up launch, on the ctx stream; out_us[8] = microseconds per launch {s2b_images, s2b from the
// image's side, a copy of the phase batch's size, b2s_images, b2s from the phase side, a copy of the image batch's size, 0, 0}.
extern "C" int dcgp_debug_dilate_time(dcgp_ctx* ctx, int rows, int H, int W, int C, int d, int iters, double* out_us) {
  if (!ctx || !out_us || rows <= 0 || H <= 0 || W <= 0 || C <= 0 || d < 1 || iters <= 0)
    return ctx ? ctx_fail(ctx, DCGP_ERR_ARG, "debug_dilate_time: bad args") : DCGP_ERR_ARG;
  const long n_img = (long)rows * H * W * C, n_ph = (long)rows * d * d * dilate_ceil_div(H, d) * dilate_ceil_div(W, d) * C;
  if ((n_ph + 255) / 256 > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "debug_dilate_time: shape exceeds one launch");
  double* img = (double*)ws_get(ctx, "dilate_time_img", (size_t)n_img * sizeof(double));
  double* ph = (double*)ws_get(ctx, "dilate_time_ph", (size_t)n_ph * sizeof(double));
  double* other = (double*)ws_get(ctx, "dilate_time_copy", (size_t)n_ph * sizeof(double));
  if (!img || !ph || !other) return DCGP_ERR_ALLOC;
  HIP_TRY(ctx, hipMemsetAsync(img, 0, (size_t)n_img * sizeof(double), ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(ph, 0, (size_t)n_ph * sizeof(double), ctx->stream));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(ctx, hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); return ctx_fail(ctx, DCGP_ERR_HIP, "debug_dilate_time: event creation failed"); }
  int rc = DCGP_OK;
  auto timed = [&](int slot, auto&& launch) {
    for (int i = -1; i < iters && rc == DCGP_OK; ++i) {   // i == -1: warm-up
      if (i == 0 && hipEventRecord(e0, ctx->stream) != hipSuccess) rc = DCGP_ERR_HIP;
      if (rc == DCGP_OK) rc = launch();
    }
    float ms = 0.f;
    if (rc == DCGP_OK && (hipEventRecord(e1, ctx->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
      rc = DCGP_ERR_HIP;
    out_us[slot] = 1e3 * (double)ms / iters;
  };
  auto ok = [] { return hipGetLastError() == hipSuccess ? DCGP_OK : DCGP_ERR_HIP; };
  const dim3 g_img((unsigned)((n_img + 255) / 256)), g_ph((unsigned)((n_ph + 255) / 256)), b(256);
  timed(0, [&] { return s2b_images(ctx, ctx->stream, img, rows, H, W, C, d, ph); });
  timed(1, [&] {
    if (hipMemsetAsync(ph, 0, (size_t)n_ph * sizeof(double), ctx->stream) != hipSuccess) return (int)DCGP_ERR_HIP;
    hipLaunchKernelGGL(s2b_scatter_kernel, g_img, b, 0, ctx->stream, img, n_img, H, W, C, d, ph);
    return ok();
  });
  timed(2, [&] { hipLaunchKernelGGL(dilate_copy_kernel, g_ph, b, 0, ctx->stream, ph, n_ph, other); return ok(); });
  timed(3, [&] { return b2s_images(ctx, ctx->stream, ph, 1, rows, H, W, C, d, img); });
  timed(4, [&] { hipLaunchKernelGGL(b2s_scatter_kernel, g_ph, b, 0, ctx->stream, ph, n_ph, H, W, C, d, img); return ok(); });
  timed(5, [&] { hipLaunchKernelGGL(dilate_copy_kernel, g_img, b, 0, ctx->stream, img, n_img, other); return ok(); });
  out_us[6] = out_us[7] = 0.0;
  hipStreamSynchronize(ctx->stream);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  if (rc != DCGP_OK) return ctx_fail(ctx, rc, "debug_dilate_time: a launch or an event failed");
  return DCGP_OK;
}

// pad.hip -- zero padding of a layer's input (dcgp_model_set_input_padding) and its adjoint.  A padded layer is a VALID layer on a physically
// padded copy of its input: the sweeps, the fused layer kernel, the head kernels and the reverse kernels see an ordinary image.  Both kernels are
// one coalesced fp64 pass over the larger of the two buffers' index range, the index map is pad_map.h's.
#include "model_state.h"
#include "pad_map.h"

namespace {

// dst [rows][H + 2p][W + 2p][C] <- src [rows][H][W][C]; the border is written on every call (the buffer is a reused workspace)
__global__ void pad_images_kernel(const double* __restrict__ src, long n_pad, int H, int W, int C, int p, double* __restrict__ dst) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pad) return;
  const long j = pad_source_index(i, H, W, C, p);
  dst[i] = j < 0 ? 0.0 : src[j];
}

// dst [rows][H][W][C] <- the interior of src [reps][rows][H + 2p][W + 2p][C], summed over the reps replicas in the order 0, 1, ...
// (reps == 1: the plain crop; reps == S: the replica sum of a tiled batch's input gradient in the same pass)
__global__ void crop_images_kernel(const double* __restrict__ src, int reps, long n_src, long rep_stride, int H, int W, int C, int p,
                                   double* __restrict__ dst) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_src) return;
  const long i = pad_padded_index(j, H, W, C, p);
  double acc = src[i];
  for (int r = 1; r < reps; ++r) acc += src[(long)r * rep_stride + i];
  dst[j] = acc;
}

}  // namespace

int pad_images(dcgp_ctx* ctx, hipStream_t stream, const double* src, long rows, int H, int W, int C, int p, double* dst) {
  const long n_pad = rows * (H + 2L * p) * (W + 2L * p) * C;
  if (n_pad <= 0) return DCGP_OK;
  if ((n_pad + 255) / 256 > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "pad: %ld values exceed one launch", n_pad);
  hipLaunchKernelGGL(pad_images_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, stream, src, n_pad, H, W, C, p, dst);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int crop_images(dcgp_ctx* ctx, hipStream_t stream, const double* src, int reps, long rows, int H, int W, int C, int p, double* dst) {
  const long n_src = rows * H * W * C;
  if (n_src <= 0 || reps < 1) return DCGP_OK;
  if ((n_src + 255) / 256 > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "pad: %ld values exceed one launch", n_src);
  const long rep_stride = rows * (H + 2L * p) * (W + 2L * p) * C;
  hipLaunchKernelGGL(crop_images_kernel, dim3((unsigned)((n_src + 255) / 256)), dim3(256), 0, stream, src, reps, n_src, rep_stride, H, W, C, p, dst);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

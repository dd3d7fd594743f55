// conv_mean.hip -- a general linear convolutional mean function of a conv layer (conv_gp/mean_functions.py:6-41 with any filter;
// added to the conditional's mean at conv_gp/layers.py:133-134):
//     m(x)[n, p, r] = sum_l patch_p(x_n)[l] W[l, r],   W [L][R], l = (kh f + kw) C + c  (FullView's element order)
// on the layer's own window (the same f, stride and -- through the padded copy the layer reads -- padding).  Three kernels:
//   conv_mean_add              behind the point where the layer's outputs exist (conv_forward, layer_impl.h): m into out_mean and out_sample
//   conv_mean_backward_dx      behind patches_to_dx (conv_backward, grad.hip): dX += the adjoint through the patches, a gather per input pixel
//   conv_mean_backward_filter  gW[l][r] = sum_j patch_j[l] gm[j][r] from the Xcol the reverse pass holds: split-k partial sums, then their sum
// Every output element has one writer and every sum a fixed order: no atomics, two runs give the same bits.
// Forward and dX are plain fp64 FMAs (the filter from LDS / as a wave-uniform operand); the filter's gradient is the reverse pass's matrix-core
// product.  A layer's mean is 2 L R flops per column against the 2 M (L + M R) of its conditional (DESIGN.md 4y has the figures).
#include "model_state.h"
#include "gemm_gen.h"

namespace {

constexpr int kMeanLdsDoubles = 6144;   // the forward stages W in LDS up to 48 KB (L R = 2500 for 5 x 5 x 10 patches into 10 maps); beyond: read through the caches
constexpr int kChans = 4;               // the adjoint: channels a thread holds in registers

inline unsigned blocks_for(long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

struct MeanGeom { int H, W, C, f, s, Wo, P, L, R; };
MeanGeom geom_of(const LayerState& L) { return MeanGeom{L.v.H, L.v.W, L.v.C, L.v.f, L.v.s, L.v.Wo, L.v.P, L.v.L, L.Rout}; }

// one thread per (column j, map r), r fastest: the R threads of a column read the same patch (one fetch per wave), the writes are contiguous, and a
// de-duplicated first layer of a few thousand columns still puts R times as many threads on the chip.
// Column j of this call is column col0 + j of the layer: image (col0 + j) / P shown as X[image % n_mod], patch (col0 + j) % P.
__global__ __launch_bounds__(256) void conv_mean_add_kernel(const double* __restrict__ X, int n_mod, MeanGeom g, const double* __restrict__ Wm,
                                                            int w_lds, long col0, long Kc, int rep, long rep_stride,
                                                            double* __restrict__ out_mean, double* __restrict__ out_sample) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const double* __restrict__ Wl = Wm;
  if (w_lds) {
    for (int i = threadIdx.x; i < g.L * g.R; i += 256) sm[i] = Wm[i];
    __syncthreads();
    Wl = sm;
  }
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= Kc * g.R) return;
  const long j = idx / g.R;
  const int r = (int)(idx - j * g.R);
  const long jg = col0 + j;
  const long n = jg / g.P;
  const int p = (int)(jg - n * g.P), oh = p / g.Wo, ow = p - oh * g.Wo;
  const double* __restrict__ img = X + ((n % n_mod) * g.H + (long)oh * g.s) * g.W * g.C + (long)ow * g.s * g.C;
  const int fc = g.f * g.C;   // a patch row is one contiguous run of f C values of the image
  double acc = 0.0;
  for (int kh = 0; kh < g.f; ++kh) {
    const double* __restrict__ row = img + (long)kh * g.W * g.C;
    const double* __restrict__ wr = Wl + (long)kh * fc * g.R + r;
#pragma unroll 4
    for (int q = 0; q < fc; ++q) acc = fma(row[q], wr[(long)q * g.R], acc);
  }
  const long e = jg * g.R + r;
  for (int s = 0; s < rep; ++s) {
    const long o = (long)s * rep_stride + e;
    if (out_mean) out_mean[o] += acc;
    if (out_sample) out_sample[o] += acc;
  }
}

// dX[n][h][w][ch] += sum over the patches (oh, ow) that hold the pixel, at l = ((h - oh s) f + (w - ow s)) C + ch, of sum_r gm[n P + p][r] W[l][r]
// (col2im's gather, grad.hip, with the product folded in); one thread per pixel and chunk of kChans channels (the chunk is the block's, blockIdx.y), the
// taps visited in (kh, kw) order by every lane: every filter address is uniform over the wave, and each gm value a lane loads feeds kChans FMAs
__global__ __launch_bounds__(256) void conv_mean_backward_dx_kernel(const double* __restrict__ gm, long n_pix, MeanGeom g, int Ho,
                                                                    const double* __restrict__ Wm, double* __restrict__ dX) {
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= n_pix) return;
  const int c0 = blockIdx.y * kChans, nc = g.C - c0 < kChans ? g.C - c0 : kChans;
  const int w = (int)(pix % g.W), h = (int)((pix / g.W) % g.H);
  const long n = pix / ((long)g.W * g.H);
  double acc[kChans];
#pragma unroll
  for (int cc = 0; cc < kChans; ++cc) acc[cc] = 0.0;
  for (int kh = 0; kh < g.f; ++kh) {
    const int hh = h - kh, oh = hh / g.s;
    const bool row_ok = hh >= 0 && hh % g.s == 0 && oh < Ho;
    for (int kw = 0; kw < g.f; ++kw) {
      const int ww = w - kw, ow = ww / g.s;
      if (!(row_ok && ww >= 0 && ww % g.s == 0 && ow < g.Wo)) continue;
      const double* __restrict__ gr = gm + (n * g.P + (long)oh * g.Wo + ow) * g.R;
      const double* __restrict__ wr = Wm + (long)((kh * g.f + kw) * g.C + c0) * g.R;
      for (int r = 0; r < g.R; ++r) {
        const double gv = gr[r];
#pragma unroll
        for (int cc = 0; cc < kChans; ++cc)
          if (cc < nc) acc[cc] = fma(gv, wr[(long)cc * g.R + r], acc[cc]);
      }
    }
  }
#pragma unroll
  for (int cc = 0; cc < kChans; ++cc)
    if (cc < nc) dX[pix * g.C + c0 + cc] += acc[cc];
}

}  // namespace

// out_mean / out_sample (either may be nullptr) [rep][...][Kc_layer][R]: m of columns col0 .. col0 + Kc - 1 added at s rep_stride + (col0 + j) R + r, s < rep
int conv_mean_add(dcgp_ctx* ctx, const LayerState& L, const double* X, int n_mod, long col0, long Kc, int rep, long rep_stride, double* out_mean,
                  double* out_sample) {
  if (!L.mean_W) return ctx_fail(ctx, DCGP_ERR_ARG, "conv_mean_add: the layer has no mean filter");
  if (Kc <= 0 || (!out_mean && !out_sample)) return DCGP_OK;
  const MeanGeom g = geom_of(L);
  const long n = Kc * g.R;
  if ((n + 255) / 256 > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "conv_mean_add: %ld values exceed one launch", n);
  const int lr = g.L * g.R, w_lds = lr <= kMeanLdsDoubles;
  ScopedTimer t(ctx, "conv_mean_add");
  hipLaunchKernelGGL(conv_mean_add_kernel, dim3(blocks_for(n)), dim3(256), w_lds ? lr * sizeof(double) : 0, ctx->stream, X, n_mod, g, L.mean_W, w_lds,
                     col0, Kc, rep, rep_stride, out_mean, out_sample);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// gm [rows P][R]: the adjoint of the layer's mean; dXin [rows][H][W][C] += the mean function's part
int conv_mean_backward_dx(dcgp_ctx* ctx, const LayerState& L, const double* gm, int rows, double* dXin) {
  if (!L.mean_W) return ctx_fail(ctx, DCGP_ERR_ARG, "conv_mean_backward_dx: the layer has no mean filter");
  const MeanGeom g = geom_of(L);
  const long n_pix = (long)rows * g.H * g.W;
  if (n_pix <= 0) return DCGP_OK;
  if ((n_pix + 255) / 256 > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "conv_mean_backward_dx: %ld pixels exceed one launch", n_pix);
  ScopedTimer t(ctx, "conv_mean_backward_dx");
  hipLaunchKernelGGL(conv_mean_backward_dx_kernel, dim3(blocks_for(n_pix), (unsigned)((g.C + kChans - 1) / kChans)), dim3(256), 0, ctx->stream, gm, n_pix, g,
                     L.v.Ho, L.mean_W, dXin);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// Xcol [Kc][L] (im2col of the layer's input), gm [Kc][R] -> gW [L][R] = Xcol^T gm: the reverse pass's general product (gemm_gen.hip) with the
// contraction over the columns -- split along k into partial sums per chunk of columns (a buffer per stream), then their sum in chunk order
int conv_mean_backward_filter(dcgp_ctx* ctx, const LayerState& L, const double* Xcol, const double* gm, long Kc, double* gW) {
  if (!L.mean_W) return ctx_fail(ctx, DCGP_ERR_ARG, "conv_mean_backward_filter: the layer has no mean filter");
  if (Kc > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "conv_mean_backward_filter: %ld columns exceed one product", Kc);
  GenGemm e;
  e.A = Xcol; e.a_rs = 1; e.a_cs = L.v.L;        // A(l, c) = Xcol[c][l]
  e.B = gm; e.b_rs = L.Rout; e.b_cs = 1;         // B(c, r) = gm[c][r]
  e.C = gW; e.c_rs = L.Rout;
  e.M = L.v.L; e.N = L.Rout; e.K = (int)Kc;
  ScopedTimer t(ctx, "conv_mean_backward_filter");
  return gemm_gen(ctx, e);
}

namespace {
// the yardstick of dcgp_debug_conv_mean_time: n doubles read, n written
__global__ __launch_bounds__(256) void copy_kernel(const double* __restrict__ src, long n, double* __restrict__ dst) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}
}  // namespace

// Measurement aid (tools/conv_mean_time.py): the three kernels of this file alone, each beside a copy kernel that moves the bytes the kernel must
// move -- add: the read-modify-write of rep x Kc x R sample values; backward_dx: gm read, dX read and written; backward_filter: Xcol and gm read --
// on a conv layer H x W x C, f, stride, R maps, `rows` images, `rep` replicas of the output.  `iters` launches between two events behind a
// warm-up launch, on the ctx stream; out_us[8] = microseconds per launch {add, its copy, dx, its copy, filter (both stages), its copy, 0, 0}.
extern "C" int dcgp_debug_conv_mean_time(dcgp_ctx* ctx, int H, int W, int C, int f, int stride, int R, int rows, int rep, int iters, double* out_us) {
  if (!ctx || !out_us || rows <= 0 || rep <= 0 || iters <= 0) return ctx ? ctx_fail(ctx, DCGP_ERR_ARG, "debug_conv_mean_time: bad args") : DCGP_ERR_ARG;
  LayerState L;
  DCGP_TRY(L.init(ctx, false, H, W, C, f, stride, 16, R, 0, 0, 0, 1.0, 1.0, false));
  const long Kc = (long)rows * L.v.P, n_out = (long)rep * Kc * R, n_in = (long)rows * H * W * C, n_col = Kc * L.v.L, n_gm = Kc * R;
  const long n_copy[3] = {n_out, (n_gm + 2 * n_in + 1) / 2, (n_col + n_gm + 1) / 2};
  const long n_max = std::max(n_copy[0], std::max(n_copy[1], n_copy[2]));
  if ((n_max + 255) / 256 > 0x7fffffffL || Kc > 0x7fffff00L) return ctx_fail(ctx, DCGP_ERR_ARG, "debug_conv_mean_time: shape exceeds one launch");
  L.mean_W = L.dalloc(L.mean_slots() ? L.mean_slots() : (size_t)L.v.L * R);
  double *X = L.dalloc(n_in), *out = L.dalloc(n_out), *gm = L.dalloc(n_gm), *dX = L.dalloc(n_in), *Xcol = L.dalloc(n_col), *gW = L.dalloc((size_t)L.v.L * R);
  double *src = L.dalloc(n_max), *dst = L.dalloc(n_max);
  for (void* p : L.owned) if (!p) return ctx_fail(ctx, DCGP_ERR_ALLOC, "debug_conv_mean_time: device allocation failed");
  for (auto pn : {std::make_pair(L.mean_W, (long)L.v.L * R), std::make_pair(X, n_in), std::make_pair(out, n_out), std::make_pair(gm, n_gm), std::make_pair(dX, n_in),
                  std::make_pair(Xcol, n_col), std::make_pair(src, n_max)})
    HIP_TRY(ctx, hipMemsetAsync(pn.first, 0, (size_t)pn.second * sizeof(double), ctx->stream));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(ctx, hipEventCreate(&e0));
  HIP_TRY(ctx, hipEventCreate(&e1));
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
  auto copy = [&](long n) {
    hipLaunchKernelGGL(copy_kernel, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, src, n, dst);
    return hipGetLastError() == hipSuccess ? DCGP_OK : DCGP_ERR_HIP;
  };
  timed(0, [&] { return conv_mean_add(ctx, L, X, rows, 0, Kc, rep, Kc * R, nullptr, out); });
  timed(1, [&] { return copy(n_copy[0]); });
  timed(2, [&] { return conv_mean_backward_dx(ctx, L, gm, rows, dX); });
  timed(3, [&] { return copy(n_copy[1]); });
  timed(4, [&] { return conv_mean_backward_filter(ctx, L, Xcol, gm, Kc, gW); });
  timed(5, [&] { return copy(n_copy[2]); });
  out_us[6] = out_us[7] = 0.0;
  hipStreamSynchronize(ctx->stream);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  if (rc != DCGP_OK) return ctx_fail(ctx, rc, "debug_conv_mean_time: a launch or an event failed");
  return DCGP_OK;
}

extern "C" int dcgp_model_set_mean_filter(dcgp_model* model, int layer, const double* filter_host, int trainable) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (!filter_host) return ctx_fail(ctx, DCGP_ERR_ARG, "set_mean_filter: the filter is NULL");
  if (layer < 0 || layer >= (int)model->layers.size()) return ctx_fail(ctx, DCGP_ERR_ARG, "set_mean_filter: no layer %d", layer);
  LayerState& L = *model->layers[layer];
  if (L.is_head) return ctx_fail(ctx, DCGP_ERR_ARG, "set_mean_filter: layer %d is the head, only conv layers take a mean filter", layer);
  if (L.identity_mean)
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_mean_filter: layer %d was added with identity_mean (the in-launch Conv2dMean); add it without to give it a filter", layer);
  if (model->enq_seq != model->col_seq) return ctx_fail(ctx, DCGP_ERR_ARG, "set_mean_filter: enqueued steps are still to be collected");
  const size_t n = (size_t)L.v.L * L.Rout;
  if (!L.mean_W) {
    // the filter's gradient takes L R slots at the end of the layer's gradient block: the block must not exist yet
    if (L.gZ || L.pstage || L.hyp) return ctx_fail(ctx, DCGP_ERR_ARG, "set_mean_filter: layer %d has taken a gradient step; give it its filter before the first", layer);
    double* w = L.dalloc(n);
    if (!w) return ctx_fail(ctx, DCGP_ERR_ALLOC, "layer: device allocation failed");
    L.mean_W = w;
  }
  L.mean_trainable = trainable != 0;
  return L.upload(L.mean_W, filter_host, n);
}

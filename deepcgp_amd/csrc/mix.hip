// mix.hip -- a mixed conv layer: G = gp_count latent GPs emitted as R feature maps through a trainable matrix W [G][R] (gpflow's
// SharedMixed... / LinearCoregionalization on a conv layer's patches).  Per column j = (row, patch), sample first, then mix:
//     u[j, :]      = gm[j, :] + z[j, :] sqrt(gv[j, :] + jitter)                      (the layer's own kernels: its old sample, G wide)
//     sample[j, r] = sum_g u[j, g]  W[g, r]        mean[j, r] = sum_g gm[j, g] W[g, r]        var[j, r] = sum_g gv[j, g] W[g, r]^2
// every sum over g = 0 .. G-1 in that order as one FMA chain from 0.0: W = I gives the unmixed layer's values, a permutation its maps permuted.
// Three kernels:
//   mix_forward          behind the point where the layer's latent outputs exist (conv_forward, layer_impl.h), ahead of conv_mean_add
//   mix_backward_latent  gu[j, g] = sum_r gF[j, r] W[g, r] (sample_backward then runs on the latent triple, grad.hip)
//   mix_backward_w       gW[g, r] = sum_j u[j, g] gF[j, r]: per-workgroup partial sums (LDS, fixed order), then their sum in a fixed tree
// Every output element has one writer and every sum a fixed order: no atomics, two runs give the same bits.  Plain fp64, memory-bound
// (8 * 3 * (G + R) bytes a column at most); W is read from LDS.
#include "model_state.h"

namespace {

constexpr int kMixLdsDoubles = 4096;   // W staged in LDS up to 32 KB; beyond: read through the caches
constexpr int kTile = 32;              // mix_backward_w: columns staged per round

inline unsigned blocks_for(long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

// one thread per (column j, map r), r fastest: the R threads of a column read the same G latent values (one fetch per wave), the writes are
// contiguous.  Column j of this call is column col0 + j of the layer; replica s of it at s * lat_stride + (col0 + j) G in the latent buffers and at
// s * out_stride + (col0 + j) R in the outputs.
__global__ __launch_bounds__(256) void mix_forward_kernel(const double* __restrict__ Wg, int w_lds, int G, int R, const double* __restrict__ u,
                                                          const double* __restrict__ gm, const double* __restrict__ gv, long col0, long Kc, int rep,
                                                          long lat_stride, long out_stride, double* __restrict__ out_sample,
                                                          double* __restrict__ out_mean, double* __restrict__ out_var) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const double* __restrict__ Wl = Wg;
  if (w_lds) {
    for (int i = threadIdx.x; i < G * R; i += 256) sm[i] = Wg[i];
    __syncthreads();
    Wl = sm;
  }
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= Kc * R) return;
  const long j = idx / R;
  const int r = (int)(idx - j * R);
  const long jg = col0 + j;
  for (int s = 0; s < rep; ++s) {
    const long li = (long)s * lat_stride + jg * G, o = (long)s * out_stride + jg * R + r;
    if (out_sample) {
      double a = 0.0;
      for (int g = 0; g < G; ++g) a = fma(u[li + g], Wl[g * R + r], a);
      out_sample[o] = a;
    }
    if (out_mean) {
      double a = 0.0;
      for (int g = 0; g < G; ++g) a = fma(gm[li + g], Wl[g * R + r], a);
      out_mean[o] = a;
    }
    if (out_var) {
      double a = 0.0;
      for (int g = 0; g < G; ++g) { const double w = Wl[g * R + r]; a = fma(gv[li + g], w * w, a); }
      out_var[o] = a;
    }
  }
}

// one thread per (column j, latent g), g fastest: gu[j, g] = sum_r gF[j, r] W[g, r], r = 0 .. R-1 in that order
__global__ __launch_bounds__(256) void mix_backward_latent_kernel(const double* __restrict__ Wg, int w_lds, int G, int R, const double* __restrict__ gF,
                                                                  long Kc, double* __restrict__ gu) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const double* __restrict__ Wl = Wg;
  if (w_lds) {
    for (int i = threadIdx.x; i < G * R; i += 256) sm[i] = Wg[i];
    __syncthreads();
    Wl = sm;
  }
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= Kc * G) return;
  const long j = idx / G;
  const int g = (int)(idx - j * G);
  const double* __restrict__ gr = gF + j * R;
  const double* __restrict__ wr = Wl + (long)g * R;
  double a = 0.0;
  for (int r = 0; r < R; ++r) a = fma(gr[r], wr[r], a);
  gu[idx] = a;
}

// Stage 1 of gW: workgroup (x, y) owns columns [x cpw, min((x + 1) cpw, Kc)) and the pairs (g, r) = y pb .. y pb + pb - 1 (pb = min(G R, 256)).
// Its 256 threads are nsl = 256 / pb slices of pb pairs: slice q takes columns q, q + nsl, ... of every staged tile, in that order; the slices'
// sums are then added in slice order by the pair's first thread -> part[x][pair].  The order depends on (Kc, cpw, G, R) alone.
__global__ __launch_bounds__(256) void mix_backward_w_partial_kernel(const double* __restrict__ u, const double* __restrict__ gF, int G, int R, long Kc,
                                                                     long cpw, int pb, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* tu = sm;                       // [kTile][G]
  double* tf = sm + (size_t)kTile * G;   // [kTile][R]
  double* red = tf + (size_t)kTile * R;  // [nsl][pb]
  const int t = threadIdx.x, npairs = G * R, nsl = 256 / pb;
  const int q = t / pb, pl = t - q * pb, pair = blockIdx.y * pb + pl;
  const bool live = q < nsl && pair < npairs;
  const int g = live ? pair / R : 0, r = live ? pair - g * R : 0;
  const long c0 = (long)blockIdx.x * cpw, c1 = c0 + cpw < Kc ? c0 + cpw : Kc;
  double acc = 0.0;
  for (long b = c0; b < c1; b += kTile) {
    const int nt = (int)(c1 - b < kTile ? c1 - b : kTile);
    __syncthreads();   // the previous tile has been read
    for (int i = t; i < nt * G; i += 256) tu[i] = u[b * G + i];
    for (int i = t; i < nt * R; i += 256) tf[i] = gF[b * R + i];
    __syncthreads();
    if (live)
      for (int c = q; c < nt; c += nsl) acc = fma(tu[c * G + g], tf[c * R + r], acc);
  }
  if (q < nsl) red[q * pb + pl] = acc;
  __syncthreads();
  if (q == 0 && pair < npairs) {
    double s = 0.0;
    for (int k = 0; k < nsl; ++k) s += red[k * pb + pl];
    part[(long)blockIdx.x * npairs + pair] = s;
  }
}
// Stage 2, one workgroup per pair: thread t adds part[x][pair] over x = t, t + 256, ... in that order, then the 256 sums fold in LDS by halves
// (s[t] += s[t + h], h = 128, 64, .. 1): a fixed tree.  (One thread per pair walking every workgroup's partial sum was 160 us at 720 workgroups:
// a chain of dependent loads on one wave.)
__global__ __launch_bounds__(256) void mix_backward_w_sum_kernel(const double* __restrict__ part, int nwg, int npairs, double* __restrict__ gW) {
  __shared__ double red[256];
  const int p = blockIdx.x, t = threadIdx.x;
  double s = 0.0;
  for (int x = t; x < nwg; x += 256) s += part[(long)x * npairs + p];
  red[t] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  if (t == 0) gW[p] = red[0];
}

// the yardstick of dcgp_debug_mix_time: n doubles read, n written
__global__ __launch_bounds__(256) void mix_copy_kernel(const double* __restrict__ src, long n, double* __restrict__ dst) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

int check_shape(dcgp_ctx* ctx, const char* who, int G, int R, long Kc) {
  if (G < 1 || G > kMixMaxMaps) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: G = %d latent GPs, 1 .. %d are taken", who, G, kMixMaxMaps);
  if (R < 1 || R > kMixMaxMaps) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: R = %d output maps, 1 .. %d are taken", who, R, kMixMaxMaps);
  if (Kc < 0) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: %ld columns", who, Kc);
  const long n = Kc * (G > R ? G : R);
  if ((n + 255) / 256 > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: %ld values exceed one launch", who, n);
  return DCGP_OK;
}

}  // namespace

// the partial sums of mix_backward_w on Kc columns: workgroups and columns per workgroup (a few thousand columns still give ~a hundred workgroups,
// a large batch at most 1024 partial sums per pair)
void mix_w_plan(long Kc, int* nwg, long* cpw) {
  long c = (Kc + 1023) / 1024;
  c = (c + kTile - 1) / kTile * kTile;
  if (c < kTile) c = kTile;
  *cpw = c;
  *nwg = (int)((Kc + c - 1) / c);
}

int mix_forward(dcgp_ctx* ctx, const double* W, int G, int R, const double* u, const double* gm, const double* gv, long col0, long Kc, int rep,
                long lat_stride, long out_stride, double* out_sample, double* out_mean, double* out_var) {
  DCGP_TRY(check_shape(ctx, "mix_forward", G, R, Kc));
  if (!W) return ctx_fail(ctx, DCGP_ERR_ARG, "mix_forward: no mixing matrix");
  if ((out_sample && !u) || (out_mean && !gm) || (out_var && !gv)) return ctx_fail(ctx, DCGP_ERR_ARG, "mix_forward: an output without its latent input");
  if (Kc == 0 || rep <= 0 || (!out_sample && !out_mean && !out_var)) return DCGP_OK;
  const int w_lds = G * R <= kMixLdsDoubles;
  ScopedTimer t(ctx, "mix_forward");
  hipLaunchKernelGGL(mix_forward_kernel, dim3(blocks_for(Kc * R)), dim3(256), w_lds ? (size_t)G * R * sizeof(double) : 0, ctx->stream, W, w_lds, G, R, u,
                     gm, gv, col0, Kc, rep, lat_stride, out_stride, out_sample, out_mean, out_var);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int mix_backward_latent(dcgp_ctx* ctx, const double* W, int G, int R, const double* gF, long Kc, double* gu) {
  DCGP_TRY(check_shape(ctx, "mix_backward_latent", G, R, Kc));
  if (!W || !gF || !gu) return ctx_fail(ctx, DCGP_ERR_ARG, "mix_backward_latent: NULL pointer");
  if (Kc == 0) return DCGP_OK;
  const int w_lds = G * R <= kMixLdsDoubles;
  ScopedTimer t(ctx, "mix_backward_latent");
  hipLaunchKernelGGL(mix_backward_latent_kernel, dim3(blocks_for(Kc * G)), dim3(256), w_lds ? (size_t)G * R * sizeof(double) : 0, ctx->stream, W, w_lds,
                     G, R, gF, Kc, gu);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// part: nwg * G * R doubles (mix_w_plan)
int mix_backward_w(dcgp_ctx* ctx, int G, int R, const double* u, const double* gF, long Kc, double* part, double* gW) {
  DCGP_TRY(check_shape(ctx, "mix_backward_w", G, R, Kc));
  if (!u || !gF || !part || !gW) return ctx_fail(ctx, DCGP_ERR_ARG, "mix_backward_w: NULL pointer");
  const int npairs = G * R;
  if (Kc == 0) { HIP_TRY(ctx, hipMemsetAsync(gW, 0, (size_t)npairs * sizeof(double), ctx->stream)); return DCGP_OK; }
  int nwg; long cpw;
  mix_w_plan(Kc, &nwg, &cpw);
  const int pb = npairs < 256 ? npairs : 256, nsl = 256 / pb;
  const size_t lds = ((size_t)kTile * (G + R) + (size_t)nsl * pb) * sizeof(double);   // at most 32 * 2 kMixMaxMaps + 256 doubles = 34 KB
  ScopedTimer t(ctx, "mix_backward_w");
  hipLaunchKernelGGL(mix_backward_w_partial_kernel, dim3((unsigned)nwg, (unsigned)((npairs + pb - 1) / pb)), dim3(256), lds, ctx->stream, u, gF, G, R, Kc,
                     cpw, pb, part);
  LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(mix_backward_w_sum_kernel, dim3((unsigned)npairs), dim3(256), 0, ctx->stream, part, nwg, npairs, gW);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

extern "C" {

int dcgp_mix_forward(dcgp_ctx* ctx, const double* W_dev, int G, int R, const double* u_dev, const double* gm_dev, const double* gv_dev, long col0, long Kc,
                     int rep, long lat_stride, long out_stride, double* sample_dev, double* mean_dev, double* var_dev) {
  if (!ctx) return DCGP_ERR_ARG;
  if (col0 < 0 || rep < 1) return ctx_fail(ctx, DCGP_ERR_ARG, "mix_forward: col0 = %ld, rep = %d", col0, rep);
  DCGP_TRY(mix_forward(ctx, W_dev, G, R, u_dev, gm_dev, gv_dev, col0, Kc, rep, lat_stride, out_stride, sample_dev, mean_dev, var_dev));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

int dcgp_mix_backward(dcgp_ctx* ctx, const double* W_dev, int G, int R, const double* u_dev, const double* gF_dev, long Kc, double* gu_dev, double* gW_dev) {
  if (!ctx) return DCGP_ERR_ARG;
  if (gu_dev) DCGP_TRY(mix_backward_latent(ctx, W_dev, G, R, gF_dev, Kc, gu_dev));
  if (gW_dev) {
    DCGP_TRY(check_shape(ctx, "mix_backward_w", G, R, Kc));
    int nwg; long cpw;
    mix_w_plan(Kc > 0 ? Kc : 1, &nwg, &cpw);
    double* part = (double*)ws_get(ctx, "mix_part", (size_t)nwg * G * R * sizeof(double));
    if (!part) return DCGP_ERR_ALLOC;
    DCGP_TRY(mix_backward_w(ctx, G, R, u_dev, gF_dev, Kc, part, gW_dev));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

int dcgp_model_set_mixing(dcgp_model* model, int layer, const double* W_host, int G, int R) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (layer < 0 || layer >= (int)model->layers.size()) return ctx_fail(ctx, DCGP_ERR_ARG, "set_mixing: no layer %d", layer);
  LayerState& L = *model->layers[layer];
  if (L.is_head) return ctx_fail(ctx, DCGP_ERR_ARG, "set_mixing: layer %d is the head, only conv layers are mixed", layer);
  if (model->enq_seq != model->col_seq) return ctx_fail(ctx, DCGP_ERR_ARG, "set_mixing: enqueued steps are still to be collected");
  // the matrix's gradient takes G R slots at the end of the layer's gradient block, and a mean filter has one column per output map
  if (L.gZ || L.pstage || L.hyp) return ctx_fail(ctx, DCGP_ERR_ARG, "set_mixing: layer %d has taken a gradient step; give it its mixing before the first", layer);
  if (L.mean_W) return ctx_fail(ctx, DCGP_ERR_ARG, "set_mixing: layer %d has a mean filter on %d maps; give it its mixing before the filter", layer, L.Rout);
  if (!W_host) {   // off again: the layer emits its gp_count maps
    L.mix_W = nullptr; L.Rout = L.R; L.mix_trainable = false;
    model->pad_ok = false;
    ++model->param_version;
    return DCGP_OK;
  }
  if (L.identity_mean)
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_mixing: layer %d was added with identity_mean (the in-launch Conv2dMean adds into latent map 0); add it without and "
                    "give it the centre-pixel filter (dcgp_model_set_mean_filter)", layer);
  if (G != L.R) return ctx_fail(ctx, DCGP_ERR_ARG, "set_mixing: G = %d latent GPs, layer %d was added with gp_count %d", G, layer, L.R);
  if (R < 1 || R > kMixMaxMaps) return ctx_fail(ctx, DCGP_ERR_ARG, "set_mixing: R = %d output maps, 1 .. %d are taken", R, kMixMaxMaps);
  if (G > kMixMaxMaps) return ctx_fail(ctx, DCGP_ERR_ARG, "set_mixing: G = %d latent GPs, at most %d are mixed", G, kMixMaxMaps);
  if (layer + 1 < (int)model->layers.size()) {   // (a dense head's single patch is the whole output: P R values)
    const LayerState& B = *model->layers[layer + 1];
    const bool dense = B.is_head && B.v.H == 1 && B.v.W == 1;
    if (B.v.C != (dense ? L.v.P : 1) * R)
      return ctx_fail(ctx, DCGP_ERR_ARG, "set_mixing: R = %d output maps, layer %d takes C = %d channels", R, layer + 1, B.v.C);
  }
  if (!L.mix_buf || L.mix_cap < (size_t)G * R) {
    double* w = L.dalloc((size_t)G * R);
    if (!w) return ctx_fail(ctx, DCGP_ERR_ALLOC, "layer: device allocation failed");
    L.mix_buf = w; L.mix_cap = (size_t)G * R;
  }
  if (!L.mix_W) L.mix_trainable = true;
  L.mix_W = L.mix_buf; L.Rout = R;
  model->pad_ok = false;
  ++model->param_version;
  return L.upload(L.mix_W, W_host, (size_t)G * R);
}

// Measurement aid (tools/mixing_time.py): the three kernels of this file alone, each beside a copy kernel that moves the bytes the kernel must move
// -- forward: (u, gm, gv) read and (sample, mean, var) written; backward_latent: gF read, gu written; backward_w: u and gF read -- on Kc columns,
// G latent GPs, R maps.  `iters` launches between two events behind a warm-up launch; out_us[8] = microseconds per launch {forward, its copy,
// backward_latent, its copy, backward_w (both stages), its copy, 0, 0}.
int dcgp_debug_mix_time(dcgp_ctx* ctx, int G, int R, long Kc, int iters, double* out_us) {
  if (!ctx || !out_us || Kc <= 0 || iters <= 0) return ctx ? ctx_fail(ctx, DCGP_ERR_ARG, "debug_mix_time: bad args") : DCGP_ERR_ARG;
  DCGP_TRY(check_shape(ctx, "debug_mix_time", G, R, Kc));
  const long nl = Kc * G, no = Kc * R;
  const long n_copy[3] = {3 * (nl + no) / 2 + 1, (nl + no) / 2 + 1, (nl + no) / 2 + 1};
  int nwg; long cpw;
  mix_w_plan(Kc, &nwg, &cpw);
  double* base = (double*)ws_get(ctx, "mix_time", (size_t)(3 * nl + 4 * no + 2 * n_copy[0] + (long)nwg * G * R + 2L * G * R) * sizeof(double));
  if (!base) return DCGP_ERR_ALLOC;
  double *u = base, *gm = u + nl, *gv = gm + nl, *s = gv + nl, *m = s + no, *v = m + no, *gF = v + no, *src = gF + no, *dst = src + n_copy[0];
  double *part = dst + n_copy[0], *W = part + (long)nwg * G * R, *gW = W + (long)G * R;
  HIP_TRY(ctx, hipMemsetAsync(base, 0, (size_t)(gW + (long)G * R - base) * sizeof(double), ctx->stream));
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
    hipLaunchKernelGGL(mix_copy_kernel, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, src, n, dst);
    return hipGetLastError() == hipSuccess ? DCGP_OK : DCGP_ERR_HIP;
  };
  timed(0, [&] { return mix_forward(ctx, W, G, R, u, gm, gv, 0, Kc, 1, 0, 0, s, m, v); });
  timed(1, [&] { return copy(n_copy[0]); });
  timed(2, [&] { return mix_backward_latent(ctx, W, G, R, gF, Kc, u); });
  timed(3, [&] { return copy(n_copy[1]); });
  timed(4, [&] { return mix_backward_w(ctx, G, R, u, gF, Kc, part, gW); });
  timed(5, [&] { return copy(n_copy[2]); });
  out_us[6] = out_us[7] = 0.0;
  hipStreamSynchronize(ctx->stream);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  if (rc != DCGP_OK) return ctx_fail(ctx, rc, "debug_mix_time: a launch or an event failed");
  return DCGP_OK;
}

}  // extern "C"

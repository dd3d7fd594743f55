// greedy.hip -- greedy conditional-variance selection of inducing points (Burt, Rasmussen & van der Wilk, JMLR 2020; robustgp's
// ConditionalVariance): a partial pivoted Cholesky factorisation of the candidates' Gram matrix under a layer's own base kernel, in place of
// the k-means of conv_gp/kernels.py:147-164.  The Gram matrix is never formed: pivot m evaluates ONE column of it, projects out the m rows
// chosen so far and lowers every candidate's residual variance.
//
// Launch structure: one plain launch per pivot, all enqueued on the ctx's stream, no host synchronisation between them.  Launch m
//   1. reduces, in EVERY workgroup, the per-workgroup slots (largest residual, its lowest index, sum of residuals) that launch m - 1 left:
//      pivot j, its residual d_j and the Nystrom trace after m picks (a few hundred values; the kernel boundary makes them visible);
//   2. stops for good when d_j <= min_variance (the state word then holds n_greedy and this and every later launch returns at once);
//   3. stages x_j and the pivot column c_t[j], t < m, in LDS;
//   4. one lane per candidate column i: k(x_i, x_j) from the transposed candidates [d][n], the projection sum_t c_t[j] c_t[i] from the
//      factor rows [k][n] (both coalesced), c_m[i], the new residual;
//   5. leaves its slab's slot for launch m + 1 (slots double-buffered by the parity of m).
// No atomics, no grid barrier: every sum has a fixed order, so a call gives the same bits every run.
#include <cfloat>
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int GV_T = 256;          // lanes of a workgroup: one candidate column each per round
constexpr int GV_MAX_WGS = 1024;   // slots every workgroup reduces; beyond n = 256 * 1024 a lane takes several columns
constexpr int GV_MAX_K = 4096, GV_MAX_D = 4096;

struct GvArgs {
  const double* X = nullptr;    // [n][d] the candidates as given (the pivot row is read from here)
  const double* XT = nullptr;   // [d][n] transposed (ARD: divided by the lengthscales)
  const double* xn = nullptr;   // [n] |x|^2 (ArcCosine only)
  const double* ard = nullptr;  // [d] lengthscales or nullptr
  double* C = nullptr;          // [k][n] factor rows c_m
  double* resid = nullptr;      // [n] residual variances d
  double* slot_max = nullptr;   // [2][nwg]
  double* slot_sum = nullptr;   // [2][nwg]
  int* slot_idx = nullptr;      // [2][nwg]
  int* state = nullptr;         // [0] n_greedy once the selection has stalled, else -1; [1] 1 + pivot at which a residual was not finite, else 0
  int32_t* rows = nullptr;      // [k]
  double* trace = nullptr;      // [k]
  long n = 0;
  int d = 0, k = 0, nwg = 0, cpl = 1, m = 0;
  BaseKernel bk;
  double min_variance = 0.0;
};

struct Best { double v; int idx; double sum; };

__device__ __forceinline__ void take(Best& a, double v, int idx) {
  if (v > a.v || (v == a.v && idx < a.idx)) { a.v = v; a.idx = idx; }
}
// (largest value, its lowest index, sum) over the workgroup, the same bits in every lane: a butterfly inside each wave, then the four waves in order
__device__ __forceinline__ Best block_best(Best b, Best* sh) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double ov = __shfl_xor(b.v, o), os = __shfl_xor(b.sum, o);
    const int oi = __shfl_xor(b.idx, o);
    take(b, ov, oi);
    b.sum += os;
  }
  __syncthreads();   // sh may still be read from the previous use
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = b;
  __syncthreads();
  Best r = sh[0];
#pragma unroll
  for (int w = 1; w < GV_T / 64; ++w) { take(r, sh[w].v, sh[w].idx); r.sum += sh[w].sum; }
  return r;
}
__device__ __forceinline__ Best slots_best(const GvArgs& a, int par, Best* sh) {
  Best b{-1.0, INT_MAX, 0.0};
  for (int s = threadIdx.x; s < a.nwg; s += GV_T) {
    take(b, a.slot_max[par * a.nwg + s], a.slot_idx[par * a.nwg + s]);
    b.sum += a.slot_sum[par * a.nwg + s];
  }
  return block_best(b, sh);
}

// XT[l][i] = X[i][l] (/ lengthscale_l): 32 x 32 tiles through LDS, both sides coalesced
__global__ __launch_bounds__(256) void gv_transpose_kernel(const double* __restrict__ X, long n, int d, const double* __restrict__ ard,
                                                           double* __restrict__ XT) {
  __shared__ double t[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const long i0 = (long)blockIdx.x * 32;
  const int l0 = blockIdx.y * 32;
  for (int r = ty; r < 32; r += 8) {
    const long i = i0 + r;
    const int l = l0 + tx;
    double v = 0.0;
    if (i < n && l < d) { v = X[i * d + l]; if (ard) v /= ard[l]; }
    t[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int l = l0 + r;
    const long i = i0 + tx;
    if (l < d && i < n) XT[(long)l * n + i] = t[tx][r];
  }
}

// residual = the Gram matrix's own diagonal, |x|^2 for the ArcCosine, and the slots launch 0 reads.  The diagonal is a constant, nothing is
// evaluated per candidate: variance (gpflow's Kdiag) for the stationary kernels; for the ArcCosine the entry K_uu holds, BaseKernel::eval_diag's
// variance (1 - acos(1 - 1e-15) / pi) -- 1.4e-8 variance below Kdiag, and started from Kdiag the factor would be that of K + 1.4e-8 variance I
__global__ __launch_bounds__(GV_T) void gv_init_kernel(GvArgs a, double* __restrict__ xn) {
  __shared__ Best sh[GV_T / 64];
  Best e{-1.0, INT_MAX, 0.0};
  const double d0 = a.bk.type == 1 ? a.bk.eval_diag(0.0, 0.0, 0.0) : a.bk.variance;
  for (int r = 0; r < a.cpl; ++r) {
    const long i = ((long)blockIdx.x * a.cpl + r) * GV_T + threadIdx.x;
    if (i >= a.n) continue;
    a.resid[i] = d0;
    if (xn) {
      double s = 0.0;
      for (int l = 0; l < a.d; ++l) { const double v = a.XT[(long)l * a.n + i]; s = fma(v, v, s); }
      xn[i] = s;
    }
    take(e, d0, (int)i);
    e.sum += d0;
  }
  e = block_best(e, sh);
  if (threadIdx.x == 0) {
    a.slot_max[a.nwg + blockIdx.x] = e.v; a.slot_idx[a.nwg + blockIdx.x] = e.idx; a.slot_sum[a.nwg + blockIdx.x] = e.sum;
  }
}

template <int T>
__global__ __launch_bounds__(GV_T) void gv_pivot_kernel(GvArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ Best sh[GV_T / 64];
  double* xj = smem;         // [d]
  double* cj = smem + a.d;   // [m]
  const int tid = threadIdx.x, m = a.m;
  const long n = a.n;
  if (a.state[0] >= 0 || a.state[1] != 0) return;   // stalled, or a residual was not finite: nothing more is selected
  const Best p = slots_best(a, (m + 1) & 1, sh);
  const int j = p.idx;
  const double dj = p.v;
  const bool first = blockIdx.x == 0 && tid == 0;
  if (first && m > 0) a.trace[m - 1] = p.sum;
  if (!(dj > a.min_variance)) {   // every workgroup finds the same
    if (first) a.state[0] = m;
    return;
  }
  if (first) a.rows[m] = j;
  for (int l = tid; l < a.d; l += GV_T) {
    double v = a.X[(long)j * a.d + l];
    if (a.ard) v /= a.ard[l];   // the same division as the transposition's: a duplicate of x_j is at distance exactly 0
    xj[l] = v;
  }
  for (int t = tid; t < m; t += GV_T) cj[t] = a.C[(long)t * n + j];
  __syncthreads();
  const double sq = sqrt(dj);
  const double nj = T == 1 ? a.xn[j] : 0.0;
  Best e{-1.0, INT_MAX, 0.0};
  bool bad = false;
  for (int r = 0; r < a.cpl; ++r) {
    const long i = ((long)blockIdx.x * a.cpl + r) * GV_T + tid;
    if (i >= n) continue;
    // k(x_i, x_j): squared distance by differences (stationary kernels), inner product (ArcCosine)
    double s = 0.0;
    const double* __restrict__ xi = a.XT + i;
    if (T == 1) {
#pragma unroll 8
      for (int l = 0; l < a.d; ++l) s = fma(xi[(long)l * n], xj[l], s);
    } else {
#pragma unroll 8
      for (int l = 0; l < a.d; ++l) { const double df = xi[(long)l * n] - xj[l]; s = fma(df, df, s); }
    }
    const double kv = T == 1 ? a.bk.template eval_as<1>(s, a.xn[i], nj) : a.bk.template eval_as<T>(0.0, s, 0.0);
    // sum_t c_t[j] c_t[i]: four chains, t mod 4, combined in a fixed order
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const double* __restrict__ ci = a.C + i;
    int t = 0;
    for (; t + 16 <= m; t += 16) {   // sixteen loads in flight a lane: a pick's few hundred waves do not fill the chip, the reads' latency is what there is to hide
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = ci[(long)(t + u) * n];
#pragma unroll
      for (int u = 0; u < 16; ++u) acc[u & 3] = fma(cj[t + u], v[u], acc[u & 3]);
    }
    for (; t + 4 <= m; t += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = fma(cj[t + u], ci[(long)(t + u) * n], acc[u]);
    }
    for (int u = 0; t < m; ++t, ++u) acc[u] = fma(cj[t], ci[(long)t * n], acc[u]);
    const double proj = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    const bool piv = i == (long)j;
    const double di = a.resid[i];
    // nothing is left of a candidate at residual 0 (an earlier pick, or a copy of one): its entry is an exact zero, not the rounding of one
    const double c = piv ? sq : di == 0.0 ? 0.0 : (kv - proj) / sq;
    double dn = di - c * c;
    if (!(fabs(dn) <= DBL_MAX)) bad = true;   // NaN or infinite: not clamped away
    dn = piv ? 0.0 : fmax(dn, 0.0);
    a.C[(long)m * n + i] = c;
    a.resid[i] = dn;
    take(e, dn, (int)i);
    e.sum += dn;
  }
  if (bad) a.state[1] = m + 1;
  e = block_best(e, sh);
  if (tid == 0) {
    const int s = (m & 1) * a.nwg + blockIdx.x;
    a.slot_max[s] = e.v; a.slot_idx[s] = e.idx; a.slot_sum[s] = e.sum;
  }
}

// behind the last pivot launch: n_greedy, the trace of the last pick, and the trace repeated over the picks that were not made
__global__ __launch_bounds__(GV_T) void gv_finish_kernel(GvArgs a) {
  __shared__ Best sh[GV_T / 64];
  const int stalled = a.state[0];
  const int ng = stalled >= 0 ? stalled : a.k;
  const Best p = slots_best(a, (ng + 1) & 1, sh);   // what the last launch that selected left (ng == 0: the initial slots)
  if (stalled < 0 && threadIdx.x == 0) a.trace[a.k - 1] = p.sum;
  for (int m = ng + threadIdx.x; m < a.k; m += GV_T) a.trace[m] = p.sum;
  __syncthreads();   // every lane has read the state word
  if (threadIdx.x == 0) a.state[0] = ng;
}

__global__ void gv_empty_kernel() {}

// device buffers of one call: freed on every way out
struct GvBuffers {
  dcgp_ctx* ctx;
  std::vector<void*> ptrs;
  explicit GvBuffers(dcgp_ctx* c) : ctx(c) {}
  ~GvBuffers() { for (void* p : ptrs) dev_free(ctx, p); }
  void* get(size_t bytes, const char* label) {
    void* p = nullptr;
    if (dev_alloc(ctx, &p, bytes, label) != hipSuccess) {
      ctx_fail(ctx, DCGP_ERR_ALLOC, "greedy_variance: allocation of %zu bytes ('%s') failed", bytes, label);
      return nullptr;
    }
    ptrs.push_back(p);
    return p;
  }
};

template <int T>
int gv_launch(dcgp_ctx* ctx, const GvArgs& a, size_t lds) {
  if (lds > 48 * 1024)
    HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&gv_pivot_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  GvArgs b = a;
  for (int m = 0; m < a.k; ++m) {
    b.m = m;
    hipLaunchKernelGGL(gv_pivot_kernel<T>, dim3(a.nwg), dim3(GV_T), lds, ctx->stream, b);
    LAUNCH_CHECK(ctx);
  }
  return DCGP_OK;
}

}  // namespace

#define GV_ARG(cond, ...) \
  do { if (!(cond)) return ctx_fail(ctx, DCGP_ERR_ARG, __VA_ARGS__); } while (0)

extern "C" int dcgp_greedy_variance(dcgp_ctx* ctx, const double* X, long n, int d, int k, int kernel_type, double variance, double p1, double p2,
                                    const double* ard_lengthscales, double min_variance, int32_t* rows_out, double* trace_out,
                                    double* residual_out, double* factor_out, int* n_greedy_out) {
  if (!ctx) return DCGP_ERR_ARG;
  GV_ARG(X, "greedy_variance: X is NULL");
  GV_ARG(rows_out, "greedy_variance: rows_out is NULL");
  GV_ARG(trace_out, "greedy_variance: trace_out is NULL");
  GV_ARG(residual_out, "greedy_variance: residual_out is NULL");
  GV_ARG(n_greedy_out, "greedy_variance: n_greedy_out is NULL");
  GV_ARG(d >= 1 && d <= GV_MAX_D, "greedy_variance: d = %d outside 1 .. %d", d, GV_MAX_D);
  GV_ARG(k >= 1 && k <= GV_MAX_K, "greedy_variance: k = %d outside 1 .. %d", k, GV_MAX_K);
  GV_ARG(n >= 1 && n <= 0x7fffffffL, "greedy_variance: n = %ld outside 1 .. 2^31 - 1", n);
  GV_ARG(k <= n, "greedy_variance: k = %d exceeds n = %ld", k, n);
  GV_ARG(kernel_type >= 0 && kernel_type <= 3, "greedy_variance: unknown kernel_type %d (0 rbf, 1 acos, 2 matern32, 3 matern52)", kernel_type);
  GV_ARG(!ard_lengthscales || kernel_type == 0, "greedy_variance: ard_lengthscales go with kernel_type 0 (rbf), got %d", kernel_type);
  GV_ARG(variance > 0.0 && std::isfinite(variance), "greedy_variance: variance must be positive, got %g", variance);
  if (kernel_type == 1) {
    GV_ARG(p1 > 0.0 && std::isfinite(p1), "greedy_variance: p1 (weight variance) must be positive, got %g", p1);
    GV_ARG(p2 >= 0.0 && std::isfinite(p2), "greedy_variance: p2 (bias variance) must not be negative, got %g", p2);
  } else {
    GV_ARG(p1 > 0.0 && std::isfinite(p1), "greedy_variance: p1 (lengthscale) must be positive, got %g", p1);
  }
  GV_ARG(min_variance >= 0.0, "greedy_variance: min_variance must not be negative, got %g", min_variance);
  if (ard_lengthscales) {   // before anything is enqueued: the only read-back in front of the launches
    std::vector<double> ls(d);
    HIP_TRY(ctx, hipMemcpy(ls.data(), ard_lengthscales, (size_t)d * sizeof(double), hipMemcpyDeviceToHost));
    for (int l = 0; l < d; ++l) GV_ARG(ls[l] > 0.0 && std::isfinite(ls[l]), "greedy_variance: ard_lengthscales[%d] must be positive, got %g", l, ls[l]);
  }

  GvArgs a;
  const long wg_cap = ctx->opt.greedy_wgs > 0 ? (ctx->opt.greedy_wgs < GV_MAX_WGS ? ctx->opt.greedy_wgs : GV_MAX_WGS) : GV_MAX_WGS;
  a.cpl = (int)((n + GV_T * wg_cap - 1) / (GV_T * wg_cap));
  a.nwg = (int)((n + (long)GV_T * a.cpl - 1) / ((long)GV_T * a.cpl));
  a.n = n; a.d = d; a.k = k; a.min_variance = min_variance;
  a.bk.type = kernel_type; a.bk.variance = variance; a.bk.p2 = 0.0;
  if (kernel_type == 1) { a.bk.p1 = p1; a.bk.p2 = p2; }
  else a.bk.p1 = ard_lengthscales ? 1.0 : 1.0 / (p1 * p1);

  GvBuffers buf(ctx);
  double* XT = (double*)buf.get((size_t)d * n * sizeof(double), "greedy_XT");
  if (!XT) return DCGP_ERR_ALLOC;
  double* C = factor_out;
  if (!C && !(C = (double*)buf.get((size_t)k * n * sizeof(double), "greedy_factor"))) return DCGP_ERR_ALLOC;
  double* xn = nullptr;
  if (kernel_type == 1 && !(xn = (double*)buf.get((size_t)n * sizeof(double), "greedy_norms"))) return DCGP_ERR_ALLOC;
  // slots: [2][nwg] maxima, [2][nwg] sums, [2][nwg] indices, then the two state words
  const size_t slot_bytes = (size_t)2 * a.nwg * (2 * sizeof(double) + sizeof(int)) + 2 * sizeof(int);
  char* slots = (char*)buf.get(slot_bytes, "greedy_slots");
  if (!slots) return DCGP_ERR_ALLOC;
  a.X = X; a.XT = XT; a.xn = xn; a.ard = ard_lengthscales; a.C = C; a.resid = residual_out;
  a.slot_max = (double*)slots; a.slot_sum = a.slot_max + 2 * a.nwg; a.slot_idx = (int*)(a.slot_sum + 2 * a.nwg); a.state = a.slot_idx + 2 * a.nwg;
  a.rows = rows_out; a.trace = trace_out;

  HIP_TRY(ctx, hipMemsetAsync(a.state, 0xff, sizeof(int), ctx->stream));       // -1: not stalled
  HIP_TRY(ctx, hipMemsetAsync(a.state + 1, 0, sizeof(int), ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(rows_out, 0xff, (size_t)k * sizeof(int32_t), ctx->stream));   // -1: not selected
  if (factor_out) HIP_TRY(ctx, hipMemsetAsync(factor_out, 0, (size_t)k * n * sizeof(double), ctx->stream));
  hipLaunchKernelGGL(gv_transpose_kernel, dim3((unsigned)((n + 31) / 32), (d + 31) / 32), dim3(256), 0, ctx->stream, X, n, d, ard_lengthscales, XT);
  LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(gv_init_kernel, dim3(a.nwg), dim3(GV_T), 0, ctx->stream, a, xn);
  LAUNCH_CHECK(ctx);
  const size_t lds = (size_t)(d + k) * sizeof(double);
  {
    ScopedTimer t(ctx, "greedy_pivots");
    int rc = DCGP_OK;
    if (kernel_type == 0) rc = gv_launch<0>(ctx, a, lds);
    else if (kernel_type == 1) rc = gv_launch<1>(ctx, a, lds);
    else if (kernel_type == 2) rc = gv_launch<2>(ctx, a, lds);
    else rc = gv_launch<3>(ctx, a, lds);
    if (rc != DCGP_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }   // nothing of this call is in flight when its buffers go
  }
  hipLaunchKernelGGL(gv_finish_kernel, dim3(1), dim3(GV_T), 0, ctx->stream, a);
  LAUNCH_CHECK(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_info, a.state, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *n_greedy_out = ctx->h_info[0];
  if (ctx->h_info[1] != 0)
    return ctx_fail(ctx, DCGP_ERR_ARG, "greedy_variance: non-finite residual at pivot %d (are the candidates finite?)", ctx->h_info[1] - 1);
  return DCGP_OK;
}

// `count` empty launches, each behind the one before on the ctx's stream: what the kernel boundaries of a pivot loop cost by themselves
extern "C" int dcgp_debug_empty_launches(dcgp_ctx* ctx, int count, int wgs, double* ms_out) {
  if (!ctx || !ms_out || count < 1 || wgs < 1) return ctx ? ctx_fail(ctx, DCGP_ERR_ARG, "debug_empty_launches: bad arguments") : DCGP_ERR_ARG;
  hipEvent_t e0, e1;
  HIP_TRY(ctx, hipEventCreate(&e0));
  HIP_TRY(ctx, hipEventCreate(&e1));
  HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
  for (int i = 0; i < count; ++i) hipLaunchKernelGGL(gv_empty_kernel, dim3(wgs), dim3(GV_T), 0, ctx->stream);
  HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
  HIP_TRY(ctx, hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  LAUNCH_CHECK(ctx);
  *ms_out = ms;
  return DCGP_OK;
}

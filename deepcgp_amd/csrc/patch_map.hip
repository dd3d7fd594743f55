// patch_map.hip -- per-patch evidence maps of a patch head: c[n][p][r] = (w_p / P) sum_m k(z_m, x_n[p]) beta[m][r], the head's posterior
// mean split over the P patches of the image (sum_p c[n][p][:] = Kzx^T beta = Fmean).  One launch, K_uf never stored.
//
// A workgroup (4 waves) owns a strip of CS = 64 NY consecutive patch columns g = n P + p of the [N P] column space -- patches of one or
// several images, the last strip ragged.  The strip is staged in LDS as the explicit B operand [Lq][CS] of the sweeps' product
// (sweep_dev.h: rows l < L = sqrt(c) x, row L = 1, row L + 1 = -c |x|^2 / 2 against ZS rows (sqrt(c) z, -c |z|^2 / 2 + log2 variance, 1)),
// so that the gather of sub-step s is `ds_read_b64` at a per-lane base plus a constant: no address arithmetic beside the MFMAs, whatever
// the patch geometry (stride, H != W, channels).  Wave w owns NY column fragments of 16 and walks every 16-row fragment u of Z:
//   1. t[m][p] = sum_k ZS[k][m] B[k][p] on v_mfma_f64_16x16x4_f64 (Lq / 4 sub-steps; ZS through a buffer descriptor from L2, both operands
//      one chunk of 16 / NY sub-steps ahead of their MFMAs), 2^t by exp2_n (common.h);
//   2. the accumulator layout of 1. (lane (lrow, lcol), register v: row m = lrow + 4 v, column p = lcol) IS the A operand of
//      out^T[p][r] += K^T[p][m] beta[m][r] for the four rows m = lrow + 4 v: four MFMAs per block of 16 outputs with B = beta rows from a
//      zero-padded copy [Mp][Rp] -- no shuffle, no LDS round trip.  The result tile has p as rows and r as columns: a fragment's stores
//      are 16 R consecutive doubles of out[N][P][R].
// A strip with a column of c |x|^2 > 2^16 takes the exact form of 1. (kPmExactAbove below).
// Nothing is reduced across waves or workgroups and nothing is accumulated in memory: the result is bit-identical from run to run.
// NY by the strip's LDS image: 4 (Lq <= 32: the 5 x 5 x 1 and 3 x 3 x 3 patches), 2 (Lq <= 68) at two workgroups per CU, else 1 (the
// 5 x 5 x 10 patches: 126 KB, one workgroup per CU -- one wave per SIMD, which is what the prefetch depth is sized for).
#include "common.h"
#include "layer.h"
#include "sweep_dev.h"
#include <cmath>

namespace {

// ---- operands: ZS of the head's Z (zs_task) and beta, zero padded to [Mp][Rp], in one launch ----
struct PmPrepArgs {
  ZsTask zs; int n_zs = 0;                      // items of zs_task (0: ZS is already there)
  const double* beta = nullptr; int R = 0;      // [M][R], or nullptr: beta = LinvT alpha
  const double* LinvT = nullptr;                // [Mp][Mp] inv(L)^T
  const double* alpha = nullptr; int Rpa = 0;   // [Mp][Rpa] inv(L) q_mu (q_mu itself when whitened)
  double* betaP = nullptr; int M = 0, Mp = 0, Rp = 0;
};
__global__ __launch_bounds__(256) void pm_prep_kernel(PmPrepArgs a) {
  __shared__ double zs_t[32][33];
  if ((int)blockIdx.x < a.n_zs) {
    zs_task(a.zs, blockIdx.x, 1 << 30, zs_t);
    return;
  }
  const int idx = ((int)blockIdx.x - a.n_zs) * 256 + threadIdx.x;
  if (idx >= a.Mp * a.Rp) return;
  const int m = idx / a.Rp, r = idx - m * a.Rp;
  double v = 0.0;
  if (m < a.M && r < a.R) {
    if (a.beta) {
      v = a.beta[(long)m * a.R + r];
    } else {   // row m of the upper triangular inv(L)^T against column r of alpha, in index order
      const double* __restrict__ lt = a.LinvT + (long)m * a.Mp;
      for (int k = m; k < a.M; ++k) v = fma(lt[k], a.alpha[(long)k * a.Rpa + r], v);
    }
  }
  a.betaP[idx] = v;
}

struct PatchMapArgs {
  const double* X = nullptr; int n_mod = 0;   // [n_mod][H][W][C]; column g shows image (g / P) % n_mod
  int H = 0, W = 0, C = 0, f = 0, s = 0, Wo = 0, P = 0, L = 0, Lq = 0, HWC = 0;
  const double* ZS = nullptr; int Mp = 0;     // [Lq][Mp]
  double csq = 1.0;
  const double* betaP = nullptr; int R = 0, Rp = 0;   // [Mp][Rp], zero beyond (M, R)
  const double* w = nullptr; double inv_P = 1.0;
  double log2var = 0.0;                        // the exact form's additive term (the MFMA form reads it from ZS row L)
  long NP = 0;                                 // columns
  double* out = nullptr;                       // [NP][R]
};

// The MFMA form accumulates the base-2 exponent t = c (z.x - |z|^2 / 2 - |x|^2 / 2) through partial sums as large as c |x|^2, so where
// the kernel value is not negligible (z near x) its absolute error is a few ulp(c |x|^2) -- measured 2.5 ulp at 250 elements -- and that
// is the value's relative error.  Up to c |x|^2 = 2^16 (ulp 1.5e-11) this stays below 4e-11; a strip with a column above it takes the
// exact form instead: t = -c |x - z|^2 / 2 from the differences themselves on the VALU, no cancellation (several times slower, and only
// met by inputs tens of lengthscales from the origin).
constexpr double kPmExactAbove = 65536.0;

template <int NY>
constexpr int pm_cs() { return 64 * NY; }
template <int NY>
size_t pm_lds(int Lq) {
  return ((size_t)Lq * pm_cs<NY>() + 2 * pm_cs<NY>() + 256) * sizeof(double) + (size_t)((Lq + 1) & ~1) * sizeof(int);
}

template <int NY, int NRB>
__global__ __launch_bounds__(256, NY == 1 ? 1 : 2) void patch_map_kernel(PatchMapArgs a) {
  constexpr int CS = 64 * NY;        // columns of the strip
  constexpr int CK = 16 / NY;        // sub-steps per chunk: 16 MFMAs between the requests of a chunk's operands and their use
  constexpr int KR = 256 / CS;       // staging: rows of the strip written per pass
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int L = a.L, Lq = a.Lq, nk4 = Lq >> 2, nfm = a.Mp >> 4;
  double* Bm = smem;                                      // [Lq][CS]
  double* wcol = Bm + (size_t)Lq * CS;                    // [CS]  w_p / P of the column's patch, 0 beyond the last column
  long* cbase = reinterpret_cast<long*>(wcol + CS);       // [CS]  offset of the patch's first element in X, -1 beyond the last column
  double* sqp = reinterpret_cast<double*>(cbase + CS);    // [256] partial sums of squares
  int* koffs = reinterpret_cast<int*>(sqp + 256);         // [Lq]  offset of patch element l = (kh, kw, c) behind the first one
  const int tid = threadIdx.x, lane = tid & 63, lrow = lane >> 4, lcol = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long g0 = (long)blockIdx.x * CS;
  const int rc0 = (int)blockIdx.y * (16 * NRB);           // first output of this workgroup's block of outputs

  // ---- the strip: tables, then the B operand and its norm rows ----
  for (int col = tid; col < CS; col += 256) {
    const long g = g0 + col;
    const bool in = g < a.NP;
    const long n = in ? g / a.P : 0;
    const int p = in ? (int)(g - n * a.P) : 0;
    const int oh = p / a.Wo, ow = p - oh * a.Wo;
    cbase[col] = in ? (n % a.n_mod) * (long)a.HWC + (long)(oh * a.s * a.W + ow * a.s) * a.C : -1;
    wcol[col] = in ? a.w[p] * a.inv_P : 0.0;
  }
  for (int l = tid; l < Lq; l += 256) {
    const int ll = l < L ? l : 0;
    const int tq = ll / a.C, c = ll - tq * a.C;
    const int kh = tq / a.f, kw = tq - kh * a.f;
    koffs[l] = (kh * a.W + kw) * a.C + c;
  }
  __syncthreads();
  {
    const int col = tid & (CS - 1), kr = tid / CS;
    const long cb = cbase[col];
    const double* __restrict__ xp = a.X + (cb < 0 ? 0 : cb);
    double sq = 0.0;
    for (int k0 = kr; k0 < L; k0 += 8 * KR) {   // 8 loads in flight per thread
      double t[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = k0 + e * KR;
        t[e] = ld_guard(xp, koffs[k < L ? k : 0], k < L && cb >= 0) * a.csq;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = k0 + e * KR;
        if (k < L) Bm[(size_t)k * CS + col] = t[e];
        sq = fma(t[e], t[e], sq);
      }
    }
    sqp[tid] = sq;
  }
  __syncthreads();
  double csq_x2 = 0.0;   // c |x|^2 of column tid
  if (tid < CS) {
    double sq = 0.0;
#pragma unroll
    for (int q = 0; q < KR; ++q) sq += sqp[q * CS + tid];
    csq_x2 = sq;
    Bm[(size_t)L * CS + tid] = 1.0;
    Bm[(size_t)(L + 1) * CS + tid] = -0.5 * sq;
    for (int l = L + 2; l < Lq; ++l) Bm[(size_t)l * CS + tid] = 0.0;
  }
  const bool exact = __syncthreads_or(csq_x2 > kPmExactAbove) != 0;   // (workgroup-uniform)

  // ---- this wave's NY column fragments against every row fragment of Z ----
  const __amdgpu_buffer_rsrc_t zrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(a.ZS), 0, Lq * a.Mp * 8, 0x00020000);
  const int zstep = 4 * a.Mp * 8;
  const int zv0 = (lrow * a.Mp + lcol) * 8;
  const double* bp = Bm + lrow * CS + wave * (16 * NY) + lcol;   // + 16 y + 4 CS s
  const double* __restrict__ btp = a.betaP + (long)lrow * a.Rp + rc0 + lcol;

  d4 outv[NY][NRB];
#pragma unroll
  for (int y = 0; y < NY; ++y)
#pragma unroll
    for (int b = 0; b < NRB; ++b) outv[y][b] = d4{0.0, 0.0, 0.0, 0.0};

  auto loadA = [&](double (&av)[CK], int u, int s0) {
    const int zvo = zv0 + u * 128;
#pragma unroll
    for (int q = 0; q < CK; ++q) {
      const int s = min(s0 + q, nk4 - 1);   // (scalar)
      av[q] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(zrs, zvo, s * zstep, 0));
    }
  };
  auto loadB = [&](double (&bv)[CK][NY], int s0) {
    const double* b0 = bp + (size_t)s0 * (4 * CS);
#pragma unroll
    for (int q = 0; q < CK; ++q) {
      if (s0 + q < nk4) {
#pragma unroll
        for (int y = 0; y < NY; ++y) bv[q][y] = b0[q * (4 * CS) + 16 * y];
      }
    }
  };

  const int nch = (nk4 + CK - 1) / CK;
  double ac[CK], an[CK], bc[CK][NY], bn[CK][NY];
#pragma unroll
  for (int q = 0; q < CK; ++q)
#pragma unroll
    for (int y = 0; y < NY; ++y) bc[q][y] = bn[q][y] = 0.0;
  loadA(ac, 0, 0);
  loadB(bc, 0);
  for (int u = 0; u < nfm; ++u) {
    // rows 16 u + lrow + 4 v of beta: requested here, used behind the fragment's product
    double bt[4][NRB];
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int b = 0; b < NRB; ++b) bt[v][b] = btp[(long)(16 * u + 4 * v) * a.Rp + 16 * b];
    d4 acc[NY];
#pragma unroll
    for (int y = 0; y < NY; ++y) acc[y] = d4{0.0, 0.0, 0.0, 0.0};
    if (exact) {
      // large arguments: rows 16 u + lrow + 4 v against this wave's columns from the differences of the scaled operands
      const double* __restrict__ zp = a.ZS + 16 * u + lrow;
      const double* xq = Bm + wave * (16 * NY) + lcol;
      double sd[NY][4];
#pragma unroll
      for (int y = 0; y < NY; ++y)
#pragma unroll
        for (int v = 0; v < 4; ++v) sd[y][v] = 0.0;
      for (int l = 0; l < L; ++l) {
        double zv[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) zv[v] = zp[(long)l * a.Mp + 4 * v];
#pragma unroll
        for (int y = 0; y < NY; ++y) {
          const double xv = xq[(size_t)l * CS + 16 * y];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const double d = xv - zv[v];
            sd[y][v] = fma(d, d, sd[y][v]);
          }
        }
      }
#pragma unroll
      for (int y = 0; y < NY; ++y)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[y][v] = fma(-0.5, sd[y][v], a.log2var);
    } else
    for (int c = 0; c < nch; ++c) {
      // the operands of the chunk that follows (the first chunk of the next row fragment behind the last one)
      const bool last = c + 1 == nch;
      const int un = last ? min(u + 1, nfm - 1) : u, sn = last ? 0 : (c + 1) * CK;
      loadA(an, un, sn);
      loadB(bn, sn);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < CK; ++q) {
        if (c * CK + q < nk4) {
#pragma unroll
          for (int y = 0; y < NY; ++y) acc[y] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[q], bc[q][y], acc[y], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < CK; ++q) {
        ac[q] = an[q];
#pragma unroll
        for (int y = 0; y < NY; ++y) bc[q][y] = bn[q][y];
      }
    }
    double t[4 * NY];
#pragma unroll
    for (int y = 0; y < NY; ++y)
#pragma unroll
      for (int v = 0; v < 4; ++v) t[4 * y + v] = acc[y][v];
    exp2_n<4 * NY>(t);
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int b = 0; b < NRB; ++b)
#pragma unroll
        for (int y = 0; y < NY; ++y) outv[y][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(t[4 * y + v], bt[v][b], outv[y][b], 0, 0, 0);
  }

  // ---- (w_p / P) and the stores: rows p = lrow + 4 v of the fragment, outputs rc0 + 16 b + lcol ----
#pragma unroll
  for (int y = 0; y < NY; ++y) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int col = wave * (16 * NY) + 16 * y + lrow + 4 * v;
      const long g = g0 + col;
      const double wp = wcol[col];
#pragma unroll
      for (int b = 0; b < NRB; ++b) {
        const int r = rc0 + 16 * b + lcol;
        if (g < a.NP && r < a.R) a.out[g * a.R + r] = outv[y][b][v] * wp;
      }
    }
  }
}

template <int NY, int NRB>
int pm_launch(dcgp_ctx* ctx, const PatchMapArgs& a) {
  const size_t lds = pm_lds<NY>(a.Lq);
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)patch_map_kernel<NY, NRB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const long strips = (a.NP + pm_cs<NY>() - 1) / pm_cs<NY>();
  hipLaunchKernelGGL((patch_map_kernel<NY, NRB>), dim3((unsigned)strips, (unsigned)(a.Rp / (16 * NRB))), dim3(256), lds, ctx->stream, a);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

}  // namespace

// out[rows][P][R] for `rows` images, row n showing X[n % n_mod]; asynchronous on ctx->stream.  ZS == nullptr: built here from Z.
// beta [M][R], or nullptr: beta = LinvT alpha (the head's own factors: alpha = inv(L) q_mu, q_mu itself when whitened).
int patch_map(dcgp_ctx* ctx, const double* X, long rows, int n_mod, const ViewGeom& v, const double* Z, const double* ZS, int M, double variance,
              double lengthscale, const double* w, const double* beta, const double* LinvT, const double* alpha, int Rpa, int R, double* out,
              const std::string& pfx) {
  const int Mp = round_up(M, 16), Lq = sweep_lq(v.L);
  const int NRB = R > 16 ? 2 : 1, Rp = round_up(R, 16 * NRB);
  const long NP = rows * v.P;
  if (pm_lds<1>(Lq) > 160 * 1024) return ctx_fail(ctx, DCGP_ERR_ARG, "patch_mean: patches of %d elements exceed the strip's LDS image", v.L);
  if ((long)Lq * Mp * 8 >= (1L << 31) || (NP + 63) / 64 >= (1L << 31) || Rp / 16 > 65535)
    return ctx_fail(ctx, DCGP_ERR_ARG, "patch_mean: problem too large (M %d, columns %ld, outputs %d)", M, NP, R);
  ScopedTimer tm(ctx, "patch_map");
  double* betaP = (double*)ws_get(ctx, pfx + "pm_beta", (size_t)Mp * Rp * sizeof(double));
  if (!betaP) return DCGP_ERR_ALLOC;
  PmPrepArgs p;
  if (!ZS) {
    double* zs = (double*)ws_get(ctx, pfx + "pm_ZS", (size_t)Lq * Mp * sizeof(double));
    if (!zs) return DCGP_ERR_ALLOC;
    p.zs.Z = Z; p.zs.ZS = zs; p.zs.M = M; p.zs.Mp = Mp; p.zs.L = v.L; p.zs.Lq = Lq;
    p.zs.csq = sqrt(1.4426950408889634074) / lengthscale; p.zs.log2var = log2(variance);
    p.n_zs = zs_items(Mp, v.L);
    ZS = zs;
  }
  p.beta = beta; p.R = R; p.LinvT = LinvT; p.alpha = alpha; p.Rpa = Rpa; p.betaP = betaP; p.M = M; p.Mp = Mp; p.Rp = Rp;
  hipLaunchKernelGGL(pm_prep_kernel, dim3(p.n_zs + (Mp * Rp + 255) / 256), dim3(256), 0, ctx->stream, p);
  LAUNCH_CHECK(ctx);
  PatchMapArgs a;
  a.X = X; a.n_mod = n_mod;
  a.H = v.H; a.W = v.W; a.C = v.C; a.f = v.f; a.s = v.s; a.Wo = v.Wo; a.P = v.P; a.L = v.L; a.Lq = Lq; a.HWC = v.H * v.W * v.C;
  a.ZS = ZS; a.Mp = Mp; a.csq = sqrt(1.4426950408889634074) / lengthscale;
  a.betaP = betaP; a.R = R; a.Rp = Rp; a.w = w; a.inv_P = 1.0 / (double)v.P; a.log2var = log2(variance); a.NP = NP; a.out = out;
  const int ny = pm_lds<4>(Lq) <= 72 * 1024 ? 4 : (pm_lds<2>(Lq) <= 72 * 1024 ? 2 : 1);
  if (NRB == 1) return ny == 4 ? pm_launch<4, 1>(ctx, a) : (ny == 2 ? pm_launch<2, 1>(ctx, a) : pm_launch<1, 1>(ctx, a));
  return ny == 4 ? pm_launch<4, 2>(ctx, a) : (ny == 2 ? pm_launch<2, 2>(ctx, a) : pm_launch<1, 2>(ctx, a));
}

extern "C" int dcgp_convkernel_patch_mean(dcgp_ctx* ctx, const double* X, int N, int H, int W, int C, int f, int stride, const double* Z, int M,
                                          double variance, double lengthscale, const double* w, const double* beta, int R, double* out_NPR) {
  if (!ctx) return DCGP_ERR_ARG;
  if (!(N >= 0 && M > 0 && R >= 1 && f > 0 && stride > 0 && H > 0 && W > 0 && C > 0 && f <= H && f <= W && variance > 0 && lengthscale > 0))
    return ctx_fail(ctx, DCGP_ERR_ARG, "convkernel_patch_mean: bad args (N %d, H %d, W %d, C %d, f %d, stride %d, M %d, R %d)", N, H, W, C, f, stride, M, R);
  if (N == 0) return DCGP_OK;
  if (!(X && Z && w && beta && out_NPR)) return ctx_fail(ctx, DCGP_ERR_ARG, "convkernel_patch_mean: NULL pointer");
  ViewGeom v;
  v.set(H, W, C, f, stride);
  DCGP_TRY(patch_map(ctx, X, N, N, v, Z, nullptr, M, variance, lengthscale, w, beta, nullptr, nullptr, 0, R, out_NPR, "op_"));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

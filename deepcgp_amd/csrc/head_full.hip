// head_full.hip -- full covariances of the classification head (prediction only, off the training path).
//
//   * pair_conv_kernel   : ConvKernel.K          (conv_gp/kernels.py:81-104)
//                          K[b,n,n'] = (1/P^2) sum_{p,p'} w_p w_p' k(x_{n,p}, x2_{n',p'})
//   * pair_add_kernel    : AdditivePatchKernel.K (conv_gp/kernels.py:34-51)
//                          K[b,n,n'] = (1/P) sum_p w_p k(x_{n,p}, x2_{n',p})
//   * reparam_full_kernel: doubly_stochastic_dgp.utils.reparameterize(full_cov=True) for S x D matrices at once
//
// The image-pair Gram never materialises the NP x N2P patch Gram matrix.  One workgroup takes one image pair (n, n') -- or a
// contiguous range of its 64-row patch tiles when there are few pairs -- stages both images in LDS and walks 64 x 64 tiles of
// the pair's P x P patch Gram: the cross term x.x' on v_mfma_f64_16x16x4_f64 with both operands gathered from LDS through
// patch_base + koff (the layout of head_kdiag_body, rbf.hip), the kernel value as 2^t with
//     t = c x.x' + h_n[p] + h'_{n'}[p'] (+ log2 variance),   c = log2(e) / l^2,   h[p] = -c |x_p|^2 / 2
// (h: one per-image pass, pair_norms_kernel), weighted and summed in registers.  Partial sums of a pair go to their own slots
// and are added in a fixed order by pair_reduce_kernel: no atomics, two calls give the same bits.  With X2 == NULL only the
// pairs n <= n' run (a pair of an image with itself uses the symmetry of its patch Gram, as Kdiag does) and the reduction stores
// every value at [n][n'] and [n'][n], so K equals K^T bit for bit.
#include "common.h"

namespace {

constexpr int KP_T = 64;   // patch tile (rows and columns)

__device__ __forceinline__ int pbase(int p, int P, int Wo, int s, int W, int C) {
  if (p >= P) p = 0;
  const int oh = p / Wo, ow = p - oh * Wo;
  return (oh * s * W + ow * s) * C;
}

// h[img][p] = -c |x_q|^2 / 2 for every image of the launch and p < Pp, q = the patch the sweep gathers for p (pbase: patch 0 beyond P).
// A padding row or column thus evaluates a true kernel value (<= variance) that its zero weight removes; with h = 0 there it would be
// 2^(c x_0.x') unbounded -- inf once the argument passes 1024, and 0 * inf = NaN in the weighted sum.  grid: images, 256 threads.
__global__ __launch_bounds__(256) void pair_norms_kernel(const double* __restrict__ X, int H, int W, int C, int f, int s, int Wo, int P,
                                                          int L, int Pp, double c, double* __restrict__ h) {
  const long img = blockIdx.x;
  const double* __restrict__ x = X + img * (long)H * W * C;
  for (int p = threadIdx.x; p < Pp; p += 256) {
    double acc = 0.0;
    const int pb = pbase(p, P, Wo, s, W, C);
    for (int l = 0; l < L; ++l) {
      const int cc = l % C, t = l / C, kw = t % f, kh = t / f;
      const double v = x[pb + (kh * W + kw) * C + cc];
      acc = fma(v, v, acc);
    }
    h[img * Pp + p] = -0.5 * c * acc;
  }
}

struct PairArgs {
  const double* X = nullptr; const double* X2 = nullptr;   // [B][N][H][W][C], [B][N2][H][W][C] (X2 == X when sym)
  const double* h1 = nullptr; const double* h2 = nullptr;  // [B][N][Pp], [B][N2][Pp]
  const double* w = nullptr;                               // [P]
  const double* etab = nullptr;                            // 2^(j / 256), j < 256 (exp2_table)
  double* partial = nullptr;                               // [B][npairs][nsplit]
  int N = 0, N2 = 0, H = 0, W = 0, C = 0, f = 0, s = 0, Wo = 0, P = 0, L = 0, Lp = 0, p_tiles = 0, nsplit = 1, sym = 0;
  long npairs = 0;
  double c = 1.0, log2var = 0.0;
};

// pair q -> (n, n'): n <= n' enumerated column by column (sym), or row-major over N x N2
__device__ __forceinline__ void pair_decode(const PairArgs& a, long q, int& n, int& n2) {
  if (a.sym) {
    long j = (long)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
    while (j * (j + 1) / 2 > q) --j;
    while ((j + 1) * (j + 2) / 2 <= q) ++j;
    n2 = (int)j;
    n = (int)(q - j * (j + 1) / 2);
  } else {
    n = (int)(q / a.N2);
    n2 = (int)(q % a.N2);
  }
}

// image [HWC] of X + off -> LDS, 8 loads in flight per thread
__device__ __forceinline__ void stage_image(const double* __restrict__ x, int HWC, double* img) {
  for (int i0 = 0; i0 < HWC; i0 += 8 * 256) {
    double t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = i0 + e * 256 + (int)threadIdx.x;
      t[e] = x[i < HWC ? i : 0];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = i0 + e * 256 + (int)threadIdx.x;
      if (i < HWC) img[i] = t[e];
    }
  }
}

// one workgroup = one image pair and one range of its tile rows; 4 waves as 2 (rows) x 2 (columns) of 32 x 32 per tile
__global__ __launch_bounds__(256, 2) void pair_conv_kernel(PairArgs a) {
  const long g = blockIdx.x;
  const int split = (int)(g % a.nsplit);
  const long q = (g / a.nsplit) % a.npairs;
  const int b = (int)(g / ((long)a.nsplit * a.npairs));
  int n, n2;
  pair_decode(a, q, n, n2);
  const bool self = a.sym && n == n2;
  const int H = a.H, W = a.W, C = a.C, s = a.s, Wo = a.Wo, P = a.P, L = a.L, Lp = a.Lp, p_tiles = a.p_tiles;
  const int HWC = H * W * C, HWCp = (HWC + 1) & ~1, Pp = p_tiles * KP_T;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* img1 = smem;                                   // [HWCp]
  double* img2 = self ? img1 : img1 + HWCp;              // [HWCp]
  double* h1s = img1 + 2 * HWCp;                         // [Pp]  h of image n + log2 variance
  double* h2s = h1s + Pp;                                // [Pp]
  double* wl = h2s + Pp;                                 // [Pp]  weights, 0 beyond P
  double* etab = wl + Pp;                                // [256]
  double* red = etab + 256;                              // [4]
  int* koff = reinterpret_cast<int*>(red + 4);           // [Lp]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lrow = lane >> 4, lcol = lane & 15;

  stage_image(a.X + ((long)b * a.N + n) * HWC, HWC, img1);
  if (!self) stage_image(a.X2 + ((long)b * a.N2 + n2) * HWC, HWC, img2);
  const double* __restrict__ h1g = a.h1 + ((long)b * a.N + n) * Pp;
  const double* __restrict__ h2g = a.h2 + ((long)b * a.N2 + n2) * Pp;
  for (int p = tid; p < Pp; p += 256) {
    h1s[p] = h1g[p] + a.log2var;
    h2s[p] = h2g[p];
    wl[p] = p < P ? a.w[p] : 0.0;
  }
  etab[tid] = a.etab[tid];
  for (int l = tid; l < Lp; l += 256) {
    const int ll = l < L ? l : 0;
    const int cc = ll % C, t = ll / C, kw = t % a.f, kh = t / a.f;
    koff[l] = (kh * W + kw) * C + cc;
  }
  __syncthreads();

  const int r0 = (int)((long)split * p_tiles / a.nsplit), r1 = (int)((long)(split + 1) * p_tiles / a.nsplit);
  const int nk4 = Lp >> 2;
  const bool last_in = 4 * (nk4 - 1) + lrow < L;
  const double c = a.c;
  double sum = 0.0;
  for (int tr = r0; tr < r1; ++tr) {
    int pa[2];
    double hr[2][4], wr[2][4], rs[2][4];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      pa[x] = pbase(tr * KP_T + wm * 32 + x * 16 + lcol, P, Wo, s, W, C);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int p = tr * KP_T + wm * 32 + x * 16 + lrow + 4 * v;
        hr[x][v] = h1s[p]; wr[x][v] = wl[p]; rs[x][v] = 0.0;
      }
    }
    for (int tc = self ? tr : 0; tc < p_tiles; ++tc) {
      int pbc[2];
#pragma unroll
      for (int y = 0; y < 2; ++y) pbc[y] = pbase(tc * KP_T + wn * 32 + y * 16 + lcol, P, Wo, s, W, C);
      d4 acc[2][2];
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = d4{0.0, 0.0, 0.0, 0.0};
      // operands gathered one k sub-step ahead of the MFMAs that use them, their offsets a group of four sub-steps ahead
      // (head_kdiag_body: offset -> gather -> MFMA in one step exposes two dependent LDS round trips per step)
      auto offs = [&](int k4, int (&ko)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) ko[u] = koff[4 * min(k4 + u, nk4 - 1) + lrow];
      };
      auto gather = [&](int ko, bool kin, double (&av)[2], double (&bv)[2]) {
#pragma unroll
        for (int x = 0; x < 2; ++x) { const double v = img1[pa[x] + ko]; av[x] = kin ? v : 0.0; }
#pragma unroll
        for (int y = 0; y < 2; ++y) { const double v = img2[pbc[y] + ko]; bv[y] = kin ? v : 0.0; }
      };
      auto mma = [&](const double (&av)[2], const double (&bv)[2]) {
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
          for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x], bv[y], acc[x][y], 0, 0, 0);
      };
      int kc[4], kn[4];
      double ac[2], bc[2], an[2], bn[2];
      offs(0, kc);
      gather(kc[0], nk4 > 1 || last_in, ac, bc);
      int k4 = 0;
      for (; k4 + 4 < nk4; k4 += 4) {
        offs(k4 + 4, kn);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (u < 3) gather(kc[u + 1], true, an, bn);
          else gather(kn[0], k4 + 4 < nk4 - 1 || last_in, an, bn);
          mma(ac, bc);
#pragma unroll
          for (int x = 0; x < 2; ++x) { ac[x] = an[x]; bc[x] = bn[x]; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) kc[u] = kn[u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (k4 + u < nk4) {
          if (u < 3 && k4 + u + 1 < nk4) gather(kc[u + 1], k4 + u + 1 < nk4 - 1 || last_in, an, bn);
          mma(ac, bc);
#pragma unroll
          for (int x = 0; x < 2; ++x) { ac[x] = an[x]; bc[x] = bn[x]; }
        }
      const double sym = (self && tc != tr) ? 2.0 : 1.0;
#pragma unroll
      for (int y = 0; y < 2; ++y) {
        const int pc = tc * KP_T + wn * 32 + y * 16 + lcol;
        const double hc = h2s[pc], wc = sym * wl[pc];
#pragma unroll
        for (int x = 0; x < 2; ++x) {
          double t[4];
#pragma unroll
          for (int v = 0; v < 4; ++v) t[v] = fma(acc[x][y][v], c, hr[x][v] + hc);
          exp2_tab_n<4>(t, etab);
#pragma unroll
          for (int v = 0; v < 4; ++v) rs[x][v] = fma(wc, t[v], rs[x][v]);
        }
      }
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int v = 0; v < 4; ++v) sum = fma(wr[x][v], rs[x][v], sum);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (tid == 0) a.partial[g] = (red[0] + red[1]) + (red[2] + red[3]);
}

// additive mode: one workgroup per image pair, patch p by thread p mod 256
__global__ __launch_bounds__(256) void pair_add_kernel(PairArgs a) {
  const long g = blockIdx.x;
  const long q = g % a.npairs;
  const int b = (int)(g / a.npairs);
  int n, n2;
  pair_decode(a, q, n, n2);
  const int W = a.W, C = a.C, HWC = a.H * W * C, HWCp = (HWC + 1) & ~1, Pp = a.p_tiles * KP_T;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* img1 = smem;
  double* img2 = img1 + HWCp;
  double* red = img2 + HWCp;                       // [4]
  int* koff = reinterpret_cast<int*>(red + 4);     // [L]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  stage_image(a.X + ((long)b * a.N + n) * HWC, HWC, img1);
  stage_image(a.X2 + ((long)b * a.N2 + n2) * HWC, HWC, img2);
  for (int l = tid; l < a.L; l += 256) {
    const int cc = l % C, t = l / C, kw = t % a.f, kh = t / a.f;
    koff[l] = (kh * W + kw) * C + cc;
  }
  __syncthreads();
  const double* __restrict__ h1g = a.h1 + ((long)b * a.N + n) * Pp;
  const double* __restrict__ h2g = a.h2 + ((long)b * a.N2 + n2) * Pp;
  double sum = 0.0;
  for (int p = tid; p < a.P; p += 256) {
    const int pb = pbase(p, a.P, a.Wo, a.s, W, C);
    double dot = 0.0;
    for (int l = 0; l < a.L; ++l) dot = fma(img1[pb + koff[l]], img2[pb + koff[l]], dot);
    double t[1] = {fma(dot, a.c, (h1g[p] + a.log2var) + h2g[p])};
    exp2_n<1>(t);
    sum = fma(a.w[p], t[0], sum);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (tid == 0) a.partial[g] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[b][n][n'] = scale * (partial slots of the pair, in order); sym: also [n'][n]
__global__ void pair_reduce_kernel(PairArgs a, double scale, double* __restrict__ out) {
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (q >= a.npairs) return;
  int n, n2;
  pair_decode(a, q, n, n2);
  const double* pp = a.partial + ((long)b * a.npairs + q) * a.nsplit;
  double sum = 0.0;
  for (int i = 0; i < a.nsplit; ++i) sum += pp[i];
  const double v = sum * scale;
  double* ob = out + (long)b * a.N * a.N2;
  ob[(long)n * a.N2 + n2] = v;
  if (a.sym && n != n2) ob[(long)n2 * a.N2 + n] = v;
}

// out[s,:,d] = mean[s,:,d] + chol(var[s,:,:,d] + jitter I) z[s,:,d]; one workgroup per (s, d), the factor in LDS (N <= 128).
// info[s * D + d] = 0, or the 1-based column of the first pivot that is not positive (the matrix's output is then not written).
__global__ __launch_bounds__(256) void reparam_full_kernel(const double* __restrict__ mean, const double* __restrict__ var,
                                                           const double* __restrict__ z, int N, int D, double jitter,
                                                           double* __restrict__ out, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* A = smem;            // [N][N] row-major, lower triangle used
  double* zs = A + N * N;      // [N]
  __shared__ int fail;
  const int sd = blockIdx.x, s_ = sd / D, d = sd % D, tid = threadIdx.x;
  const long base = (long)s_ * N * N * D + d;
  for (int e = tid; e < N * N; e += 256) {
    const int i = e / N, j = e % N;
    A[e] = j <= i ? var[base + (long)e * D] + (i == j ? jitter : 0.0) : 0.0;
  }
  for (int i = tid; i < N; i += 256) zs[i] = z[((long)s_ * N + i) * D + d];
  if (tid == 0) fail = 0;
  __syncthreads();
  for (int k = 0; k < N; ++k) {
    const double piv = A[k * N + k];
    if (!(piv > 0.0)) {   // also NaN
      if (tid == 0) fail = k + 1;
      break;
    }
    const double dk = sqrt(piv);
    __syncthreads();   // every thread has read the pivot
    for (int i = k + 1 + tid; i < N; i += 256) A[i * N + k] /= dk;
    if (tid == 0) A[k * N + k] = dk;
    __syncthreads();
    const int m = N - k - 1;
    for (int e = tid; e < m * m; e += 256) {
      const int i = k + 1 + e / m, j = k + 1 + e % m;
      if (j <= i) A[i * N + j] = fma(-A[i * N + k], A[j * N + k], A[i * N + j]);
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid == 0) info[sd] = fail;
  if (fail) return;
  for (int i = tid; i < N; i += 256) {
    double acc = 0.0;
    for (int j = 0; j <= i; ++j) acc = fma(A[i * N + j], zs[j], acc);
    const long o = ((long)s_ * N + i) * D + d;
    out[o] = mean[o] + acc;
  }
}

}  // namespace

extern "C" {

#define HF_ARG(cond, msg) \
  if (!(cond)) return ctx ? ctx_fail(ctx, DCGP_ERR_ARG, msg) : DCGP_ERR_ARG

int dcgp_convkernel_k(dcgp_ctx* ctx, const double* X, const double* X2, int B, int N, int N2, int H, int W, int C, int f, int stride,
                      double variance, double lengthscale, const double* w, int additive, double* out) {
  HF_ARG(ctx && X && w && out && B > 0 && N > 0 && f > 0 && stride > 0 && f <= H && f <= W && C > 0 && variance > 0 &&
             lengthscale > 0, "convkernel_k: bad args");
  const bool sym = X2 == nullptr;
  if (sym) N2 = N;
  HF_ARG(N2 > 0, "convkernel_k: N2 must be positive");
  const int Ho = (H - f) / stride + 1, Wo = (W - f) / stride + 1, P = Ho * Wo, L = f * f * C;
  PairArgs a;
  a.X = X; a.X2 = sym ? X : X2; a.w = w;
  a.N = N; a.N2 = N2; a.H = H; a.W = W; a.C = C; a.f = f; a.s = stride; a.Wo = Wo; a.P = P; a.L = L; a.Lp = (L + 3) & ~3;
  a.p_tiles = (P + KP_T - 1) / KP_T; a.sym = sym ? 1 : 0;
  a.npairs = sym ? (long)N * (N + 1) / 2 : (long)N * N2;
  a.c = 1.4426950408889634074 / (lengthscale * lengthscale);
  a.log2var = log2(variance);
  const int Pp = a.p_tiles * KP_T, HWC = H * W * C, HWCp = (HWC + 1) & ~1;
  // few pairs: a pair's tile rows shared by up to p_tiles workgroups so that the launch fills the chip (about 8 workgroups per CU)
  const long want = 8L * ctx->n_cus;
  const long base_wgs = (long)B * a.npairs;
  a.nsplit = additive ? 1 : (int)std::max(1L, std::min((long)a.p_tiles, (want + base_wgs - 1) / base_wgs));
  const long nwg = base_wgs * a.nsplit;
  // the dispatch grid counts work-items in 32 bits: workgroups x 256 < 2^32
  HF_ARG(nwg * 256 < (1L << 32) && (long)B * N * 256 < (1L << 32) && (long)B * N2 * 256 < (1L << 32) && B <= 65535 &&
             (long)B * N * Pp < (1L << 31) && (long)B * N2 * Pp < (1L << 31),
         "convkernel_k: problem too large (more than 2^24 workgroups, or a batch of more than 2^31 patch slots)");
  size_t lds;
  if (additive) lds = (size_t)(2 * HWCp + 4) * sizeof(double) + (size_t)L * sizeof(int);
  else lds = (size_t)(2 * HWCp + 3 * Pp + 256 + 4) * sizeof(double) + (size_t)a.Lp * sizeof(int);
  HF_ARG(lds <= 160 * 1024, "convkernel_k: two images and their patch tables do not fit LDS");
  double* h1 = (double*)ws_get(ctx, "hf_h1", (size_t)B * N * Pp * sizeof(double));
  double* h2 = sym ? h1 : (double*)ws_get(ctx, "hf_h2", (size_t)B * N2 * Pp * sizeof(double));
  double* partial = (double*)ws_get(ctx, "hf_partial", (size_t)nwg * sizeof(double));
  if (!h1 || !h2 || !partial) return DCGP_ERR_ALLOC;
  a.h1 = h1; a.h2 = h2; a.partial = partial;
  if (!additive) {
    a.etab = exp2_table(ctx);
    if (!a.etab) return DCGP_ERR_ALLOC;
  }
  ScopedTimer t(ctx, "convkernel_k");
  hipLaunchKernelGGL(pair_norms_kernel, dim3((unsigned)(B * N)), dim3(256), 0, ctx->stream, X, H, W, C, f, stride, Wo, P, L, Pp, a.c, h1);
  LAUNCH_CHECK(ctx);
  if (!sym) {
    hipLaunchKernelGGL(pair_norms_kernel, dim3((unsigned)(B * N2)), dim3(256), 0, ctx->stream, X2, H, W, C, f, stride, Wo, P, L, Pp, a.c, h2);
    LAUNCH_CHECK(ctx);
  }
  if (additive) {
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)pair_add_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(pair_add_kernel, dim3((unsigned)nwg), dim3(256), lds, ctx->stream, a);
  } else {
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)pair_conv_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(pair_conv_kernel, dim3((unsigned)nwg), dim3(256), lds, ctx->stream, a);
  }
  LAUNCH_CHECK(ctx);
  const double scale = additive ? 1.0 / (double)P : 1.0 / ((double)P * (double)P);
  hipLaunchKernelGGL(pair_reduce_kernel, dim3((unsigned)((a.npairs + 255) / 256), (unsigned)B), dim3(256), 0, ctx->stream, a, scale, out);
  LAUNCH_CHECK(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

int dcgp_reparam_full_cov(dcgp_ctx* ctx, const double* mean, const double* var, const double* z, int S, int N, int D,
                          double jitter, double* out, int* info_host) {
  HF_ARG(ctx && mean && var && z && out && S > 0 && N > 0 && D > 0, "reparam_full_cov: bad args");
  if (info_host) *info_host = 0;
  if (N > 128) return ctx_fail(ctx, DCGP_ERR_ARG, "reparam_full_cov: N = %d exceeds the 128 rows a factor in LDS holds", N);
  const long nmat = (long)S * D;
  HF_ARG(nmat * 256 < (1L << 32), "reparam_full_cov: too many matrices");
  int* d_info = (int*)ws_get(ctx, "hf_reparam_info", (size_t)nmat * sizeof(int));
  if (!d_info) return DCGP_ERR_ALLOC;
  const size_t lds = (size_t)(N * N + N) * sizeof(double);
  ScopedTimer t(ctx, "reparam_full_cov");
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)reparam_full_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(reparam_full_kernel, dim3((unsigned)nmat), dim3(256), lds, ctx->stream, mean, var, z, N, D, jitter, out, d_info);
  LAUNCH_CHECK(ctx);
  std::vector<int> info(nmat);
  HIP_TRY(ctx, hipMemcpyAsync(info.data(), d_info, (size_t)nmat * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (long i = 0; i < nmat; ++i)
    if (info[i]) {
      if (info_host) *info_host = info[i];
      return ctx_fail(ctx, DCGP_ERR_NOT_PD, "reparam_full_cov: matrix (sample %ld, output %ld) not positive definite at column %d",
                      i / D, i % D, info[i]);
    }
  return DCGP_OK;
}

}  // extern "C"

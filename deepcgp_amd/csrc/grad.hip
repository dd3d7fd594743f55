// grad.hip -- reverse pass of the ELBO (the reference gets it from TensorFlow autodiff of the graph it
// builds at conv_gp/experiment.py:84-108).  Runs over the state the forward pass (model.hip) left on the device:
// every layer's K_uf and A1 = inv(L) K_uf, the factors and their inverses, G_r / alpha, and the per-layer
// (sample, mean, var).  Per layer, given d ELBO / d(mean, var) of its outputs:
//
//   conditional   mean = alpha^T A1,  var = Knn - sum_m A1^2 + sum_m (G_r^T A1)^2   (the forward's re-association)
//     dT_r = 2 (G_r^T A1) o dvar_r        d alpha = A1 dmean        dG_r = tril(A1 dT_r^T) = tril(2 A1 diag(dvar_r) A1^T G_r)
//     dA1  = alpha dmean^T - 2 A1 o sum_r dvar_r + sum_r G_r dT_r
//     unwhitened: dq_mu = inv(L)^T d alpha, dq_sqrt_r = tril(inv(L)^T dG_r), dL -= tril(dq_mu alpha^T + sum_r (inv(L)^T dG_r) G_r^T)
//     dKuf = inv(L)^T dA1,  dL -= tril(dKuf A1^T)
//   Cholesky      S = inv(L)^T Phi(L^T dL) inv(L)   (Phi: lower triangle, diagonal halved; Murray 2016), used unsymmetrised
//   kernels       E = dK o K:  dvariance = sum E / variance, dlengthscale = sum E d^2 / l^3,
//                 dZ = (E X - rowsum(E) o Z) / l^2,  dX = (E^T Z - colsum(E) o X) / l^2  on im2col'd patches, col2im gather
//   KL            closed form in inv(K) (no second Cholesky adjoint), sample: dmean += dF, dvar += dF (F - mean) / (2 (var + jitter))
//
// The R M^2 K products that fit the forward's tuned kernel run on it (gemm.hip: dT with a column-scaled store, dA1 as one
// launch with the R blocks stacked along k, dK_uf); everything else goes through gemm_gen (strided MFMA GEMM, deterministic
// split-k, the adjoints' corrections in its epilogue) and elementwise / reduction kernels.
// Scheduling (Lanes, below): the main stream carries the data path only -- the column-wise adjoint of each conditional, the patch-kernel
// adjoint, dX for the layer below; the conditional's M x M chain (W_r -> dG_r -> dq_sqrt -> dL -> Cholesky adjoint -> S) runs on a second
// stream, what needs S (Gram adjoint of K_uu, scalar sums) and the KL pieces on a third; zero fills, parameter-only operands and the KL
// adjoint's products are enqueued beside the FORWARD pass (grad_kl_early).  Every buffer two streams touch is ordered by an event; the main
// stream joins the others once, at the end of the step.  No atomics anywhere: the gradients are reproducible run to run
// (tests: test_gradients_repeat_in_steady_state).  The oracle for this file is oracle/grad.py.
#include <algorithm>
#include <chrono>
#include <initializer_list>

#include "model_state.h"
#include "gemm_gen.h"

namespace {

constexpr int VAR_SLOT = 0, LS_SLOT = 16, P2_SLOT = 32;   // gslots: [0,16) variance, [16,32) lengthscale | acos weight variance, [32,48) acos bias variance

inline unsigned blocks_for(long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

__device__ __forceinline__ double block_sum_256(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// ---- likelihood ------------------------------------------------------------------------------------------------
// d sum_rows weight * ve(row) / d(mu, var).  Same quadrature as varexp_kernel (cond.hip): 20 Gauss-Hermite nodes,
// cdf = (1 - 2e-4) Phi + 1e-4, clips at 1e-10.  One thread per (row, node) evaluates the node's terms for every class
// into LDS; one thread per (row, class) then adds the 20 nodes in a fixed order.  RM_ROWS rows per 256-thread block.
constexpr int RM_ROWS = 12, RM_KMAX = 16;
__global__ __launch_bounds__(256) void robustmax_grad_kernel(const double* __restrict__ mu, const double* __restrict__ var, const int32_t* __restrict__ y,
                                                             int rows, int n_labels, int K, double eps, const double* __restrict__ gh, double weight,
                                                             double* __restrict__ gm, double* __restrict__ gv) {
  __shared__ double tm[RM_ROWS][20][RM_KMAX], tv[RM_ROWS][20][RM_KMAX];
  const int t = threadIdx.x, lr = t / 20, g = t % 20;
  const int row = blockIdx.x * RM_ROWS + lr;
  const double inv_sqrt_pi = 0.56418958354775628695, inv_sqrt_2pi = 0.39894228040143267794;
  if (lr < RM_ROWS && row < rows) {
    const int lab = y[row % n_labels];
    const double* m = mu + (long)row * K;
    const double* v = var + (long)row * K;
    const double vy = v[lab];
    const bool live_y = 2.0 * vy > 1e-10;
    const double sy = sqrt(fmax(2.0 * vy, 1e-10));
    const double xg = gh[g], wg = gh[20 + g] * inv_sqrt_pi;
    const double X = m[lab] + xg * sy;
    double prod = 1.0;
    for (int k = 0; k < K; ++k) {
      if (k == lab) continue;
      const double d = (X - m[k]) / sqrt(fmax(v[k], 1e-10));
      prod *= 0.5 * (1.0 + erf(d * 0.70710678118654752440)) * (1.0 - 2e-4) + 1e-4;
    }
    double qs = 0.0;
    for (int k = 0; k < K; ++k) {
      if (k == lab) continue;
      const double sig = sqrt(fmax(v[k], 1e-10));
      const double d = (X - m[k]) / sig;
      const double cdf = 0.5 * (1.0 + erf(d * 0.70710678118654752440)) * (1.0 - 2e-4) + 1e-4;
      const double q = wg * prod / cdf * exp(-0.5 * d * d) * inv_sqrt_2pi * (1.0 - 2e-4);
      tm[lr][g][k] = -q / sig;
      tv[lr][g][k] = v[k] > 1e-10 ? -q * d / (2.0 * v[k]) : 0.0;
      qs += q / sig;
    }
    tm[lr][g][lab] = qs;
    tv[lr][g][lab] = live_y ? qs * xg / sy : 0.0;
  }
  __syncthreads();
  const double c = log(1.0 - eps) - log(eps / (K - 1.0));
  for (int idx = t; idx < RM_ROWS * K; idx += 256) {
    const int r2 = idx / K, k = idx % K, row2 = blockIdx.x * RM_ROWS + r2;
    if (row2 >= rows) continue;
    double a = 0.0, b = 0.0;
    for (int gg = 0; gg < 20; ++gg) { a += tm[r2][gg][k]; b += tv[r2][gg][k]; }
    gm[(long)row2 * K + k] = c * weight * a;
    gv[(long)row2 * K + k] = c * weight * b;
  }
}

// GT[(r * Mp + k) * Mp + i] = G[r][i][k]: the R transposes stacked along k (pads included)
__global__ void restack_transpose_kernel(const double* __restrict__ G, int Mp, int R, double* __restrict__ GT) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long mm = (long)Mp * Mp;
  if (idx >= mm * R) return;
  const int r = (int)(idx / mm);
  const int k = (int)((idx % mm) / Mp), i = (int)(idx % Mp);
  GT[idx] = G[r * mm + (long)i * Mp + k];
}

// previous layer's (dmean, dvar) from d sample:  sample = mean + z sqrt(var + jitter),  z = (sample - mean) / sqrt(var + jitter)
__global__ void sample_backward_kernel(const double* __restrict__ dF, const double* __restrict__ sample, const double* __restrict__ mean,
                                       const double* __restrict__ var, double jitter, long n, double* __restrict__ gm,
                                       double* __restrict__ gv) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double d = dF[i];
  gm[i] = d;
  gv[i] = d * (sample[i] - mean[i]) / (2.0 * (var[i] + jitter));
}

// the same for a de-duplicated first layer, whose S samples share one conditional: the S gradients arriving per element add up
// (gm[i] = sum_s of the kernel above at s * n + i, in the order s = 0, 1, ...)
__global__ void sample_backward_dedup_kernel(const double* __restrict__ dF, const double* __restrict__ sample, const double* __restrict__ mean,
                                             const double* __restrict__ var, double jitter, int S, long n, double* __restrict__ gm,
                                             double* __restrict__ gv) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double sa = 0.0, sb = 0.0;
  for (int s = 0; s < S; ++s) {
    const long k = (long)s * n + i;
    const double d = dF[k];
    sa += d;
    sb += d * (sample[k] - mean[k]) / (2.0 * (var[k] + jitter));
  }
  gm[i] = sa;
  gv[i] = sb;
}

// out[i] = sum_s in[s * n + i]: the S samples of a de-duplicated first layer share one conditional
__global__ void reduce_replicas_kernel(const double* __restrict__ a, const double* __restrict__ b, int S, long n, double* __restrict__ oa,
                                       double* __restrict__ ob) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double sa = 0.0, sb = 0.0;
  for (int s = 0; s < S; ++s) { sa += a[(long)s * n + i]; sb += b[(long)s * n + i]; }
  oa[i] = sa;
  ob[i] = sb;
}

// ---- conditional -----------------------------------------------------------------------------------------------
__global__ void rowsum_small_kernel(const double* __restrict__ a, long n, int R, double* __restrict__ out) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  double s = 0.0;
  for (int r = 0; r < R; ++r) s += a[c * R + r];
  out[c] = s;
}

// dA1[m][c] -= 2 A1[m][c] gvs[c]
__global__ void dA1_fix_kernel(double* __restrict__ dA1, const double* __restrict__ A1, const double* __restrict__ gvs, int M, long Kc,
                               long ld) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int m = blockIdx.y;
  if (c >= Kc || m >= M) return;
  dA1[m * ld + c] -= 2.0 * A1[m * ld + c] * gvs[c];
}

// dst_b[i][j] (+)= alpha * (j <= i ? src_b[i][j] : 0)
__global__ void mask_lower_kernel(const double* __restrict__ src, long lds, long sbs, double* __restrict__ dst, long ldd, long dbs, int M,
                                  double alpha, int accumulate) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, b = blockIdx.z;
  if (j >= M) return;
  const double v = j <= i ? alpha * src[b * sbs + i * lds + j] : 0.0;
  double* d = dst + b * dbs + i * ldd + j;
  *d = accumulate ? *d + v : v;
}

// dst[i][j] (+)= alpha * src[i][j]   (rectangular copy between leading dimensions)
__global__ void copy2d_kernel(const double* __restrict__ src, long lds, double* __restrict__ dst, long ldd, int rows, int cols, double alpha,
                              int accumulate) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= cols || i >= rows) return;
  const double v = alpha * src[i * lds + j];
  double* d = dst + i * ldd + j;
  *d = accumulate ? *d + v : v;
}

// gq_sqrt[r][i][i] += 1 / Lq[r][i][i]   (- d/dLq of -1/2 log det(Lq Lq^T))
__global__ void kl_diag_kernel(double* __restrict__ gq, const double* __restrict__ Lq, int M, int Mp, int R, double kw) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= M * R) return;
  const int r = idx / M, i = idx % M;
  gq[((long)r * M + i) * M + i] += kw / Lq[((long)r * Mp + i) * Mp + i];
}

// Matern32 (BT == 2) / Matern52 (BT == 3) at rho = r^2 + 1e-12: the value k and g = -2 dk/drho = 3 variance exp(-a) | (5 / 3) variance (1 + a) exp(-a),
// a = sqrt(3 rho) | sqrt(5 rho).  Finite at r = 0.
template <int BT>
__device__ __forceinline__ void matern_k_g(double rho, double variance, double* k, double* g) {
  const double a = sqrt((BT == 2 ? 3.0 : 5.0) * rho), e = variance * exp(-a);
  if (BT == 2) { *k = (1.0 + a) * e; *g = 3.0 * e; }
  else { *k = fma(a, fma(a, 1.0 / 3.0, 1.0), 1.0) * e; *g = (5.0 / 3.0) * (1.0 + a) * e; }
}
// ---- RBF Gram backward ------------------------------------------------------------------------------------------
// One block per row i.  S = d ELBO / dK (not symmetrised).  Writes Es[i][j] = (S_ij + S_ji) k_ij (or nothing if Es is
// null), rs[i] = sum_j Es[i][j], and the per-row partial sums pv[i] = sum_j S_ij k_ij / variance, pl[i] = sum_j S_ij k_ij d_ij^2 / l^3.
// BT: 0 RBF; 2 / 3 Matern32 / Matern52, which are functions of rho = d^2 / l^2 + 1e-12 like the RBF (dk/drho = -k / 2 there): their g = -2 dk/drho takes
// the place of k in E, so that dZ and the lengthscale sum keep their form; the variance sum stays sum(S o K) / variance
template <int BT>
__global__ __launch_bounds__(256) void kuu_backward_kernel(const double* __restrict__ Z, const double* __restrict__ ZT, int ldzt, int M, int L,
                                                           const double* __restrict__ S, long lds,
                                                           double variance, double inv_l2, double inv_l3, double* __restrict__ Es, long lde,
                                                           double* __restrict__ rs, double* __restrict__ pv, double* __restrict__ pl) {
  __shared__ double red[256];
  const int i = blockIdx.x, t = threadIdx.x;
  double srow = 0.0, sv = 0.0, sl = 0.0;
  for (int j = t; j < M; j += 256) {
    double d2 = 0.0;
    if (ZT) {   // k-major copy of Z (prepare_all): neighbouring threads read neighbouring j
      for (int l = 0; l < L; ++l) {
        const double d = Z[(long)i * L + l] - ZT[(long)l * ldzt + j];
        d2 += d * d;
      }
    } else {
      for (int l = 0; l < L; ++l) {
        const double d = Z[(long)i * L + l] - Z[(long)j * L + l];
        d2 += d * d;
      }
    }
    double k, g;
    if constexpr (BT == 0) {
      k = variance * exp(-0.5 * d2 * inv_l2);
      g = k;
    } else {
      matern_k_g<BT>(fma(d2, inv_l2, 1e-12), variance, &k, &g);
    }
    const double e = S[i * lds + j] * g;
    sv += BT == 0 ? e : S[i * lds + j] * k;
    sl += e * d2;
    if (Es) {
      const double es = e + S[j * lds + i] * g;
      Es[i * lde + j] = es;
      srow += es;
    }
  }
  const double a = block_sum_256(srow, red), b = block_sum_256(sv, red), c = block_sum_256(sl, red);
  if (t == 0) {
    if (rs) rs[i] = a;
    pv[i] = b / variance;
    pl[i] = c * inv_l3;
  }
}

// ---- patch kernels backward -------------------------------------------------------------------------------------
// Xcol[c][l], c = n * P + p, l = (kh * f + kw) * C + ch  (FullView.extract_patches, conv_gp/views.py:46-54)
// A patch row (kh fixed) is ONE contiguous run of f C doubles of the image, and so is its place in Xcol: block (n, oh) copies the
// Wo f runs of its patch row -- thread (run slot, j): no division inside the loop.  (One thread per element with 64-bit index
// arithmetic: 26 us for the head's 41 MB at the headline size; one 250-element patch per block: 28.)
// SC (an ARD conv layer): Xcol[.][l] = patch[l] * sc[l], the patch divided by its per-dimension lengthscales while it is gathered
template <bool SC>
__global__ __launch_bounds__(256) void im2col_kernel(const double* __restrict__ X, int n_mod, int H, int W, int C, int f, int s, int Ho, int Wo,
                                                     int L, double* __restrict__ Xcol, const double* __restrict__ sc) {
  const int fc = f * C, n = blockIdx.x / Ho, oh = blockIdx.x - n * Ho;
  const int per = fc >= 256 ? 1 : 256 / fc;               // runs in flight per pass
  const int slot = fc >= 256 ? 0 : threadIdx.x / fc, j0 = fc >= 256 ? threadIdx.x : threadIdx.x - slot * fc;
  if (slot >= per) return;
  const double* __restrict__ img = X + (long)(n % n_mod) * H * W * C;
  double* __restrict__ out = Xcol + ((long)n * Ho * Wo + (long)oh * Wo) * L;
  const int runs = Wo * f;                                 // run r = ow * f + kh
  for (int r = slot; r < runs; r += per) {
    const int ow = r / f, kh = r - ow * f;
    const double* __restrict__ src = img + ((long)(oh * s + kh) * W + ow * s) * C;
    double* __restrict__ dst = out + (long)ow * L + kh * fc;
    for (int j = j0; j < fc; j += 256) {
      if constexpr (SC) dst[j] = src[j] * sc[kh * fc + j];
      else dst[j] = src[j];
    }
  }
}

// dX[n][h][w][ch] = sum over the patches that contain the pixel (adjoint of extract_patches; gather, no atomics)
// SC (an ARD conv layer): dXcol holds the gradient of the SCALED patches, element l of a patch counts sc[l] times
template <bool SC>
__global__ void col2im_kernel(const double* __restrict__ dXcol, int N, int H, int W, int C, int f, int s, int Ho, int Wo, int L,
                              double* __restrict__ dX, const double* __restrict__ sc) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)N * H * W * C) return;
  const int ch = (int)(idx % C);
  const int w = (int)((idx / C) % W), h = (int)((idx / ((long)C * W)) % H);
  const int n = (int)(idx / ((long)C * W * H));
  const int P = Ho * Wo;
  double acc = 0.0;
  for (int kh = 0; kh < f; ++kh) {
    const int hh = h - kh;
    if (hh < 0 || hh % s) continue;
    const int oh = hh / s;
    if (oh >= Ho) continue;
    for (int kw = 0; kw < f; ++kw) {
      const int ww = w - kw;
      if (ww < 0 || ww % s) continue;
      const int ow = ww / s;
      if (ow >= Wo) continue;
      const double g = dXcol[((long)n * P + oh * Wo + ow) * L + (kh * f + kw) * C + ch];
      if constexpr (SC) acc = fma(g, sc[(kh * f + kw) * C + ch], acc);
      else acc += g;
    }
  }
  dX[idx] = acc;
}

// Conv2dMean adjoint (conv_gp/mean_functions.py:28-41): map 0 of patch p copied the centre pixel of channel 0, so
// dX[n][oh s + f/2][ow s + f/2][0] += gm[(n P + p) R + 0]; distinct patches have distinct centres (no conflicts)
__global__ void idmean_backward_kernel(const double* __restrict__ gm, long Kc, int R, int P, int Wo, int H, int W, int C, int f, int s,
                                       double* __restrict__ dX) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= Kc) return;
  const long n = c / P;
  const int p = (int)(c % P), oh = p / Wo, ow = p % Wo;
  dX[((n * H + oh * s + f / 2) * W + ow * s + f / 2) * C] += gm[c * R];
}

// One thread per column c and row chunk (blockIdx.y), loop over the chunk's rows:
//   E[m][c] = dK[m][c / pdiv] * (w ? w[c % pdiv] * wscale : 1) * K[m][c]   (written over dK when pdiv == 1, else into E),
//   csp[chunk][c] = sum_m E, rawp[chunk][c] = sum_m dK K (head: for d patch_weights), per-block partials
//   pv = sum E, pl = sum E d^2 with d^2 = -2 l^2 log(K / variance).
__global__ __launch_bounds__(256) void e_form_kernel(const double* __restrict__ dK, long lddk, int pdiv, const double* __restrict__ w,
                                                     double wscale, const double* __restrict__ K, long ldk, double* __restrict__ E, long lde,
                                                     int M, int rows_per_chunk, long Kc, double inv_var, double two_l2,
                                                     double* __restrict__ csp, double* __restrict__ rawp, double* __restrict__ pv,
                                                     double* __restrict__ pl) {
  __shared__ double red[256];
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  const int m0 = blockIdx.y * rows_per_chunk, m1 = min(M, m0 + rows_per_chunk);
  double sc = 0.0, sr = 0.0, sd = 0.0;
  if (c < Kc) {
    const long cd = c / pdiv;
    const double f = w ? w[c % pdiv] * wscale : 1.0;
    for (int m = m0; m < m1; ++m) {
      const double k = K[m * ldk + c];
      const double r = dK[m * lddk + cd] * k;
      const double e = r * f;
      E[m * lde + c] = e;
      sr += r;
      sc += e;
      // d^2 = -2 l^2 log(k / variance).  A response so small that k / variance is a denormal or rounds to zero (the unit sweep's 2^t keeps
      // denormals where the launch-per-tile sweep flushed them: log -> -inf against e -> 0 would make the lengthscale gradient NaN) weighs
      // less than 1e-300: skipped
      const double q = k * inv_var;
      if (q >= 2.2250738585072014e-308) sd -= e * two_l2 * log(q);
    }
    csp[(long)blockIdx.y * Kc + c] = sc;
    if (rawp) rawp[(long)blockIdx.y * Kc + c] = sr;
  }
  const double a = block_sum_256(sc, red), b = block_sum_256(sd, red);
  if (threadIdx.x == 0) {
    pv[(long)blockIdx.y * gridDim.x + blockIdx.x] = a;
    pl[(long)blockIdx.y * gridDim.x + blockIdx.x] = b;
  }
}

// the same for two arrays at once (e_form: column sums of E and of dK o K)
__global__ void sum_chunks2_kernel(const double* __restrict__ pa, const double* __restrict__ pb, int chunks, long n, double* __restrict__ oa,
                                   double* __restrict__ ob) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double a = 0.0, b = 0.0;
  for (int ch = 0; ch < chunks; ++ch) { a += pa[(long)ch * n + i]; b += pb[(long)ch * n + i]; }
  oa[i] = a;
  ob[i] = b;
}
// out[i] = sum_ch part[ch][i]
__global__ void sum_chunks_kernel(const double* __restrict__ part, int chunks, long n, double* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int ch = 0; ch < chunks; ++ch) s += part[(long)ch * n + i];
  out[i] = s;
}

// part[chunk][m] = sum over the chunk's columns of A[m][c]: block (m, chunk); sum_chunks_kernel finishes
__global__ __launch_bounds__(256) void rowsum_big_kernel(const double* __restrict__ A, long ld, long Kc, long cols_per_chunk, int M,
                                                         double* __restrict__ part) {
  __shared__ double red[256];
  const int m = blockIdx.x;
  const long c0 = (long)blockIdx.y * cols_per_chunk, c1 = min(Kc, c0 + cols_per_chunk);
  double s = 0.0;
  for (long c = c0 + threadIdx.x; c < c1; c += 256) s += A[m * ld + c];
  const double r = block_sum_256(s, red);
  if (threadIdx.x == 0) part[(long)blockIdx.y * M + m] = r;
}

// out[p] (+)= scale * sum_n raw[n * P + p]: one block per p
__global__ __launch_bounds__(256) void strided_sum_kernel(const double* __restrict__ raw, int N, int P, double scale, int accumulate,
                                                          double* __restrict__ out) {
  __shared__ double red[256];
  const int p = blockIdx.x;
  double s = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) s += raw[(long)n * P + p];
  const double r = block_sum_256(s, red);
  if (threadIdx.x == 0) out[p] = accumulate ? out[p] + scale * r : scale * r;
}

// ConvKernel.Kdiag backward (conv_gp/kernels.py:106-115): block per (image n, patch p), thread per p'.
// Gm[n][p][p'] = x_p . x_p' in, E[n][p][p'] = g_n w_p w_p' k_pp' / P^2 out (over Gm; the squared norms come from the
// copy `norms`, because other blocks overwrite the diagonal they would otherwise be read from).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// one wave per (image n, patch p): 4 rows per 256-thread block, lanes stride over p'
__global__ __launch_bounds__(256) void kdiag_backward_kernel(double* __restrict__ Gm, const double* __restrict__ norms, const double* __restrict__ gkd,
                                                             const double* __restrict__ w, int P, double variance, double inv_l2,
                                                             double* __restrict__ dwn, double* __restrict__ pv, double* __restrict__ pl) {
  const int n = blockIdx.y, p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;
  double* G = Gm + ((long)n * P + p) * P;
  const double* nr = norms + (long)n * P;
  const double gpp = nr[p], wp = w[p];
  const double coef = gkd[n] / ((double)P * P);
  double se = 0.0, sd = 0.0, sw = 0.0;
  for (int q = lane; q < P; q += 64) {
    const double d2 = gpp + nr[q] - 2.0 * G[q];
    const double k = variance * exp(-0.5 * d2 * inv_l2);
    const double e = coef * wp * w[q] * k;
    sw += k * w[q];
    se += e;
    sd += e * d2;
    G[q] = e;
  }
  se = wave_sum(se); sd = wave_sum(sd); sw = wave_sum(sw);
  if (lane == 0) {
    const long o = (long)n * P + p;
    pv[o] = se;          // sum E over the row (also the row sum the patch gradient needs)
    pl[o] = sd;
    dwn[o] = 2.0 * coef * sw;
  }
}
// AdditivePatchKernel.Kdiag = variance * mean(w):  t[0] = sum_n g_n, t[1] = mean(w)
__global__ void additive_kdiag_backward_kernel(const double* __restrict__ t, int P, double variance, double* __restrict__ gw,
                                               double* __restrict__ var_slot) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < P) gw[p] += t[0] * variance / P;
  if (p == 0) *var_slot = t[0] * t[1];
}
__global__ void kdiag_norms_kernel(const double* __restrict__ Gm, int P, long n_img, double* __restrict__ norms) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_img * P) return;
  const long n = idx / P;
  const int p = (int)(idx % P);
  norms[idx] = Gm[(n * P + p) * P + p];
}

// the layer's three scalar gradients from their 16 slots each: lanes 16 q .. 16 q + 15 hold the slots of sum q (one load per lane -- one thread
// walking the 48 slots took ~50 us of a step's tail stream: a load, a wait and an add 48 times over)
__global__ void scal_finish_kernel(const double* __restrict__ slots, double* __restrict__ gscal) {
  if (blockIdx.x) return;
  const int lane = threadIdx.x, q = lane >> 4, i = lane & 15;
  double v = q < 3 ? slots[(q == 0 ? VAR_SLOT : (q == 1 ? LS_SLOT : P2_SLOT)) + i] : 0.0;
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
  if (q < 3 && i == 0) gscal[q] = v;
}

// ---- ArcCosine(order 0) base kernel (--base-kernel acos, conv layers) ------------------------------------------------
// K = variance (pi - theta) / pi, theta = acos(c'), c' = 1e-15 + (1 - 2e-15) c, c = (w x.z + b) / sqrt(Q A), Q = w |z|^2 + b,
// A = w |x|^2 + b.  With F = dLoss/dc = dK variance (1 - 2e-15) / (pi sin theta), F1 = F / sqrt(Q A), F2 = F c:
//   dZ = w (F1 X - (rowsum(F2) / Q) o Z),  dX = w (F1^T Z - (colsum(F2) / A) o X)     -- the RBF adjoint's shape with
//   E -> F1, rowsum(E) -> rowsum(F2) / Q, colsum(E) -> colsum(F2) / A, 1 / l^2 -> w, so patch_backward / kuu GEMMs are shared;
//   dw = sum F1 s - F2 (a / A + q / Q) / 2,  db = sum F1 - F2 (1 / A + 1 / Q) / 2   (s = x.z, a = |x|^2, q = |z|^2).
// theta and c are recovered from the stored K (theta = pi (1 - K / variance)).  Coincident points (sin theta ~ 0) carry no
// gradient except through the variance: c == 1 there identically in z, w and b (oracle/grad.py _acos_backward).
__global__ void rownorm_kernel(const double* __restrict__ X, long rows, int L, double* __restrict__ out) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= rows) return;
  double s = 0.0;
  for (int l = 0; l < L; ++l) { const double v = X[c * L + l]; s += v * v; }
  out[c] = s;
}
// one thread per column c and row chunk (blockIdx.y): F1 (beside dK: the chain stream still reads dK), F2, csp[chunk][c] = sum_m F2 / A_c, block partials
__global__ __launch_bounds__(256) void acos_e_form_kernel(const double* __restrict__ dK, double* __restrict__ F1, long ld, const double* __restrict__ K, double* __restrict__ F2,
                                                          int M, int rows_per_chunk, long Kc, double variance, double w, double b,
                                                          const double* __restrict__ zn, const double* __restrict__ xn, double* __restrict__ csp,
                                                          double* __restrict__ pv, double* __restrict__ pw, double* __restrict__ pb) {
  __shared__ double red[256];
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  const int m0 = blockIdx.y * rows_per_chunk, m1 = min(M, m0 + rows_per_chunk);
  double sv = 0.0, sw = 0.0, sb = 0.0, sc = 0.0;
  if (c < Kc) {
    const double a2 = xn[c], A = w * a2 + b;
    for (int m = m0; m < m1; ++m) {
      const double k = K[m * ld + c], dk = dK[m * ld + c];
      const double theta = 3.14159265358979323846 * (1.0 - k / variance);
      const double sn = sin(theta), cc = (cos(theta) - 1e-15) / (1.0 - 2e-15);
      const double F = sn > 1e-12 ? dk * variance * 0.31830988618379067154 * (1.0 - 2e-15) / sn : 0.0;
      const double q2 = zn[m], Q = w * q2 + b, rt = sqrt(Q * A);
      const double f1 = F / rt, f2 = F * cc;
      F1[m * ld + c] = f1;
      F2[m * ld + c] = f2;
      sv += dk * k;
      sw += f1 * (cc * rt - b) / w - 0.5 * f2 * (a2 / A + q2 / Q);
      sb += f1 - 0.5 * f2 * (1.0 / A + 1.0 / Q);
      sc += f2;
    }
    csp[(long)blockIdx.y * Kc + c] = sc / A;
  }
  const double a = block_sum_256(sv, red), bb = block_sum_256(sw, red), cc2 = block_sum_256(sb, red);
  if (threadIdx.x == 0) {
    const long o = (long)blockIdx.y * gridDim.x + blockIdx.x;
    pv[o] = a; pw[o] = bb; pb[o] = cc2;
  }
}
// v[i] /= (w * n[i] + b)
__global__ void acos_divide_kernel(double* __restrict__ v, const double* __restrict__ n, int M, double w, double b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M) v[i] /= (w * n[i] + b);
}
// Matern K_uf adjoint, one thread per column c and row chunk (blockIdx.y).  In: E[m][c] = z_m . x_c (a product of Z and Xcol).  Out: E = dK o g with
// g = -2 dk/drho at rho = max(|z|^2 + |x|^2 - 2 z.x, 0) / l^2 + 1e-12, the forward pass's own argument; csp[chunk][c] = sum_m E, block partials
// pv = sum dK o K (K as the forward pass stored it) and pl = sum E d^2: what e_form_kernel leaves for the RBF
template <int BT>
__global__ __launch_bounds__(256) void matern_e_form_kernel(const double* __restrict__ dK, double* __restrict__ E, long ld, const double* __restrict__ K,
                                                            int M, int rows_per_chunk, long Kc, double variance, double inv_l2,
                                                            const double* __restrict__ zn, const double* __restrict__ xn, double* __restrict__ csp,
                                                            double* __restrict__ pv, double* __restrict__ pl) {
  __shared__ double red[256];
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  const int m0 = blockIdx.y * rows_per_chunk, m1 = min(M, m0 + rows_per_chunk);
  double sv = 0.0, sl = 0.0, sc = 0.0;
  if (c < Kc) {
    const double a2 = xn[c];
    for (int m = m0; m < m1; ++m) {
      const double dk = dK[m * ld + c];
      const double d2 = fmax(zn[m] + a2 - 2.0 * E[m * ld + c], 0.0);
      double k, g;
      matern_k_g<BT>(fma(d2, inv_l2, 1e-12), variance, &k, &g);
      const double e = dk * g;
      E[m * ld + c] = e;
      sv += dk * K[m * ld + c];
      sl += e * d2;
      sc += e;
    }
    csp[(long)blockIdx.y * Kc + c] = sc;
  }
  const double a = block_sum_256(sv, red), b = block_sum_256(sl, red);
  if (threadIdx.x == 0) {
    const long o = (long)blockIdx.y * gridDim.x + blockIdx.x;
    pv[o] = a; pl[o] = b;
  }
}
// Gram adjoint, one block per row i (both arguments are Z; the diagonal is skipped): Es[i][j] = (F_ij + F_ji) / sqrt(Q_i Q_j),
// rs[i] = sum_j (F_ij + F_ji) c_ij / Q_i, partials pv (variance), pw, pb
__global__ __launch_bounds__(256) void acos_kuu_backward_kernel(const double* __restrict__ Z, const double* __restrict__ zn, int M, int L,
                                                                const double* __restrict__ S, long lds, double variance, double w, double b,
                                                                double* __restrict__ Es, long lde, double* __restrict__ rs,
                                                                double* __restrict__ pv, double* __restrict__ pw, double* __restrict__ pb) {
  __shared__ double red[256];
  const int i = blockIdx.x, t = threadIdx.x;
  const double qi = zn[i], Qi = w * qi + b;
  double srow = 0.0, sv = 0.0, sw = 0.0, sb = 0.0;
  for (int j = t; j < M; j += 256) {
    double s = 0.0;
    for (int l = 0; l < L; ++l) s += Z[(long)i * L + l] * Z[(long)j * L + l];
    const double qj = zn[j], Qj = w * qj + b, rt = sqrt(Qi * Qj);
    const double c = (w * s + b) / rt;
    const double cp = fmin(1e-15 + (1.0 - 2e-15) * c, 1.0);
    const double theta = acos(cp);
    const double k = variance * (1.0 - (j == i ? acos(1.0 - 1e-15) : theta) * 0.31830988618379067154);   // the diagonal: BaseKernel::eval_diag
    const double Sij = S[i * lds + j];
    sv += Sij * k;
    double es = 0.0;
    if (j != i) {
      const double sn = sin(theta);
      const double g = sn > 1e-12 ? variance * 0.31830988618379067154 * (1.0 - 2e-15) / sn : 0.0;
      const double Fij = Sij * g, Fji = S[j * lds + i] * g;
      const double f1 = Fij / rt;
      sw += f1 * s - 0.5 * Fij * c * (qi / Qi + qj / Qj);
      sb += f1 - 0.5 * Fij * c * (1.0 / Qi + 1.0 / Qj);
      es = (Fij + Fji) / rt;
      srow += (Fij + Fji) * c;
    }
    if (Es) Es[i * lde + j] = es;
  }
  const double a = block_sum_256(srow, red), bv = block_sum_256(sv, red), cw = block_sum_256(sw, red), db = block_sum_256(sb, red);
  if (t == 0) {
    if (rs) rs[i] = a / Qi;
    pv[i] = bv / variance;
    pw[i] = cw;
    pb[i] = db;
  }
}

// ---- dense RBF(ARD) head (--last-kernel rbf) --------------------------------------------------------------------------
// out[i][d] = in[(i % n_mod)][d] * s[d]
__global__ void scale_rows_kernel(const double* __restrict__ in, int n_mod, long rows, int D, const double* __restrict__ s, double* __restrict__ out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * D) return;
  const long i = idx / D;
  const int d = (int)(idx % D);
  out[idx] = in[(i % n_mod) * D + d] * s[d];
}
// chain rule back through x / l, z / l: gZ = dZs o s, dX = dXs o s (if wanted), and one block per input dimension d:
// gard[d] = -s_d (sum_m dZs[m][d] Zs[m][d] + sum_n dXs[n][d] Xs[n][d])
__global__ __launch_bounds__(256) void ard_finish_kernel(const double* __restrict__ dZs, const double* __restrict__ Zs, int M, const double* __restrict__ dXs,
                                                         const double* __restrict__ Xs, long N, int D, const double* __restrict__ s,
                                                         double* __restrict__ gZ, double* __restrict__ dX, double* __restrict__ gard) {
  __shared__ double red[256];
  const int d = blockIdx.x, t = threadIdx.x;
  const double sd = s[d];
  double acc = 0.0;
  for (int m = t; m < M; m += 256) {
    const double g = dZs[(long)m * D + d];
    acc += g * Zs[(long)m * D + d];
    gZ[(long)m * D + d] = g * sd;
  }
  for (long n = t; n < N; n += 256) {
    const double g = dXs[n * D + d];
    acc += g * Xs[n * D + d];
    if (dX) dX[n * D + d] = g * sd;
  }
  const double r = block_sum_256(acc, red);
  if (t == 0) gard[d] = -sd * r;
}

// ---- ARD conv layer: RBF(f f C, ARD=True) on the patches ------------------------------------------------------------
// part[c][d] = sum over the rows r of chunk c of dXs[r][d] Xs[r][d]: the patches' share of the lengthscale gradient, in a fixed order.
// 256 / D rows in flight per pass (D <= 256), one otherwise.
__global__ __launch_bounds__(256) void ard_xsum_kernel(const double* __restrict__ dXs, const double* __restrict__ Xs, long rows, int D, long rpc,
                                                       double* __restrict__ part) {
  __shared__ double red[256];
  const int t = threadIdx.x, Dq = D < 256 ? D : 256, per = 256 / Dq, rr = t / Dq, dd = t - rr * Dq;
  const long r0 = (long)blockIdx.x * rpc, r1 = r0 + rpc < rows ? r0 + rpc : rows;
  for (int d0 = 0; d0 < D; d0 += Dq) {
    const int d = d0 + dd;
    double acc = 0.0;
    if (rr < per && d < D)
      for (long r = r0 + rr; r < r1; r += per) acc = fma(dXs[r * D + d], Xs[r * D + d], acc);
    red[t] = acc;
    __syncthreads();
    if (rr == 0 && d < D) {
      double sum = 0.0;
      for (int q = 0; q < per; ++q) sum += red[q * Dq + dd];
      part[(long)blockIdx.x * D + d] = sum;
    }
    __syncthreads();
  }
}
// The chain rule back through x o s, z o s (s = 1 / lengthscales), one block per patch element d: gZ[m][d] = dZs[m][d] s_d and
// gard[d] = -s_d (sum_m dZs Zs + sum_m dZ0s Z0s [the frozen prior's Gram matrix, unwhitened layers] + sum_c xpart[c][d])
__global__ __launch_bounds__(256) void ard_conv_finish_kernel(const double* __restrict__ dZs, const double* __restrict__ Zs, const double* __restrict__ dZ0s,
                                                              const double* __restrict__ Z0s, int M, int D, const double* __restrict__ xpart, int chunks,
                                                              const double* __restrict__ s, double* __restrict__ gZ, double* __restrict__ gard) {
  __shared__ double red[256];
  const int d = blockIdx.x, t = threadIdx.x;
  const double sd = s[d];
  double acc = 0.0;
  for (int m = t; m < M; m += 256) {
    const double g = dZs[(long)m * D + d];
    acc = fma(g, Zs[(long)m * D + d], acc);
    gZ[(long)m * D + d] = g * sd;
    if (dZ0s) acc = fma(dZ0s[(long)m * D + d], Z0s[(long)m * D + d], acc);
  }
  for (int c = t; c < chunks; c += 256) acc += xpart[(long)c * D + d];
  const double r = block_sum_256(acc, red);
  if (t == 0) gard[d] = -sd * r;
}

// ---- host helpers ------------------------------------------------------------------------------------------------
struct Bk {   // per-backward bookkeeping
  dcgp_model* m;
  dcgp_ctx* ctx;
  std::string pfx;   // workspace prefix of the layer being processed
  int slot_v = 0, slot_l = 0, slot_b = 0;
  // hyper-parameter partial sums of the layer being processed: collected here, reduced into the layer's scalar slots by ONE launch at the end of
  // its reverse pass (end_layer; they feed nothing else, and each used to be a 5 us launch in the middle of the data path)
  struct PendingSum { const double* in; long n; double scale; double* out; };
  std::vector<PendingSum> pending;
  bool last_layer = false;     // the layer being processed is the last one of the reverse pass (layer 0)
  int prep = 0;                // the layer being processed: bit 0 fills + GT + Lc, bit 1 S_r done beside the forward pass (grad_kl_early)
  bool kl_early = false;       // the layer being processed had its kl_products beside the forward pass (grad_kl_early)
  bool side_pending = false;   // a layer left the end of its reverse pass on the side stream: model_backward joins once, at the end
  double klw = 1.0;   // weight of the (replicated) KL term on this rank: 1 / number of batch shards
  // model_backward_data (the input gradient): only the data path runs -- the column-wise adjoint of each conditional, the patch kernel's adjoint with
  // respect to the patches, dX.  Nothing is written outside the "g_" workspaces: no gradient block, no scalar slot, no chain, no KL, no dZ.
  bool data_only = false;
  // a mixed layer (mix.hip): what the walk hands its conv_backward beside the latent (gm, gv) -- the gradient gF of its Rout maps for the mean filter's
  // adjoints [rows P][Rout] (summed over the replicas of a de-duplicated first layer), and for gW every replica's columns: u and gF [mix_cols][.]
  const double* mix_gF = nullptr; const double* mix_gF_all = nullptr; long mix_cols = 0;
  double* ws(const char* name, size_t n_doubles) { return (double*)ws_get(ctx, pfx + "g_" + name, (n_doubles ? n_doubles : 1) * sizeof(double)); }
};

// The three streams of a layer's reverse pass.  main: the data path (the column-wise adjoint, the patch-kernel adjoint, dX for the layer
// below).  chain: the M x M chain of the conditional (W_r -> dG_r -> dq_sqrt -> dL -> Cholesky adjoint -> S).  tail: what needs S -- the Gram
// adjoint of K_uu, the KL pieces, the scalar sums, dZ.  Nothing on chain or tail feeds the layer below: the main stream never waits for
// them inside a step (model_backward joins once, at the end).  Option grad_nofork / no side stream: all three are the main stream.
struct Lanes { hipStream_t main, chain, tail; bool forked; };
Lanes lanes_of(dcgp_ctx* c) {
  Lanes l;
  l.main = c->stream;
  l.forked = !c->opt.grad_nofork && !c->no_side && c->stream2 && c->stream2 != c->stream;
  l.chain = l.forked ? c->stream2 : c->stream;
  l.tail = l.forked ? (c->stream_aux ? c->stream_aux : c->stream2) : c->stream;
  return l;
}
// launches issued in its lifetime go to `s`, behind `after` (an event already recorded on another stream) when s is not the current stream
struct OnStream {
  dcgp_ctx* ctx;
  hipStream_t saved;
  bool ok = true;
  OnStream(dcgp_ctx* c, hipStream_t s, hipEvent_t after) : ctx(c), saved(c->stream) {
    if (s != saved && after && hipStreamWaitEvent(s, after, 0) != hipSuccess) ok = false;
    c->stream = s;
  }
  ~OnStream() { ctx->stream = saved; }
};

GenGemm mk(const double* A, long ars, long acs, const double* B, long brs, long bcs, double* C, long crs, int M, int N, int K) {
  GenGemm g;
  g.A = A; g.a_rs = ars; g.a_cs = acs; g.B = B; g.b_rs = brs; g.b_cs = bcs; g.C = C; g.c_rs = crs; g.M = M; g.N = N; g.K = K;
  return g;
}

#define NEED(p) do { if (!(p)) return DCGP_ERR_ALLOC; } while (0)

// scale * sum(part[0..n)) goes to the next slot of the layer: which = 0 variance, 1 lengthscale | acos weight variance, 2 acos bias variance
int add_scalar(Bk& bk, LayerState& L, int which, const double* part, long n, double scale) {
  if (bk.data_only) return DCGP_OK;
  int& s = which == 0 ? bk.slot_v : (which == 1 ? bk.slot_l : bk.slot_b);
  if (s >= 16) return ctx_fail(bk.ctx, DCGP_ERR_ARG, "grad: out of scalar slots");
  bk.pending.push_back({part, n, scale, L.gslots + (which == 0 ? VAR_SLOT : (which == 1 ? LS_SLOT : P2_SLOT)) + s});
  ++s;
  return DCGP_OK;
}
struct ScalarPart { int which; const double* part; long n; double scale; };
int add_scalars(Bk& bk, LayerState& L, std::initializer_list<ScalarPart> parts) {
  for (const ScalarPart& p : parts) {
    if (p.part) DCGP_TRY(add_scalar(bk, L, p.which, p.part, p.n, p.scale));   // (null: a sum this base kernel does not have)
  }
  return DCGP_OK;
}
int flush_scalars(Bk& bk) {
  for (size_t i = 0; i < bk.pending.size(); i += REDUCE_JOBS_MAX) {
    ReduceJobs j{};
    int k = 0;
    for (; k < REDUCE_JOBS_MAX && i + k < bk.pending.size(); ++k) {
      const Bk::PendingSum& p = bk.pending[i + k];
      j.in[k] = p.in; j.n[k] = p.n; j.scale[k] = p.scale; j.out[k] = p.out;
    }
    DCGP_TRY(reduce_sum_multi(bk.ctx, j, k));
  }
  bk.pending.clear();
  return DCGP_OK;
}

// sc: nullptr, or [L] factors of the patch elements (an ARD conv layer's 1 / lengthscales)
int im2col(dcgp_ctx* ctx, const LayerState& L, const double* Xin, int n_mod, long Kc, double* Xcol, const double* sc = nullptr) {
  const long rows = Kc / L.v.P;
  if (rows * L.v.Ho > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "grad: too many patch rows");
  hipLaunchKernelGGL(sc ? im2col_kernel<true> : im2col_kernel<false>, dim3((unsigned)(rows * L.v.Ho)), dim3(256), 0, ctx->stream, Xin, n_mod, L.v.H, L.v.W,
                     L.v.C, L.v.f, L.v.s, L.v.Ho, L.v.Wo, L.v.L, Xcol, sc);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// row chunks of an E-form launch (a thread per column and chunk): enough to put a few thousand blocks on the chip, 16 rows or more each
struct RowChunks { unsigned nb; int chunks, rpc; };
RowChunks row_chunks(int M, long Kc) {
  const unsigned nb = blocks_for(Kc);
  const int chunks = std::min((int)std::min<long>(16, std::max<long>(1, 2048 / nb)), (M + 15) / 16);
  const int rpc = (M + chunks - 1) / chunks;
  return {nb, (M + rpc - 1) / rpc, rpc};
}

// out[m] = sum_c A[m][c] over Kc columns: per-chunk partial sums (4096 columns or more a chunk, at most 32 chunks), then their sum
int row_sums(Bk& bk, const double* A, long ld, long Kc, int M, double* out) {
  dcgp_ctx* ctx = bk.ctx;
  const int chunks = (int)std::min<long>(32, (Kc + 4095) / 4096);
  const long cpc = round_up_l((Kc + chunks - 1) / chunks, 256);
  double* rsp = bk.ws("pb_rsp", (size_t)chunks * M);
  NEED(rsp);
  hipLaunchKernelGGL(rowsum_big_kernel, dim3(M, chunks), dim3(256), 0, ctx->stream, A, ld, Kc, cpc, M, rsp);
  LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(sum_chunks_kernel, dim3(blocks_for(M)), dim3(256), 0, ctx->stream, rsp, chunks, (long)M, out);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// a workspace of at least min_bytes that the forward pass left for the layer being processed; nullptr, with the context's error set, if it is not there
const double* forward_left(Bk& bk, const char* name, size_t min_bytes, const char* what) {
  auto it = bk.ctx->ws.find(bk.pfx + name);
  if (it != bk.ctx->ws.end() && it->second.second >= min_bytes) return (const double*)it->second.first;
  ctx_fail(bk.ctx, DCGP_ERR_ARG, "grad: the forward pass left no %s", what);
  return nullptr;
}

// the hyper-parameter partial sums a Gram backward left in its scratch (`tag`) -> the layer's scalar slots
int kuu_scalars(Bk& bk, LayerState& L, const char* tag) {
  const std::string t(tag);
  const int M = L.M;
  if (L.base_type == 1) DCGP_TRY(add_scalar(bk, L, 2, bk.ws((t + "_pb").c_str(), M), M, 1.0));
  return add_scalars(bk, L, {{0, bk.ws((t + "_pv").c_str(), M), M, 1.0}, {1, bk.ws((t + "_pl").c_str(), M), M, 1.0}});
}

// RBF Gram backward from S = d ELBO / dK (unsymmetrised).  dZ accumulates into L.gZ when Zsrc is the live Z (want_dz).
// tag: prefix of its scratch; defer_scalars: leave the hyper-parameter partial sums there (kuu_scalars adds them later -- the scalar
// slots of a layer are zeroed at the start of its reverse pass, and the KL half of a frozen prior runs before that)
// dz_after: the product that adds into dZ is enqueued behind this event (the patch adjoint adds into the same dZ on another stream)
int kuu_backward(Bk& bk, LayerState& L, const double* Zsrc, const double* S, long lds, bool want_dz, double* dz_out = nullptr,
                 const char* tag = "kuu", bool defer_scalars = false, hipEvent_t dz_after = nullptr) {
  dcgp_ctx* ctx = bk.ctx;
  const int M = L.M, Ld = L.v.L;
  const double inv_l2 = 1.0 / (L.ls * L.ls), inv_l3 = inv_l2 / L.ls;
  const std::string t(tag);
  double *Es = nullptr, *rs = nullptr;
  double* pv = bk.ws((t + "_pv").c_str(), M);
  double* pl = bk.ws((t + "_pl").c_str(), M);
  NEED(pv); NEED(pl);
  if (want_dz) { Es = bk.ws((t + "_Es").c_str(), (size_t)M * M); rs = bk.ws((t + "_rs").c_str(), M); NEED(Es); NEED(rs); }
  double cz = inv_l2;      // factor of the dZ combination: 1 / l^2 (RBF) or the weight variance (ArcCosine)
  if (L.base_type == 1) {
    double* pb = bk.ws((t + "_pb").c_str(), M);
    double* znv = bk.ws((t + "_zn").c_str(), M);
    NEED(pb); NEED(znv);
    hipLaunchKernelGGL(rownorm_kernel, dim3(blocks_for(M)), dim3(256), 0, ctx->stream, Zsrc, (long)M, Ld, znv);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(acos_kuu_backward_kernel, dim3(M), dim3(256), 0, ctx->stream, Zsrc, znv, M, Ld, S, lds, L.variance, L.acos_w, L.acos_b,
                       Es, (long)M, rs, pv, pl, pb);
    LAUNCH_CHECK(ctx);
    cz = L.acos_w;
  } else {
    auto kern = L.base_type == 0 ? kuu_backward_kernel<0> : (L.base_type == 2 ? kuu_backward_kernel<2> : kuu_backward_kernel<3>);
    hipLaunchKernelGGL(kern, dim3(M), dim3(256), 0, ctx->stream, Zsrc, Zsrc == L.Z ? L.ZT : nullptr, L.Mp, M, Ld, S, lds, L.variance,
                       inv_l2, inv_l3, Es, (long)M, rs, pv, pl);
    LAUNCH_CHECK(ctx);
  }
  if (!defer_scalars) DCGP_TRY(kuu_scalars(bk, L, tag));
  if (want_dz) {
    // dZ += cz (Es Z - rs o Z): the correction rides in the product's epilogue
    if (dz_after) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, dz_after, 0));
    GenGemm e = mk(Es, M, 1, Zsrc, Ld, 1, dz_out ? dz_out : L.gZ, Ld, M, Ld, M);
    e.alpha = cz; e.accumulate = 1; e.sub_v = rs; e.sub_x = Zsrc; e.sx_rs = Ld;
    DCGP_TRY(gemm_gen(ctx, e));
  }
  return DCGP_OK;
}

// Patch-kernel backward: E [M x Kc] (ld) = d ELBO / dKfull o Kfull is ready, cs = its column sums.
// dZ += (E Xcol - rowsum(E) o Z) / l^2;  dXcol (=|+=) (E^T Z - cs o Xcol) / l^2 when requested.
// dz_lanes (the head): the dZ product goes to the TAIL stream, behind an event recorded here -- nothing on the main stream reads dZ, the tail stream is
// idle at this point of the head's reverse pass and adds its own term into the same dZ later (kuu_backward: in stream order behind this one), and the two
// long products of the patch adjoint (73 + 86 us at the headline size, neither of them bound by the matrix pipe) then run beside each other
int patch_backward(Bk& bk, LayerState& L, const double* E, long ld, long Kc, const double* cs, const double* Xcol, double* dXcol,
                   int dx_accumulate, const double* Zuse = nullptr, double* dz_out = nullptr, const double* rs_in = nullptr, double cz = 0.0,
                   const Lanes* dz_lanes = nullptr) {
  dcgp_ctx* ctx = bk.ctx;
  const int M = L.M, Ld = L.v.L;
  const double inv_l2 = cz != 0.0 ? cz : 1.0 / (L.ls * L.ls);   // cz: the ArcCosine adjoint passes its weight variance (and its own row vector)
  double* rs = rs_in ? const_cast<double*>(rs_in) : bk.ws("pb_rs", M);
  NEED(rs);
  if (!rs_in && !bk.data_only) DCGP_TRY(row_sums(bk, E, ld, Kc, M, rs));
  const double* Zp = Zuse ? Zuse : L.Z;
  if (!bk.data_only) {   // dZ += (E Xcol - rs o Z) / l^2: one product over the columns (split along k), the correction in its epilogue
    GenGemm e = mk(E, ld, 1, Xcol, Ld, 1, dz_out ? dz_out : L.gZ, Ld, M, Ld, (int)Kc);
    e.alpha = inv_l2; e.accumulate = 1; e.sub_v = rs; e.sub_x = Zp; e.sx_rs = Ld;
    if (dz_lanes && dz_lanes->forked && !dz_out && !ctx->opt.grad_dz_main) {
      HIP_TRY(ctx, hipEventRecord(ctx->ev_g[5], ctx->stream));   // E, Xcol, rs are there
      OnStream on(ctx, dz_lanes->tail, ctx->ev_g[5]);
      if (!on.ok) return ctx_fail(ctx, DCGP_ERR_HIP, "grad: stream wait failed");
      DCGP_TRY(gemm_gen(ctx, e));
    } else {
      DCGP_TRY(gemm_gen(ctx, e));
    }
  }
  if (dXcol) {   // dXcol (+)= (E^T Z - cs o Xcol) / l^2
    GenGemm e = mk(E, 1, ld, Zp, Ld, 1, dXcol, Ld, (int)Kc, Ld, M);
    e.alpha = inv_l2; e.accumulate = dx_accumulate; e.sub_v = cs; e.sub_x = Xcol; e.sx_rs = Ld;
    DCGP_TRY(gemm_gen(ctx, e));
  }
  return DCGP_OK;
}

// KL backward of one layer (ELBO = ... - KL), in two halves.
// kl_products: everything that is a product of parameter-only matrices -- inv(K) q_mu, inv(K) Lq_r, -dKL/dK_prior -- into scratch.  The last one
// goes into `Sacc` [M x M, ld Mp] (head: the prior shares the live Z; s_first: Sacc is written, otherwise added to) or, Sacc == null, through
// the Gram backward on the frozen Z0 (conv layers), whose partial sums stay in scratch.  Nothing here reads the step's data or writes a
// gradient buffer: grad_kl_early runs it beside the FORWARD pass, where the side stream is idle -- at the end of a layer's reverse pass
// (fourteen short launches) it was the tail of the whole step.
// kl_apply: adds the pieces to dq_mu / dq_sqrt and the scalar slots (a whitened layer has no products: its KL adjoint is q_mu and Lq themselves).
int kl_products(Bk& bk, LayerState& L, double* Sacc, bool s_first) {
  dcgp_ctx* ctx = bk.ctx;
  if (L.white) return DCGP_OK;
  const int M = L.M, Mp = L.Mp, R = L.R, Rp = L.g.Rp;
  const long mm = (long)Mp * Mp;
  const double kw = bk.klw;
  const double* Lpinv = L.g.Kp ? L.g.Lpinv : L.g.Linv;
  double* a1 = bk.ws("kl_a1", (size_t)Mp * Rp);
  double* Kimu = bk.ws("kl_Kimu", (size_t)Mp * Rp);
  double* Wm = bk.ws("kl_W", (size_t)R * mm);
  double* KiL = bk.ws("kl_KiL", (size_t)R * mm);
  NEED(a1); NEED(Kimu); NEED(Wm); NEED(KiL);
  DCGP_TRY(gemm_gen(ctx, mk(Lpinv, Mp, 1, L.q_mu, R, 1, a1, Rp, M, R, M)));
  DCGP_TRY(gemm_gen(ctx, mk(Lpinv, 1, Mp, a1, Rp, 1, Kimu, Rp, M, R, M)));
  GenGemm g1 = mk(Lpinv, Mp, 1, L.g.Lq, Mp, 1, Wm, Mp, M, M, M);
  g1.batch = R; g1.b_bs = mm; g1.c_bs = mm;
  DCGP_TRY(gemm_gen(ctx, g1));
  const long Rm = (long)R * Mp;
  if (Mp > M) HIP_TRY(ctx, hipMemsetAsync(KiL, 0, (size_t)R * mm * sizeof(double), ctx->stream));   // (the padded k of the stacked product below)
  GenGemm g2 = mk(Lpinv, 1, Mp, Wm, Mp, 1, KiL, Rm, M, M, M);        // inv(K) Lq_r, stored [i][r][k]
  g2.batch = R; g2.b_bs = mm; g2.c_bs = Mp;
  DCGP_TRY(gemm_gen(ctx, g2));
  // -dKL/dK = -1/2 [R inv(K) - (inv(K) q_mu)(inv(K) q_mu)^T - sum_r (inv(K) Lq_r)(inv(K) Lq_r)^T]
  double* Sk = Sacc;
  int acc = s_first ? 0 : 1;
  if (!Sk) { Sk = bk.ws("kl_S", (size_t)mm); NEED(Sk); acc = 0; }
  GenGemm g3 = mk(Lpinv, 1, Mp, Lpinv, Mp, 1, Sk, Mp, M, M, M);
  g3.alpha = -0.5 * R * kw; g3.accumulate = acc;
  DCGP_TRY(gemm_gen(ctx, g3));
  GenGemm g4 = mk(Kimu, Rp, 1, Kimu, 1, Rp, Sk, Mp, M, M, R);
  g4.alpha = 0.5 * kw; g4.accumulate = 1;
  DCGP_TRY(gemm_gen(ctx, g4));
  GenGemm g5 = mk(KiL, Rm, 1, KiL, 1, Rm, Sk, Mp, M, M, (int)Rm);     // all r at once, stacked along k
  g5.alpha = 0.5 * kw; g5.accumulate = 1;
  DCGP_TRY(gemm_gen(ctx, g5));
  if (!Sacc && L.in_scale) {
    // ARD conv layer: K_p(Z0) is the Gram matrix of Z0 o s, so it depends on the lengthscales although Z0 is frozen -- the adjoint with respect to
    // the scaled rows stays in scratch (conv_layer_ard_finish turns it into the prior's share of gard; nothing of it goes to gZ)
    double* Z0s = bk.ws("klz_Zs", (size_t)M * L.v.L);
    double* dZ0s = bk.ws("klz_dZs", (size_t)M * L.v.L);
    NEED(Z0s); NEED(dZ0s);
    hipLaunchKernelGGL(scale_rows_kernel, dim3(blocks_for((long)M * L.v.L)), dim3(256), 0, ctx->stream, L.Z0, M, (long)M, L.v.L, L.in_scale, Z0s);
    LAUNCH_CHECK(ctx);
    HIP_TRY(ctx, hipMemsetAsync(dZ0s, 0, (size_t)M * L.v.L * sizeof(double), ctx->stream));
    DCGP_TRY(kuu_backward(bk, L, Z0s, Sk, Mp, true, dZ0s, "klz", true));
  } else if (!Sacc) {
    DCGP_TRY(kuu_backward(bk, L, L.Z0, Sk, Mp, false, nullptr, "klz", true));   // frozen Z0: hyper-parameters only
  }
  return DCGP_OK;
}
int kl_apply(Bk& bk, LayerState& L, bool frozen_prior) {
  dcgp_ctx* ctx = bk.ctx;
  if (bk.kl_early) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_kl3, 0));   // the products came from the auxiliary stream
  const int M = L.M, Mp = L.Mp, R = L.R, Rp = L.g.Rp;
  const long mm = (long)Mp * Mp;
  const double kw = bk.klw;
  if (L.white) {
    hipLaunchKernelGGL(copy2d_kernel, dim3(blocks_for(R), M), dim3(256), 0, ctx->stream, L.q_mu, (long)R, L.gq_mu, (long)R, M, R, -kw, 1);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(mask_lower_kernel, dim3(blocks_for(M), M, R), dim3(256), 0, ctx->stream, L.g.Lq, (long)Mp, mm, L.gq_sqrt, (long)M,
                       (long)M * M, M, -kw, 1);
    LAUNCH_CHECK(ctx);
  } else {
    const long Rm = (long)R * Mp;
    const double* Kimu = bk.ws("kl_Kimu", (size_t)Mp * Rp);
    const double* KiL = bk.ws("kl_KiL", (size_t)R * mm);
    NEED(Kimu); NEED(KiL);
    hipLaunchKernelGGL(copy2d_kernel, dim3(blocks_for(R), M), dim3(256), 0, ctx->stream, Kimu, (long)Rp, L.gq_mu, (long)R, M, R, -kw, 1);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(mask_lower_kernel, dim3(blocks_for(M), M, R), dim3(256), 0, ctx->stream, KiL, Rm, (long)Mp, L.gq_sqrt, (long)M,
                       (long)M * M, M, -kw, 1);
    LAUNCH_CHECK(ctx);
    if (frozen_prior) DCGP_TRY(kuu_scalars(bk, L, "klz"));
  }
  hipLaunchKernelGGL(kl_diag_kernel, dim3(blocks_for((long)M * R)), dim3(256), 0, ctx->stream, L.gq_sqrt, L.g.Lq, M, Mp, R, kw);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// Parameter-only operands of cond_backward: sgg == false: G^T stacked along k (GT) and the lower triangle of the factor (Lc);
// sgg == true: S_r = G_r G_r^T, the strip kernel's operand.
int param_operands(Bk& bk, LayerState& L, bool sgg) {
  dcgp_ctx* ctx = bk.ctx;
  const int M = L.M, Mp = L.Mp, R = L.R;
  const long mm = (long)Mp * Mp;
  const GpMats& g = L.g;
  if (sgg) {
    double* Sgg = bk.ws("Sgg", (size_t)R * mm);
    NEED(Sgg);
    if (Mp > M) HIP_TRY(ctx, hipMemsetAsync(Sgg, 0, (size_t)R * mm * sizeof(double), ctx->stream));
    GenGemm sg = mk(g.G, Mp, 1, g.G, 1, Mp, Sgg, Mp, M, M, M);
    sg.batch = R; sg.a_bs = mm; sg.b_bs = mm; sg.c_bs = mm;
    return gemm_gen(ctx, sg);
  }
  if (L.has_qsqrt) {
    double* GT = bk.ws("GT", (size_t)R * mm);
    NEED(GT);
    hipLaunchKernelGGL(restack_transpose_kernel, dim3(blocks_for(R * mm)), dim3(256), 0, ctx->stream, g.G, Mp, R, GT);
    LAUNCH_CHECK(ctx);
  }
  double* Lc = bk.ws("Lc", (size_t)mm);
  NEED(Lc);
  hipLaunchKernelGGL(mask_lower_kernel, dim3(blocks_for(M), M, 1), dim3(256), 0, ctx->stream, g.K, (long)Mp, 0L, Lc, (long)Mp, 0L, M, 1.0, 0);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// The terms of dL that do not come out of the chain:  dL = -tril(dq_mu alpha^T) [unwhitened; the first writer of dL],  dL (+)= -tril(dKuf A1^T).
// The first one is ALWAYS formed on the main stream, right behind dq_mu: the tail stream adds the KL part into dq_mu as soon as ev_g[1] is past.
int dl_term_mu(Bk& bk, LayerState& L, double* dL) {
  GenGemm l1 = mk(L.gq_mu, L.R, 1, L.g.alpha, 1, L.g.Rp, dL, L.Mp, L.M, L.M, L.R);
  l1.alpha = -1.0; l1.lower_only = 1;
  return gemm_gen(bk.ctx, l1);
}
int dl_term_kuf(Bk& bk, LayerState& L, const double* A1, long ld, long Kc, const double* dKuf, double* dL) {
  GenGemm l3 = mk(dKuf, ld, 1, A1, 1, ld, dL, L.Mp, L.M, L.M, (int)Kc);
  l3.alpha = -1.0; l3.lower_only = 1; l3.accumulate = L.white ? 0 : 1;   // (whitened: the only term)
  return gemm_gen(bk.ctx, l3);
}

// The conditional's backward shared by conv layers and the head, in two calls.  Kuf, A1: [Mp x ld] with Kc live columns; gm, gv: [Kc][R].
// cond_backward_main (main stream): dKuf [M x ld], gvs [Kc] = sum_r gv (= d ELBO / d Knn), dq_mu; enqueues the chain's first part (W_r -> dG_r
//   -> dq_sqrt and its term of dL) on the chain stream behind ev_g[0] and marks its own end with ev_g[1].
// cond_backward_finish (chain stream, behind ev_g[1]): dL's other terms and the Cholesky adjoint, S = d ELBO / dKuu (data part) [M x M, ld Mp];
//   s_acc: S already holds the KL part (kl_products ran first): add to it.  Marks its end with ev_g[2].
// dl_on_main: dL's term from dK_uf is formed on the main stream as well (the last layer of the reverse pass: nothing follows it there, and the
// chain is what the step ends on).
int cond_backward_main(Bk& bk, const Lanes& ln, LayerState& L, const double* A1, long ld, long Kc, const double* gm, const double* gv, double* dKuf,
                       double* gvs, bool dl_on_main) {
  dcgp_ctx* ctx = bk.ctx;
  const int M = L.M, Mp = L.Mp, R = L.R, Rp = L.g.Rp;
  const long mm = (long)Mp * Mp;
  const GpMats& g = L.g;
  if (ln.forked) HIP_TRY(ctx, hipEventRecord(ctx->ev_g[0], ln.main));   // A1 and gv are there: the chain may start
  hipLaunchKernelGGL(rowsum_small_kernel, dim3(blocks_for(Kc)), dim3(256), 0, ctx->stream, gv, Kc, R, gvs);
  LAUNCH_CHECK(ctx);
  // The column-wise part of the adjoint -- dT, dA1, dK_uf -- in one strip-resident launch where the shape allows and there are
  // enough columns to fill the chip (conv_bwd_fused.hip); its operand S_r = G_r G_r^T is parameter-only.
  ConvBwdArgs fb;
  fb.A1 = A1; fb.ld = ld; fb.Kc = (int)Kc; fb.alpha = L.g.alpha; fb.Rp = Rp; fb.Linv = L.g.Linv; fb.gv = gv; fb.gm = gm; fb.gvs = gvs;
  fb.M = M; fb.Mp = Mp; fb.R = R; fb.dKuf = dKuf;
  const long min_cols = ctx->opt.fused_bwd_min_cols >= 0 ? ctx->opt.fused_bwd_min_cols : 4096;   // (tests: the strip kernel at sizes the oracle checks)
  const bool fused_bwd = L.has_qsqrt && !L.white && Kc >= min_cols && conv_bwd_fused_ok(ctx, fb);
  double* dA1 = fused_bwd ? nullptr : bk.ws("dA1", (size_t)Mp * ld);
  double* dalpha = bk.ws("dalpha", (size_t)Mp * Rp);
  double* dG = bk.ws("dG", (size_t)R * mm);
  double* dL = bk.ws("dL", (size_t)mm);
  if (!fused_bwd) NEED(dA1);
  NEED(dalpha); NEED(dG); NEED(dL);
  const long Rm = (long)R * Mp;
  double* GT = nullptr;
  if (L.has_qsqrt) {
    GT = bk.ws("GT", (size_t)R * mm);
    NEED(GT);
  }
  // (parameter-only operands: G^T stacked, S_r = G_r G_r^T, the factor's lower triangle -- already there when grad_kl_early prepared them)
  if (!(bk.prep & 1)) DCGP_TRY(param_operands(bk, L, false));
  if (fused_bwd) {
    if (!(bk.prep & 2)) DCGP_TRY(param_operands(bk, L, true));
    fb.S = bk.ws("Sgg", (size_t)R * mm);
    NEED(fb.S);
  }
  if (!(bk.prep & 1) && ln.forked) HIP_TRY(ctx, hipEventRecord(ctx->ev_g[0], ln.main));   // (the chain reads G^T: behind the launch that made it)
  // main stream: dT, dA1, dK_uf on the tuned kernels ...
  if (fused_bwd) {
    // (the chain's W_r contraction runs BESIDE this launch also where both fill the chip -- tens of thousands of columns: started behind it
    // instead, the tiled step took 4.07 ms against 3.90)
    DCGP_TRY(conv_bwd_fused(ctx, fb));
  } else {
    int dA1_acc = 0;
    // the padded rows M..Mp-1 of dA1 are operands of the gemm_tn launch that forms dK_uf (times zeros of inv(L)'s padding):
    // they must be finite whichever path writes the live rows
    if (Mp > M) HIP_TRY(ctx, hipMemsetAsync(dA1 + (size_t)M * ld, 0, (size_t)(Mp - M) * ld * sizeof(double), ctx->stream));
    if (L.has_qsqrt) {
      double* dT = bk.ws("dT", (size_t)R * Mp * ld);
      NEED(dT);
      const bool tn_ok = (long)Mp * ld * 8 < (1L << 31);
      if (tn_ok) {   // dT_r = 2 (G_r^T A1) o gv_r: the forward's stage-3 product, stored, columns scaled in the epilogue
        GemmArgs a;
        a.Wt = g.G; a.ldw = Mp; a.wBatch = mm; a.nW = R;
        a.B = A1; a.ldb = (int)ld;
        a.C = dT; a.ldc = (int)ld; a.cBatch = (long)Mp * ld;
        a.cscale = gv; a.csCol = R; a.csBatch = 1; a.calpha = 2.0;
        a.Mi = Mp; a.Mk = Mp; a.Kc = (int)Kc; a.tri = 2;
        DCGP_TRY(gemm_tn(ctx, a, nullptr));
      } else {
        GenGemm t = mk(g.G, 1, Mp, A1, ld, 1, dT, ld, Mp, (int)Kc, Mp);
        t.batch = R; t.a_bs = mm; t.c_bs = (long)Mp * ld; t.alpha = 2.0; t.colscale = gv; t.cs_s = R; t.cs_bs = 1;
        DCGP_TRY(gemm_gen(ctx, t));
      }
      // dA1 = sum_r G_r dT_r: ONE product with the R blocks stacked along k (GT [R Mp x Mp], dT [R Mp x ld])
      // (few columns -- a de-duplicated first layer, the head: the 72-workgroup launch would be one long k chain; gemm_gen splits k)
      if (Rm * ld * 8 < (1L << 31) && Kc >= 16384) {
        GemmArgs a;
        a.Wt = GT; a.ldw = Mp;
        a.B = dT; a.ldb = (int)ld;
        a.C = dA1; a.ldc = (int)ld;
        a.Mi = Mp; a.Mk = (int)Rm; a.Kc = (int)Kc; a.tri = 0;
        DCGP_TRY(gemm_tn(ctx, a, nullptr));
      } else {
        DCGP_TRY(gemm_gen(ctx, mk(GT, 1, Mp, dT, ld, 1, dA1, ld, M, (int)Kc, (int)Rm)));
      }
      dA1_acc = 1;
    }
    // dA1 (+)= alpha gm^T - 2 A1 o gvs
    {
      GenGemm a = mk(g.alpha, Rp, 1, gm, 1, R, dA1, ld, M, (int)Kc, R);
      a.accumulate = dA1_acc;
      DCGP_TRY(gemm_gen(ctx, a));
    }
    hipLaunchKernelGGL(dA1_fix_kernel, dim3(blocks_for(Kc), M), dim3(256), 0, ctx->stream, dA1, A1, gvs, M, Kc, ld);
    LAUNCH_CHECK(ctx);
    // dKuf = inv(L)^T dA1
    if ((long)Mp * ld * 8 < (1L << 31)) {   // inv(L) row-major IS the k-major operand of inv(L)^T; upper-triangular product
      GemmArgs a;
      a.Wt = g.Linv; a.ldw = Mp;
      a.B = dA1; a.ldb = (int)ld;
      a.C = dKuf; a.ldc = (int)ld;
      a.Mi = Mp; a.Mk = Mp; a.Kc = (int)Kc; a.tri = 2;
      DCGP_TRY(gemm_tn(ctx, a, nullptr));
    } else {
      DCGP_TRY(gemm_gen(ctx, mk(g.Linv, 1, Mp, dA1, ld, 1, dKuf, ld, M, (int)Kc, M)));
    }
  }
  if (bk.data_only) return DCGP_OK;   // dK_uf and gvs are all the data path reads
  // ... then d alpha = A1 gm and dq_mu = d alpha (whitened) or inv(L)^T d alpha.  (d alpha used to open the chain: beside the strip kernel
  // its 288 small workgroups took 108 us instead of 8, in front of W_r.)
  DCGP_TRY(gemm_gen(ctx, mk(A1, ld, 1, gm, R, 1, dalpha, Rp, M, R, (int)Kc)));
  if (L.white) {
    hipLaunchKernelGGL(copy2d_kernel, dim3(blocks_for(R), M), dim3(256), 0, ctx->stream, dalpha, (long)Rp, L.gq_mu, (long)R, M, R, 1.0, 0);
    LAUNCH_CHECK(ctx);
  } else {
    DCGP_TRY(gemm_gen(ctx, mk(g.Linv, 1, Mp, dalpha, Rp, 1, L.gq_mu, R, M, R, M)));
  }
  if (!L.white) DCGP_TRY(dl_term_mu(bk, L, dL));
  if (dl_on_main) DCGP_TRY(dl_term_kuf(bk, L, A1, ld, Kc, dKuf, dL));
  if (ln.forked) HIP_TRY(ctx, hipEventRecord(ctx->ev_g[1], ln.main));   // dK_uf, dq_mu and dL's first term(s) are there
  // The chain's first part, ENQUEUED behind the launches above (one host thread feeds the streams at ~4 us a launch; with few columns -- the
  // head -- the main stream's launches are as short as that: fed second, it sat idle while the host was busy with the chain's).
  if (L.has_qsqrt) {
    OnStream on(ctx, ln.chain, ctx->ev_g[0]);
    if (!on.ok) return ctx_fail(ctx, DCGP_ERR_HIP, "grad: stream wait failed");
    // dG_r = tril(A1 dT_r^T) = tril(W_r G_r),  W_r = 2 A1 diag(gv_r) A1^T (symmetric).  Both operands of the long
    // contraction are then A1 itself (94 MB at the headline size: it stays in the 256 MB Infinity Cache across the R
    // batches, where the R x larger dT would stream from HBM); lower tiles only, stored to both triangles.
    double* Wr = bk.ws("Wr", (size_t)R * mm);
    NEED(Wr);
    GenGemm w = mk(A1, ld, 1, A1, 1, ld, Wr, Mp, M, M, (int)Kc);
    // (the k scaling reads gv [Kc][R] in place, stride R: a transposed copy used to cost 290 us of scattered 8-byte stores per step)
    w.batch = R; w.c_bs = mm; w.lower_only = 1; w.mirror = 1; w.alpha = 2.0; w.kscale = gv; w.ks_s = R; w.ks_bs = 1;
    {
      ScopedTimer t(ctx, L.is_head ? "grad_wr_head" : "grad_wr");   // (bench.py: roofline_train)
      DCGP_TRY(gemm_gen(ctx, w));
    }
    GenGemm d = mk(Wr, Mp, 1, g.G, Mp, 1, dG, Mp, M, M, M);
    d.batch = R; d.a_bs = mm; d.b_bs = mm; d.c_bs = mm; d.lower_only = 1;
    DCGP_TRY(gemm_gen(ctx, d));
    if (L.white) {
      hipLaunchKernelGGL(mask_lower_kernel, dim3(blocks_for(M), M, R), dim3(256), 0, ctx->stream, dG, (long)Mp, mm, L.gq_sqrt, (long)M,
                         (long)M * M, M, 1.0, 0);
      LAUNCH_CHECK(ctx);
    } else {
      double* Bm = bk.ws("Bm", (size_t)R * mm);                      // B_r = inv(L)^T dG_r, stored [i][r][k]
      NEED(Bm);
      if (Mp > M) HIP_TRY(ctx, hipMemsetAsync(Bm, 0, (size_t)R * mm * sizeof(double), ctx->stream));   // (the padded k of the stacked product below)
      GenGemm b = mk(g.Linv, 1, Mp, dG, Mp, 1, Bm, Rm, M, M, M);
      b.batch = R; b.b_bs = mm; b.c_bs = Mp;
      DCGP_TRY(gemm_gen(ctx, b));
      hipLaunchKernelGGL(mask_lower_kernel, dim3(blocks_for(M), M, R), dim3(256), 0, ctx->stream, Bm, Rm, (long)Mp, L.gq_sqrt, (long)M,
                         (long)M * M, M, 1.0, 0);
      LAUNCH_CHECK(ctx);
      if (ln.forked) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_g[1], 0));   // (dL's first writer is on the main stream)
      GenGemm l2 = mk(Bm, Rm, 1, GT, Mp, 1, dL, Mp, M, M, (int)Rm);   // dL -= tril(sum_r B_r G_r^T), stacked along k
      l2.alpha = -1.0; l2.lower_only = 1; l2.accumulate = 1;
      DCGP_TRY(gemm_gen(ctx, l2));
    }
    if (ln.forked) HIP_TRY(ctx, hipEventRecord(ctx->ev_g[4], ctx->stream));   // dq_sqrt is there
  }
  return DCGP_OK;
}

int cond_backward_finish(Bk& bk, const Lanes& ln, LayerState& L, const double* A1, long ld, long Kc, const double* dKuf, double* S, bool s_acc,
                         bool dl_on_main) {
  dcgp_ctx* ctx = bk.ctx;
  const int M = L.M, Mp = L.Mp;
  const long mm = (long)Mp * Mp;
  const GpMats& g = L.g;
  OnStream on(ctx, ln.chain, ctx->ev_g[1]);
  if (!on.ok) return ctx_fail(ctx, DCGP_ERR_HIP, "grad: stream wait failed");
  double* dL = bk.ws("dL", (size_t)mm);
  double* Lc = bk.ws("Lc", (size_t)mm);
  double* Pm = bk.ws("Pm", (size_t)mm);
  double* S1 = bk.ws("S1", (size_t)mm);
  NEED(dL); NEED(Lc); NEED(Pm); NEED(S1);
  // dL = -tril(dq_mu alpha^T [main stream, unwhitened] + sum_r B_r G_r^T [the chain's first part, unwhitened with q_sqrt] + dKuf A1^T)
  if (!dl_on_main) DCGP_TRY(dl_term_kuf(bk, L, A1, ld, Kc, dKuf, dL));
  // Cholesky adjoint: S = inv(L)^T Phi(L^T dL) inv(L)
  GenGemm ph = mk(Lc, 1, Mp, dL, Mp, 1, Pm, Mp, M, M, M);
  ph.phi = 1;   // Phi(L^T dL) in the product's epilogue
  DCGP_TRY(gemm_gen(ctx, ph));
  DCGP_TRY(gemm_gen(ctx, mk(g.Linv, 1, Mp, Pm, Mp, 1, S1, Mp, M, M, M)));
  GenGemm sf = mk(S1, Mp, 1, g.Linv, Mp, 1, S, Mp, M, M, M);
  if (s_acc) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_kl3, 0));   // S holds the KL part, written on the auxiliary stream
  sf.accumulate = s_acc ? 1 : 0;
  DCGP_TRY(gemm_gen(ctx, sf));
  if (ln.forked) HIP_TRY(ctx, hipEventRecord(ctx->ev_g[2], ctx->stream));
  return DCGP_OK;
}

// K_uf adjoint of the layer's base kernel: E [M x Kc], its column sums cs and the kernel's hyper-parameter sums (into the layer's scalar slots) from
// dK = d ELBO / dK_uf and the stored K.  Column c reads dK[m][c / pdiv], times w[c % pdiv] * wscale where w is given (the head's patch weights; raw
// then gets the unweighted column sums, for d w).  RBF: E = dK o K.  Matern: E = dK o (-2 dk/drho) over the product Z Xcol^T, then the RBF's form
// as it is.  ArcCosine: E = F1, cs = colsum(F2) / A, and out: rs = rowsum(F2) / Q, cz = the weight variance, which patch_backward takes in the
// place of rowsum(E) and 1 / l^2.  The chunks' sums are added by a second launch, except that the RBF kernel with one chunk writes cs (and raw) itself.
struct KufAdjoint { const double* rs = nullptr; double cz = 0.0; };
int kuf_adjoint(Bk& bk, LayerState& L, const double* dK, long lddk, int pdiv, const double* w, double wscale, const double* K, long ldk,
                const double* Xcol, long Kc, double* E, long lde, double* cs, double* raw, KufAdjoint* out) {
  dcgp_ctx* ctx = bk.ctx;
  const int M = L.M, Ld = L.v.L, bt = L.base_type;
  if (bt != 0 && (pdiv != 1 || w || raw || lddk != lde || ldk != lde)) return ctx_fail(ctx, DCGP_ERR_ARG, "grad: only the RBF adjoint takes patch weights or mixed leading dimensions");
  const RowChunks rc = row_chunks(M, Kc);
  const dim3 grid(rc.nb, rc.chunks);
  const long np = (long)rc.nb * rc.chunks;
  const bool direct = bt == 0 && rc.chunks == 1;
  double* pv = bk.ws("ef_pv", np);
  double* pl = bk.ws("ef_pl", np);                                   // lengthscale | ArcCosine weight variance
  double* pb = bt == 1 ? bk.ws("ef_pb", np) : nullptr;               // ArcCosine bias variance
  double* csp = direct ? cs : bk.ws("ef_csp", (size_t)rc.chunks * Kc);
  double* rawp = raw && !direct ? bk.ws("ef_rawp", (size_t)rc.chunks * Kc) : raw;
  double* xn = bt == 0 ? nullptr : bk.ws(bt == 1 ? "acos_xn" : "mat_xn", Kc);
  double* F2 = bt == 1 ? bk.ws("acos_F2", (size_t)L.Mp * lde) : nullptr;
  NEED(pv); NEED(pl); NEED(csp);
  if (raw) NEED(rawp);
  double lscale = 1.0;   // of the second sum (the variance sum: 1 / variance throughout)
  if (bt != 0) {
    NEED(xn);
    hipLaunchKernelGGL(rownorm_kernel, dim3(blocks_for(Kc)), dim3(256), 0, ctx->stream, Xcol, Kc, Ld, xn);
    LAUNCH_CHECK(ctx);
  }
  if (bt == 0) {
    hipLaunchKernelGGL(e_form_kernel, grid, dim3(256), 0, ctx->stream, dK, lddk, pdiv, w, wscale, K, ldk, E, lde, M, rc.rpc, Kc, 1.0 / L.variance,
                       2.0 * L.ls * L.ls, csp, rawp, pv, pl);
    lscale = 1.0 / (L.ls * L.ls * L.ls);
  } else if (bt == 1) {
    NEED(F2); NEED(pb);
    hipLaunchKernelGGL(acos_e_form_kernel, grid, dim3(256), 0, ctx->stream, dK, E, lde, K, F2, M, rc.rpc, Kc, L.variance, L.acos_w, L.acos_b, L.zn, xn,
                       csp, pv, pl, pb);
  } else {
    DCGP_TRY(gemm_gen(ctx, mk(L.Z, Ld, 1, Xcol, 1, Ld, E, lde, M, (int)Kc, Ld)));   // z_m . x_c
    const double inv_l2 = 1.0 / (L.ls * L.ls);
    hipLaunchKernelGGL(bt == 2 ? matern_e_form_kernel<2> : matern_e_form_kernel<3>, grid, dim3(256), 0, ctx->stream, dK, E, lde, K, M, rc.rpc, Kc,
                       L.variance, inv_l2, L.zn, xn, csp, pv, pl);
    lscale = inv_l2 / L.ls;
  }
  LAUNCH_CHECK(ctx);
  if (!direct) {
    if (raw) hipLaunchKernelGGL(sum_chunks2_kernel, dim3(blocks_for(Kc)), dim3(256), 0, ctx->stream, csp, rawp, rc.chunks, Kc, cs, raw);
    else hipLaunchKernelGGL(sum_chunks_kernel, dim3(blocks_for(Kc)), dim3(256), 0, ctx->stream, csp, rc.chunks, Kc, cs);
    LAUNCH_CHECK(ctx);
  }
  DCGP_TRY(add_scalars(bk, L, {{0, pv, np, 1.0 / L.variance}, {1, pl, np, lscale}, {2, pb, np, 1.0}}));
  if (bt == 1) {   // rowsum(F2) / Q
    double* rs = bk.ws("acos_rs", M);
    NEED(rs);
    DCGP_TRY(row_sums(bk, F2, lde, Kc, M, rs));
    hipLaunchKernelGGL(acos_divide_kernel, dim3(blocks_for(M)), dim3(256), 0, ctx->stream, rs, L.zn, M, L.acos_w, L.acos_b);
    LAUNCH_CHECK(ctx);
    *out = {rs, L.acos_w};
  }
  return DCGP_OK;
}

// the zero fills in front of a layer's reverse pass: scalar slots, gradient block
int layer_fills(Bk& bk, LayerState& L) {
  DCGP_TRY(L.ensure_grads());
  HIP_TRY(bk.ctx, hipMemsetAsync(L.gslots, 0, 48 * sizeof(double), bk.ctx->stream));
  if (L.grad_block_count() * sizeof(double) <= (8u << 20)) {   // a small block ([Z | q_mu | q_sqrt | w | gscal | gard], contiguous): one fill
    HIP_TRY(bk.ctx, hipMemsetAsync(L.gZ, 0, L.grad_block_count() * sizeof(double), bk.ctx->stream));
    return DCGP_OK;
  }
  HIP_TRY(bk.ctx, hipMemsetAsync(L.gZ, 0, (size_t)L.M * L.v.L * sizeof(double), bk.ctx->stream));
  HIP_TRY(bk.ctx, hipMemsetAsync(L.gw, 0, ((size_t)L.v.P + 3 + L.ard_slots() + L.lik_slots + L.mean_slots() + L.mix_slots()) * sizeof(double), bk.ctx->stream));   // gw, gscal, gard, glik, gmean_W, gmix_W
  if (!L.has_qsqrt) HIP_TRY(bk.ctx, hipMemsetAsync(L.gq_sqrt, 0, (size_t)L.R * L.M * L.M * sizeof(double), bk.ctx->stream));
  return DCGP_OK;
}
int begin_layer(Bk& bk, LayerState& L) {
  bk.slot_v = bk.slot_l = bk.slot_b = 0;
  bk.pending.clear();
  if (bk.data_only) return DCGP_OK;  // no gradient block is written
  if (bk.prep & 1) return DCGP_OK;   // grad_kl_early ran the fills beside the forward pass
  return layer_fills(bk, L);
}
int end_layer(Bk& bk, LayerState& L) {
  DCGP_TRY(flush_scalars(bk));
  hipLaunchKernelGGL(scal_finish_kernel, dim3(1), dim3(64), 0, bk.ctx->stream, L.gslots, L.gscal);
  LAUNCH_CHECK(bk.ctx);
  return DCGP_OK;
}

// row chunks of ard_xsum_kernel on Kc patch rows: a few hundred blocks of 256 rows or more
struct ArdChunks { int chunks; long rpc; };
ArdChunks ard_chunks(long Kc) {
  const long chunks = std::max<long>(1, std::min<long>(512, (Kc + 255) / 256));
  const long rpc = (Kc + chunks - 1) / chunks;
  return {(int)((Kc + rpc - 1) / rpc), rpc};
}

// What is left of a layer, on the tail stream.  Behind the conditional's own dq_mu / dq_sqrt (ev_g[1], ev_g[4]): the KL pieces.  Behind
// S = d ELBO / dKuu (ev_g[2]): the Gram adjoint of K_uu, whose product adds into the dZ the main stream's patch adjoint adds into (behind
// ev_g[3]).  Last the layer's scalar sums.  kd: d ELBO / d Knn per column (conv layers) or null.
int layer_tail(Bk& bk, const Lanes& ln, LayerState& L, const double* S, const double* kd, long n_kd, bool frozen_prior) {
  dcgp_ctx* ctx = bk.ctx;
  OnStream on(ctx, ln.tail, ctx->ev_g[1]);
  if (!on.ok) return ctx_fail(ctx, DCGP_ERR_HIP, "grad: stream wait failed");
  if (kd) DCGP_TRY(add_scalar(bk, L, 0, kd, n_kd, 1.0));          // Knn = variance on every column
  const bool kl_first = bk.kl_early || frozen_prior || L.white;   // (otherwise the KL products add into S: behind it)
  if (ln.forked && L.has_qsqrt) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_g[4], 0));
  if (kl_first) {
    if (!bk.kl_early) DCGP_TRY(kl_products(bk, L, nullptr, false));
    DCGP_TRY(kl_apply(bk, L, frozen_prior));
  }
  if (ln.forked) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_g[2], 0));
  if (!kl_first) {
    DCGP_TRY(kl_products(bk, L, const_cast<double*>(S), false));
    DCGP_TRY(kl_apply(bk, L, frozen_prior));
  }
  if (L.in_scale && !L.is_head) {
    // ARD conv layer (conv_backward): the Gram adjoint on the scaled rows, then the chain rule through the scaling.  Everything it reads is there:
    // the patch adjoint's dZs and the patches' sums behind ev_g[3] (waited for inside kuu_backward), the prior's share behind kl_apply
    const size_t nz = (size_t)L.M * L.v.L;
    double *Zs = bk.ws("Zs", nz), *dZs = bk.ws("dZs", nz);
    NEED(Zs); NEED(dZs);
    DCGP_TRY(kuu_backward(bk, L, Zs, S, L.Mp, true, dZs, "kuu", false, ln.forked ? ctx->ev_g[3] : nullptr));
    const bool prior = !L.white;
    const ArdChunks ac = ard_chunks(n_kd);
    double* xpart = bk.ws("ard_xpart", (size_t)ac.chunks * L.v.L);
    NEED(xpart);
    hipLaunchKernelGGL(ard_conv_finish_kernel, dim3(L.v.L), dim3(256), 0, ctx->stream, dZs, Zs, prior ? bk.ws("klz_dZs", nz) : nullptr,
                       prior ? bk.ws("klz_Zs", nz) : nullptr, L.M, L.v.L, xpart, ac.chunks, L.in_scale, L.gZ, L.gard);
    LAUNCH_CHECK(ctx);
    DCGP_TRY(end_layer(bk, L));
    // the scalar "lengthscale" slot collected d / d(unit lengthscale): meaningless here, and L.ls must stay 1 (as for the dense head)
    HIP_TRY(ctx, hipMemsetAsync(L.gscal + 1, 0, sizeof(double), ctx->stream));
  } else {
    DCGP_TRY(kuu_backward(bk, L, L.Z, S, L.Mp, true, nullptr, "kuu", false, ln.forked ? ctx->ev_g[3] : nullptr));
    DCGP_TRY(end_layer(bk, L));
  }
  if (ln.forked) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev_kl, ctx->stream));
    bk.side_pending = true;
  }
  return DCGP_OK;
}

// dXin [rows, H, W, C] from E and cs in one launch (fuse_dx: input_grad.hip, `extra` as there) or from the patch gradients dXcol by col2im's gather
// sc: nullptr, or [L]: dXcol is the gradient of the patches times sc (an ARD conv layer; not with fuse_dx)
int patches_to_dx(Bk& bk, LayerState& L, bool fuse_dx, const double* E, long ld, const double* cs, const double* Xin, int rows, int n_mod,
                  const double* extra, const double* dXcol, double* dXin, const double* sc = nullptr) {
  if (fuse_dx) return sc ? ctx_fail(bk.ctx, DCGP_ERR_ARG, "grad: the one-launch patch adjoint takes no patch scale") : patch_adjoint_fused(bk.ctx, L, E, ld, cs, Xin, rows, n_mod, extra, dXin);
  const long n = (long)rows * L.v.H * L.v.W * L.v.C;
  hipLaunchKernelGGL(sc ? col2im_kernel<true> : col2im_kernel<false>, dim3(blocks_for(n)), dim3(256), 0, bk.ctx->stream, dXcol, rows, L.v.H, L.v.W, L.v.C,
                     L.v.f, L.v.s, L.v.Ho, L.v.Wo, L.v.L, dXin, sc);
  LAUNCH_CHECK(bk.ctx);
  return DCGP_OK;
}

// ConvLayer backward.  Xin: the layer's input images ([n_mod, H, W, C], row n reads image n % n_mod); gm / gv [rows * P][R].
int conv_backward(Bk& bk, LayerState& L, const double* Xin, int rows, int n_mod, const double* gm, const double* gv, double* dXin) {
  dcgp_ctx* ctx = bk.ctx;
  const int Mp = L.Mp, P = L.v.P, Ld = L.v.L;
  const long Kc = (long)rows * P, ld = col_ld(Kc);
  Lanes ln = lanes_of(ctx);
  if (bk.data_only) { ln.forked = false; ln.chain = ln.tail = ln.main; }
  DCGP_TRY(begin_layer(bk, L));
  const double* gmf = gm;   // the mean function's adjoint: d / d mean of the layer's maps
  if (L.mix_W) {
    if (!bk.mix_gF || !bk.mix_gF_all) return ctx_fail(ctx, DCGP_ERR_ARG, "grad: a mixed layer takes its gradient from the layer above it");
    gmf = bk.mix_gF;
    if (!bk.data_only && L.mix_trainable) {   // gW behind the block's fill (a frozen matrix keeps its zero)
      int nwg; long cpw;
      mix_w_plan(bk.mix_cols, &nwg, &cpw);
      double* part = bk.ws("mix_part", (size_t)nwg * L.mix_slots());
      NEED(part);
      DCGP_TRY(mix_backward_w(ctx, L.R, L.Rout, L.lat_sample, bk.mix_gF_all, bk.mix_cols, part, L.gmix_W));
    }
  }
  // forward leftovers (conv_forward / cond_core workspaces)
  const double* Kuf = forward_left(bk, "Kuf", 0, "K_uf / A1 for this layer");
  const double* A1 = forward_left(bk, "A1", (size_t)Mp * ld * sizeof(double), "K_uf / A1 for this layer");
  if (!Kuf || !A1) return DCGP_ERR_ARG;
  double* dKuf = bk.ws("dKuf", (size_t)Mp * ld);
  double* E = bk.ws("E", (size_t)Mp * ld);       // (not over dK_uf: the chain stream still reads that)
  double* S = bk.ws("S", (size_t)Mp * Mp);
  double* gvs = bk.ws("gvs", Kc);
  double* cs = bk.ws("cs", Kc);
  double* Xcol = bk.ws("Xcol", (size_t)Kc * Ld);
  NEED(dKuf); NEED(E); NEED(S); NEED(gvs); NEED(cs); NEED(Xcol);
  // ARD (per-dimension lengthscales, L.in_scale; L.ls == 1): dense_head_backward's scheme on the patches.  The unit-lengthscale adjoints below run on
  // the scaled copies Xcol o s (im2col scales while it gathers) and Zs = Z o s and leave dZs / dXs; col2im applies s to dXs on its way to dX, and
  // layer_tail ends with gZ = s o dZs and gard_l = -s_l (sum_m dZs Zs + sum_k dXs Xs + the frozen prior's share).  dXs is formed on the first layer
  // too, where no dX is wanted: the lengthscale gradient needs it.
  const double* sc = L.in_scale;
  double *Zs = nullptr, *dZs = nullptr;
  if (sc) {
    Zs = bk.ws("Zs", (size_t)L.M * Ld); NEED(Zs);
    hipLaunchKernelGGL(scale_rows_kernel, dim3(blocks_for((long)L.M * Ld)), dim3(256), 0, ctx->stream, L.Z, L.M, (long)L.M, Ld, sc, Zs);   // (ahead of ev_g[1]: the tail stream reads it)
    LAUNCH_CHECK(ctx);
    if (!bk.data_only) {
      dZs = bk.ws("dZs", (size_t)L.M * Ld); NEED(dZs);
      HIP_TRY(ctx, hipMemsetAsync(dZs, 0, (size_t)L.M * Ld * sizeof(double), ctx->stream));
    }
  }
  // main stream: the column-wise adjoint of the conditional, then the patch-kernel adjoint -> dX.  The M x M chain behind the conditional
  // runs beside them on the chain stream, what needs its result on the tail stream (Lanes).
  DCGP_TRY(cond_backward_main(bk, ln, L, A1, ld, Kc, gm, gv, dKuf, gvs, bk.last_layer && ln.forked));
  // the input gradient's pass: dX in one launch from E and cs where the shape is covered (input_grad.hip) -- no Xcol, no dXcol, no col2im
  const bool fuse_dx = bk.data_only && dXin && patch_adjoint_fused_ok(L, rows);
  if (!fuse_dx) DCGP_TRY(im2col(ctx, L, Xin, n_mod, Kc, Xcol, sc));
  double* dXcol = nullptr;
  if ((dXin && !fuse_dx) || (sc && !bk.data_only)) { dXcol = bk.ws("dXcol", (size_t)Kc * Ld); NEED(dXcol); }
  KufAdjoint ka;
  DCGP_TRY(kuf_adjoint(bk, L, dKuf, ld, 1, nullptr, 1.0, Kuf, ld, Xcol, Kc, E, ld, cs, nullptr, &ka));
  DCGP_TRY(patch_backward(bk, L, E, ld, Kc, cs, Xcol, dXcol, 0, Zs, dZs, ka.rs, ka.cz));
  if (sc && !bk.data_only) {   // the patches' share of the lengthscale gradient, before dXs is consumed
    const ArdChunks ac = ard_chunks(Kc);
    double* xpart = bk.ws("ard_xpart", (size_t)ac.chunks * Ld);
    NEED(xpart);
    hipLaunchKernelGGL(ard_xsum_kernel, dim3(ac.chunks), dim3(256), 0, ctx->stream, dXcol, Xcol, Kc, Ld, ac.rpc, xpart);
    LAUNCH_CHECK(ctx);
  }
  if (dXin) {
    DCGP_TRY(patches_to_dx(bk, L, fuse_dx, E, ld, cs, Xin, rows, n_mod, nullptr, dXcol, dXin, sc));
    if (L.identity_mean) {
      hipLaunchKernelGGL(idmean_backward_kernel, dim3(blocks_for(Kc)), dim3(256), 0, ctx->stream, gmf, Kc, L.R, P, L.v.Wo, L.v.H, L.v.W, L.v.C,
                         L.v.f, L.v.s, dXin);
      LAUNCH_CHECK(ctx);
    }
    if (L.mean_W) DCGP_TRY(conv_mean_backward_dx(ctx, L, gmf, rows, dXin));   // the filter mean's adjoint (conv_mean.hip): gm is d / d mean, as the oracle uses it
  }
  if (bk.data_only) return DCGP_OK;
  // the filter's own gradient from the patches the pass holds (a frozen filter keeps the zero of the block's fill)
  if (L.mean_W && L.mean_trainable) {
    const double* Xraw = Xcol;
    if (sc) {   // the filter sees the patches themselves, not patches o s
      double* xr = bk.ws("Xraw", (size_t)Kc * Ld);
      NEED(xr);
      DCGP_TRY(im2col(ctx, L, Xin, n_mod, Kc, xr));
      Xraw = xr;
    }
    DCGP_TRY(conv_mean_backward_filter(ctx, L, Xraw, gmf, Kc, L.gmean_W));
  }
  // The main stream's part of this layer ends here (dX is out): it goes straight on to the layer below.
  if (ln.forked) HIP_TRY(ctx, hipEventRecord(ctx->ev_g[3], ctx->stream));
  DCGP_TRY(cond_backward_finish(bk, ln, L, A1, ld, Kc, dKuf, S, false, bk.last_layer && ln.forked));
  return layer_tail(bk, ln, L, S, gvs, Kc, true);
}

// Dense head backward: gpflow RBF(D, ARD=True) on the flattened features (--last-kernel rbf, conv_gp/models.py:160-168).
// The forward divides x and Z by the lengthscales while staging (in_scale) and runs the unit-lengthscale kernel
// (L.ls == 1), so every kernel adjoint below is the generic one on the scaled copies Xs = X o s, Zs = Z o s; the chain
// rule back through the scaling gives dZ, dX and the per-dimension lengthscale gradient (ard_finish_kernel).
int dense_head_backward(Bk& bk, LayerState& L, const double* Xin, int rows, int n_mod, const double* gm, const double* gv, double* dXin) {
  dcgp_ctx* ctx = bk.ctx;
  const int M = L.M, Mp = L.Mp, D = L.v.L;
  const long ld = col_ld(rows);
  if (L.v.P != 1 || L.kernel_type != 0) return ctx_fail(ctx, DCGP_ERR_ARG, "grad: ARD lengthscales need the single-patch head");
  DCGP_TRY(begin_layer(bk, L));
  const double* Kzx = forward_left(bk, "Kzx", 0, "K_zx for the head");
  if (!Kzx) return DCGP_ERR_ARG;
  double* A1 = bk.ws("A1h", (size_t)Mp * ld);
  double* dKzx = bk.ws("dKzx", (size_t)Mp * ld);
  double* S = bk.ws("S", (size_t)Mp * Mp);
  double* gkd = bk.ws("gkd", rows);
  double* cs = bk.ws("cs", rows);
  double* Zs = bk.ws("Zs", (size_t)M * D);
  double* Xs = bk.ws("Xs", (size_t)rows * D);
  double* dZs = bk.ws("dZs", (size_t)M * D);
  double* dXs = bk.ws("dXs", (size_t)rows * D);
  NEED(A1); NEED(dKzx); NEED(S); NEED(gkd); NEED(cs); NEED(Zs); NEED(Xs); NEED(dZs); NEED(dXs);
  if (Mp > M) HIP_TRY(ctx, hipMemsetAsync(A1 + (size_t)M * ld, 0, (size_t)(Mp - M) * ld * sizeof(double), ctx->stream));
  DCGP_TRY(gemm_gen(ctx, mk(L.g.Linv, Mp, 1, Kzx, ld, 1, A1, ld, M, rows, M)));
  Lanes ln = lanes_of(ctx);
  ln.forked = false; ln.chain = ln.tail = ln.main;   // (a few hundred columns, one patch: everything in line on the main stream)
  DCGP_TRY(cond_backward_main(bk, ln, L, A1, ld, rows, gm, gv, dKzx, gkd, false));
  if (!bk.data_only) {
    DCGP_TRY(cond_backward_finish(bk, ln, L, A1, ld, rows, dKzx, S, bk.kl_early && !L.white, false));
    if (!bk.kl_early) DCGP_TRY(kl_products(bk, L, L.white ? nullptr : S, false));
    DCGP_TRY(kl_apply(bk, L, false));
    DCGP_TRY(add_scalar(bk, L, 0, gkd, rows, 1.0));             // Kdiag = variance
  }
  hipLaunchKernelGGL(scale_rows_kernel, dim3(blocks_for((long)M * D)), dim3(256), 0, ctx->stream, L.Z, M, (long)M, D, L.in_scale, Zs);
  LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(scale_rows_kernel, dim3(blocks_for((long)rows * D)), dim3(256), 0, ctx->stream, Xin, n_mod, (long)rows, D, L.in_scale, Xs);
  LAUNCH_CHECK(ctx);
  if (!bk.data_only) {
    HIP_TRY(ctx, hipMemsetAsync(dZs, 0, (size_t)M * D * sizeof(double), ctx->stream));
    DCGP_TRY(kuu_backward(bk, L, Zs, S, Mp, true, dZs));
  }
  KufAdjoint ka;
  DCGP_TRY(kuf_adjoint(bk, L, dKzx, ld, 1, nullptr, 1.0, Kzx, ld, Xs, rows, dKzx, ld, cs, nullptr, &ka));   // E over dKzx (P == 1: K_zx is the full response)
  DCGP_TRY(patch_backward(bk, L, dKzx, ld, rows, cs, Xs, dXs, 0, Zs, dZs, ka.rs, ka.cz));
  if (bk.data_only) {   // x / l -> K_zx -> the conditional: dX = s o (E^T Zs - cs o Xs)
    if (dXin) {
      hipLaunchKernelGGL(scale_rows_kernel, dim3(blocks_for((long)rows * D)), dim3(256), 0, ctx->stream, dXs, rows, (long)rows, D, L.in_scale, dXin);
      LAUNCH_CHECK(ctx);
    }
    return DCGP_OK;
  }
  hipLaunchKernelGGL(ard_finish_kernel, dim3(D), dim3(256), 0, ctx->stream, dZs, Zs, M, dXs, Xs, (long)rows, D, L.in_scale, L.gZ, dXin, L.gard);
  LAUNCH_CHECK(ctx);
  DCGP_TRY(end_layer(bk, L));
  // the scalar "lengthscale" slot collected d / d(unit lengthscale): meaningless here, and L.ls must stay 1
  HIP_TRY(ctx, hipMemsetAsync(L.gscal + 1, 0, sizeof(double), ctx->stream));
  return DCGP_OK;
}

// SVGP head backward (ConvKernel / AdditivePatchKernel, conv_gp/kernels.py:15-136).  gm / gv [rows][R].
int head_backward(Bk& bk, LayerState& L, const double* Xin, int rows, int n_mod, const double* gm, const double* gv, double* dXin) {
  dcgp_ctx* ctx = bk.ctx;
  const int M = L.M, Mp = L.Mp, P = L.v.P, Ld = L.v.L;
  const long ld = col_ld(rows), Kc = (long)rows * P, ldf = col_ld(Kc);
  if (L.in_scale) return dense_head_backward(bk, L, Xin, rows, n_mod, gm, gv, dXin);
  DCGP_TRY(begin_layer(bk, L));
  const double* Kzx = forward_left(bk, "Kzx", 0, "K_zx for the head");
  if (!Kzx) return DCGP_ERR_ARG;
  double* A1 = bk.ws("A1h", (size_t)Mp * ld);
  double* dKzx = bk.ws("dKzx", (size_t)Mp * ld);
  double* S = bk.ws("S", (size_t)Mp * Mp);
  double* gkd = bk.ws("gkd", rows);
  double* Kfull = bk.ws("Kfull", (size_t)Mp * ldf);
  double* E = bk.ws("E", (size_t)Mp * ldf);
  double* cs = bk.ws("cs", Kc);
  double* raw = bk.ws("raw", Kc);
  double* Xcol = bk.ws("Xcol", (size_t)Kc * Ld);
  double* dXcol = bk.ws("dXcol", (size_t)Kc * Ld);
  NEED(A1); NEED(dKzx); NEED(S); NEED(gkd); NEED(Kfull); NEED(E); NEED(cs); NEED(raw); NEED(Xcol); NEED(dXcol);
  if (Mp > M) HIP_TRY(ctx, hipMemsetAsync(A1 + (size_t)M * ld, 0, (size_t)(Mp - M) * ld * sizeof(double), ctx->stream));   // padded rows: operands of gemm_tn
  // A1 = inv(L) Kzx: left behind by the forward pass's one-launch conditional in a training step (head_forward, keep_k), formed here otherwise
  if (L.a1h_ready) L.a1h_ready = false;
  else DCGP_TRY(gemm_gen(ctx, mk(L.g.Linv, Mp, 1, Kzx, ld, 1, A1, ld, M, rows, M)));
  Lanes ln = lanes_of(ctx);
  if (bk.data_only) { ln.forked = false; ln.chain = ln.tail = ln.main; }
  // as in conv_backward: the conditional's column-wise adjoint and the patch-kernel adjoints (K_zx, K_diag) on the main stream, the M x M
  // chain and what needs S beside them
  DCGP_TRY(cond_backward_main(bk, ln, L, A1, ld, rows, gm, gv, dKzx, gkd, bk.last_layer && ln.forked));
  // every patch response, Kfull[m][n * P + p] = k(Z_m, x_np): kept by the forward pass's sweep where that was the unit sweep (head_forward,
  // keep_k), evaluated again otherwise
  if (L.kfull_ready) {
    L.kfull_ready = false;
  } else {
    PatchRbfArgs a;
    a.X = Xin; a.N = rows; a.n_mod = n_mod;
    a.H = L.v.H; a.W = L.v.W; a.C = L.v.C; a.f = L.v.f; a.s = L.v.s; a.Ho = L.v.Ho; a.Wo = L.v.Wo; a.P = P; a.L = Ld;
    a.ZT = L.ZT; a.zn = L.zn; a.M = M; a.Mp = Mp; a.Lp = L.Lp;
    a.bk = L.base();
    a.out = Kfull; a.sM = ldf; a.sN = P; a.sP = 1;
    DCGP_TRY(patch_rbf(ctx, a, "grad_head_kfull"));
  }
  DCGP_TRY(im2col(ctx, L, Xin, n_mod, Kc, Xcol));
  // Kzx[m][n] = 1/P sum_p w_p k(Z_m, x_np)
  KufAdjoint ka;
  DCGP_TRY(kuf_adjoint(bk, L, dKzx, ld, P, L.w, 1.0 / P, Kfull, ldf, Xcol, Kc, E, ldf, cs, raw, &ka));
  if (!bk.data_only) {
    hipLaunchKernelGGL(strided_sum_kernel, dim3(P), dim3(256), 0, ctx->stream, raw, rows, P, 1.0 / P, 1, L.gw);
    LAUNCH_CHECK(ctx);
  }
  // (the input gradient's pass, see conv_backward: the K_zx part of dX comes from the fused launch below, ConvKernel's K_diag part rides in as `extra`)
  const bool fuse_dx = bk.data_only && dXin && patch_adjoint_fused_ok(L, rows);
  DCGP_TRY(patch_backward(bk, L, E, ldf, Kc, cs, Xcol, dXin && !fuse_dx ? dXcol : nullptr, 0, nullptr, nullptr, ka.rs, ka.cz, &ln));
  // Kdiag
  if (L.kernel_type == 0) {
    const double inv_l2 = 1.0 / (L.ls * L.ls);
    double* Gm = bk.ws("kd_G", (size_t)rows * P * P);
    double* norms = bk.ws("kd_norms", (size_t)rows * P);
    double* dwn = bk.ws("kd_dwn", (size_t)rows * P);
    double* pv = bk.ws("kd_pv", (size_t)rows * P);
    double* pl = bk.ws("kd_pl", (size_t)rows * P);
    NEED(Gm); NEED(norms); NEED(dwn); NEED(pv); NEED(pl);
    GenGemm gg = mk(Xcol, Ld, 1, Xcol, 1, Ld, Gm, P, P, P, Ld);     // per image: X_n X_n^T
    gg.batch = rows; gg.a_bs = (long)P * Ld; gg.b_bs = (long)P * Ld; gg.c_bs = (long)P * P;
    DCGP_TRY(gemm_gen(ctx, gg));
    hipLaunchKernelGGL(kdiag_norms_kernel, dim3(blocks_for((long)rows * P)), dim3(256), 0, ctx->stream, Gm, P, (long)rows, norms);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(kdiag_backward_kernel, dim3((P + 3) / 4, rows), dim3(256), 0, ctx->stream, Gm, norms, gkd, L.w, P, L.variance, inv_l2, dwn, pv, pl);
    LAUNCH_CHECK(ctx);
    DCGP_TRY(add_scalars(bk, L, {{0, pv, (long)rows * P, 1.0 / L.variance}, {1, pl, (long)rows * P, inv_l2 / L.ls}}));
    if (!bk.data_only) {
      hipLaunchKernelGGL(strided_sum_kernel, dim3(P), dim3(256), 0, ctx->stream, dwn, rows, P, 1.0, 1, L.gw);
      LAUNCH_CHECK(ctx);
    }
    if (dXin) {
      // d x_p += 2 (E_n X_n - rowsum(E_n) o X_n)_p / l^2   (E symmetric), per image
      GenGemm ge = mk(Gm, P, 1, Xcol, Ld, 1, dXcol, Ld, P, Ld, P);
      ge.batch = rows; ge.a_bs = (long)P * P; ge.b_bs = (long)P * Ld; ge.c_bs = (long)P * Ld;
      ge.alpha = 2.0 * inv_l2; ge.accumulate = fuse_dx ? 0 : 1; ge.sub_v = pv; ge.sv_bs = P; ge.sub_x = Xcol; ge.sx_rs = Ld; ge.sx_bs = (long)P * Ld;
      DCGP_TRY(gemm_gen(ctx, ge));
    }
  } else if (!bk.data_only) {   // (no x in it: nothing for the data path)
    // AdditivePatchKernel.Kdiag = mean_p w_p variance (conv_gp/kernels.py:53-61)
    double* tmp = bk.ws("kd_tmp", 2);
    NEED(tmp);
    DCGP_TRY(reduce_sum(ctx, gkd, rows, 1.0, tmp));                  // sum_n gkd
    DCGP_TRY(reduce_sum(ctx, L.w, P, 1.0 / P, tmp + 1));             // mean(w)
    hipLaunchKernelGGL(additive_kdiag_backward_kernel, dim3(blocks_for(P)), dim3(256), 0, ctx->stream, tmp, P, L.variance, L.gw,
                       L.gslots + VAR_SLOT + bk.slot_v);
    LAUNCH_CHECK(ctx);
    ++bk.slot_v;
  }
  if (dXin) DCGP_TRY(patches_to_dx(bk, L, fuse_dx, E, ldf, cs, Xin, rows, n_mod, L.kernel_type == 0 ? dXcol : nullptr, dXcol, dXin));
  if (bk.data_only) return DCGP_OK;
  // the main stream's part of the head ends here (dX is out): it goes on to the layer below (see conv_backward)
  if (ln.forked) HIP_TRY(ctx, hipEventRecord(ctx->ev_g[3], ctx->stream));
  DCGP_TRY(cond_backward_finish(bk, ln, L, A1, ld, rows, dKzx, S, bk.kl_early && !L.white, bk.last_layer && ln.forked));
  return layer_tail(bk, ln, L, S, nullptr, 0, false);
}

}  // namespace

static double kl_weight(const dcgp_model* m) {
  // the data term is summed over the batch shards (ranks); the KL term is replicated, so each shard carries 1 / shards of it
  const int shards = m->grad_shards > 0 ? m->grad_shards : (m->ctx->comm ? m->ctx->nranks : 1);
  return 1.0 / shards;
}

// Called by the forward pass of a training step (forward_all, model.hip): the KL adjoint's products of every unwhitened layer go to the
// side stream, beside the layers of the forward pass (see model_state.h for the two calls).
int grad_kl_early(dcgp_model* m, bool enqueue, bool wait_fork) {
  dcgp_ctx* ctx = m->ctx;
  const int nl = (int)m->layers.size();
  for (bool& f : m->kl_early) f = false;
  for (int& f : m->prep_early) f = 0;
  const bool side = !ctx->opt.grad_nofork && !ctx->no_side && ctx->stream2 && ctx->stream_aux;
  if (ctx->opt.grad_late_kl || !side || nl > 8) return DCGP_OK;
  if (!enqueue) return 1;
  Bk bk;
  bk.m = m; bk.ctx = ctx; bk.klw = kl_weight(m);
  hipStream_t saved = ctx->stream;
  // a stream of its own: on the side stream these ~40 launches (slow beside the forward pass's kernels) were still in front of the head's side
  // chain when the reverse pass got there
  hipStream_t es = ctx->stream_aux;
  if (wait_fork) {
    HIP_TRY(ctx, hipStreamWaitEvent(es, ctx->ev_fork, 0));
    // (the mark may sit on the main stream behind layer 0 while G / alpha of the later layers are still being written on the chain's stream)
    for (int li = 0; li < m->gkl_prep_wait && li < nl; ++li) HIP_TRY(ctx, hipStreamWaitEvent(es, m->ev_prep[m->bank][li], 0));
  }
  ctx->stream = es;
  const std::string mp = "m" + std::to_string(m->id) + "_";
  int rc = DCGP_OK;
  // first what the main stream's part of the reverse pass reads: zero fills and the parameter-only operands of every layer's conditional
  // (model_backward waits for ctx->ev_kl2 -- long past by then), the last layer first
  for (int li = nl - 1; li >= 0 && rc == DCGP_OK; --li) {
    LayerState& L = *m->layers[li];
    bk.pfx = mp + std::to_string(li) + "_";
    rc = layer_fills(bk, L);
    if (rc == DCGP_OK) rc = param_operands(bk, L, false);
    if (rc == DCGP_OK) m->prep_early[li] = 1;
    ConvBwdArgs fb;
    fb.M = L.M; fb.Mp = L.Mp; fb.R = L.R;
    if (rc == DCGP_OK && !L.is_head && L.has_qsqrt && !L.white && conv_bwd_fused_ok(ctx, fb)) {
      rc = param_operands(bk, L, true);
      if (rc == DCGP_OK) m->prep_early[li] |= 2;
    }
  }
  if (rc == DCGP_OK && hipEventRecord(ctx->ev_kl2, es) != hipSuccess) rc = DCGP_ERR_HIP;
  for (int li = 0; li < nl && rc == DCGP_OK; ++li) {
    LayerState& L = *m->layers[li];
    if (L.white) continue;
    bk.pfx = mp + std::to_string(li) + "_";
    double* Sacc = nullptr;
    if (L.is_head) {   // the head's prior shares the live Z: its part of d ELBO / dKuu opens the buffer cond_backward adds to
      Sacc = bk.ws("S", (size_t)L.Mp * L.Mp);
      if (!Sacc) { rc = DCGP_ERR_ALLOC; break; }
    }
    rc = kl_products(bk, L, Sacc, true);
    if (rc == DCGP_OK) m->kl_early[li] = true;
  }
  if (rc == DCGP_OK && hipEventRecord(ctx->ev_kl3, es) != hipSuccess) rc = DCGP_ERR_HIP;
  ctx->stream = saved;
  if (rc != DCGP_OK) { hipStreamSynchronize(es); for (bool& f : m->kl_early) f = false; for (int& f : m->prep_early) f = 0; }
  return rc;
}

// out[i] = sum_s in[s * n + i]: layer 0 saw the batch tiled S times, the S replicas' dX add up (in the order s = 0, 1, ...)
namespace {
__global__ void reduce_replicas1_kernel(const double* __restrict__ a, int S, long n, double* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int r = 0; r < S; ++r) s += a[(long)r * n + i];
  out[i] = s;
}
}  // namespace

// RobustMax seeds of the variational expectation: gm, gv [rows][K] = weight * d E_q[log p(y | f)] / d(mean, var), row r with label y[r % n_labels]
int robustmax_grad(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int rows, int n_labels, int K, double eps, double weight,
                   double* gm, double* gv) {
  if (K > RM_KMAX) return ctx_fail(ctx, DCGP_ERR_ARG, "grad: at most %d classes", RM_KMAX);
  const double* gh = gauss_hermite_table(ctx);
  if (!gh) return DCGP_ERR_ALLOC;
  ScopedTimer tm(ctx, "robustmax_grad");
  hipLaunchKernelGGL(robustmax_grad_kernel, dim3((rows + RM_ROWS - 1) / RM_ROWS), dim3(256), 0, ctx->stream, mu, var, y, rows, n_labels, K, eps, gh, weight,
                     gm, gv);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// The reverse walk over the layers, from the head's (gm, gv) [rows][R] down to layer 0, on what a forward pass with keep_outputs / keep_state left.
// bk.data_only (the input gradient): the data path alone, down to and INCLUDING layer 0's dX, which -- summed over the S replicas of a tiled batch --
// goes to out_dX [N][H W C]; nothing but workspaces is written.  Otherwise (a training step, out_dX == nullptr): every layer's gradient block, layer
// 0 produces no dX, and what grad_kl_early enqueued beside the forward pass is consumed per layer.
static int backward_walk(Bk& bk, const double* X, int N, int S, int dedup_layer0, double* gm, double* gv, double* out_dX, const char* who) {
  dcgp_model* m = bk.m;
  dcgp_ctx* ctx = bk.ctx;
  const int nl = (int)m->layers.size();
  if (!m->keep_outputs) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: the forward pass must keep the layer outputs", who);
  for (auto& l : m->layers) {
    if (l->base_type != 0 && l->is_head) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: the head kernels are RBF-based", who);
  }
  const std::string mp = "m" + std::to_string(m->id) + "_";
  bool dedup_done = false;   // layer 0's (dmean, dvar) already summed over the S replicas
  for (int li = nl - 1; li >= 0; --li) {
    LayerState& L = *m->layers[li];
    bk.pfx = mp + std::to_string(li) + "_";
    bk.last_layer = li == 0;
    if (!bk.data_only && li < 8) {
      bk.kl_early = m->kl_early[li]; bk.prep = m->prep_early[li];
      m->kl_early[li] = false; m->prep_early[li] = 0;
    }
    const int pad = li < 8 ? m->pad[li] : 0;   // a padded layer read the padded copy its forward left (model.hip: pad_input); its dX has that size
    // a dilated layer (dcgp_model_set_dilation) ran on the d^2 phase sub-images of its (padded) input, which its forward left (model.hip: split_input);
    // its (gm, gv) arrive in phase layout (below, where they are formed) and its dX comes out in phase layout
    const int dil = L.is_head ? 1 : m->dil_of(li), dd = dil * dil;
    const dcgp_model::Geom geo = m->geom(li);   // the true (padded) input size
    const double* Xin = dil > 1 ? m->dil_in[li] : (pad > 0 ? m->pad_in[li] : (li == 0 ? X : m->outs[li - 1].sample));
    if (!Xin) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: layer %d has no %s input from the forward pass", who, li, dil > 1 ? "split" : "padded");
    int rows_l = m->outs[li].rows;                  // rows entering == rows leaving ...
    // ... except for a de-duplicated first conv layer: propagate() tiles the batch S times, so layer 0 saw S identical
    // copies; the forward evaluated its conditional on the N distinct images and drew S samples from it.  The S
    // gradients arriving per image add up, and the conditional's reverse pass runs on N rows instead of S N (exact).
    if (li == 0 && dedup_layer0 && !L.is_head && rows_l == S * N && S > 1) {
      if (!dedup_done) {   // (the head-less case: the gradients came from the likelihood, not from a layer above)
        if (dil > 1) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: a dilated layer takes its gradient from the layer above it", who);
        const long n = (long)N * L.v.P * L.R;
        double* gm0 = (double*)ws_get(ctx, bk.pfx + "g_gm_dedup", (size_t)n * sizeof(double));
        double* gv0 = (double*)ws_get(ctx, bk.pfx + "g_gv_dedup", (size_t)n * sizeof(double));
        NEED(gm0); NEED(gv0);
        hipLaunchKernelGGL(reduce_replicas_kernel, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, gm, gv, S, n, gm0, gv0);
        LAUNCH_CHECK(ctx);
        gm = gm0; gv = gv0;
      }
      rows_l = N;
    }
    if (!L.is_head && L.mix_W && li == nl - 1) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: a mixed layer must have a layer above it", who);
    const int n_mod = li == 0 ? N : rows_l;
    const long img = (long)L.v.H * L.v.W * L.v.C;   // (one sub-image of a dilated layer)
    double* dXin = li == 0 ? out_dX : nullptr;   // (layer 0 of a training step: no dX)
    if (li > 0 || (out_dX && (rows_l != N || pad > 0 || dil > 1))) {
      dXin = (double*)ws_get(ctx, bk.pfx + "g_dXin", (size_t)rows_l * dd * img * sizeof(double));
      NEED(dXin);
    }
    if (L.is_head) DCGP_TRY(head_backward(bk, L, Xin, rows_l, n_mod, gm, gv, dXin));
    else DCGP_TRY(conv_backward(bk, L, Xin, rows_l * dd, n_mod * dd, gm, gv, dXin));
    if (li == 0 && out_dX && rows_l % N) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: %d rows at layer 0 for %d images", who, rows_l, N);
    if (dil > 1 && dXin) {   // back to image layout; layer 0's replica sum in the same pass where no crop follows (the crop sums otherwise)
      const bool last_pass = li == 0 && pad == 0;
      double* dimg = last_pass ? out_dX : (double*)ws_get(ctx, bk.pfx + "g_dXb2s", (size_t)rows_l * geo.H * geo.W * L.v.C * sizeof(double));
      NEED(dimg);
      if (last_pass) DCGP_TRY(b2s_images(ctx, ctx->stream, dXin, rows_l / N, N, geo.H, geo.W, L.v.C, dil, dimg));
      else DCGP_TRY(b2s_images(ctx, ctx->stream, dXin, 1, rows_l, geo.H, geo.W, L.v.C, dil, dimg));
      dXin = dimg;
    }
    if (li == 0) {
      if (out_dX && pad > 0) {       // crop to the caller's geometry, the replica sum in the same pass
        DCGP_TRY(crop_images(ctx, ctx->stream, dXin, rows_l / N, N, geo.H - 2 * pad, geo.W - 2 * pad, L.v.C, pad, out_dX));
      } else if (out_dX && rows_l != N && dil == 1) {   // the final replica sum (a dilated layer's: in its batch-to-space pass above)
        hipLaunchKernelGGL(reduce_replicas1_kernel, dim3(blocks_for(N * img)), dim3(256), 0, ctx->stream, dXin, rows_l / N, N * img, out_dX);
        LAUNCH_CHECK(ctx);
      }
      break;
    }
    auto& o = m->outs[li - 1];
    LayerState& Lb = *m->layers[li - 1];
    // a dilated layer below: its (d mean, d var) are formed in PHASE layout, phantoms included -- the gradient from above is split first (a phantom's
    // is an exact zero), the triple is the phase-layout one its forward left (a mixed layer's latent triple is in phase layout as it is)
    const int dil_b = Lb.is_head ? 1 : m->dil_of(li - 1), dd_b = dil_b * dil_b;
    const long rows_b = (long)o.rows * dd_b;   // rows of the layer below as its kernels count them
    const long n_out = dil_b > 1 ? rows_b * Lb.v.P * Lb.Rout : (long)o.rows * o.width;
    const long n = Lb.is_head ? n_out : rows_b * Lb.v.P * Lb.R;   // the (d mean, d var) the layer below takes: its GPs' (== n_out unless it is mixed)
    gm = (double*)ws_get(ctx, mp + std::to_string(li - 1) + "_g_gm", (size_t)n * sizeof(double));
    gv = (double*)ws_get(ctx, mp + std::to_string(li - 1) + "_g_gv", (size_t)n * sizeof(double));
    NEED(gm); NEED(gv);
    if (pad > 0) {   // the sample's gradient is the interior of the padded input's
      double* dcrop = (double*)ws_get(ctx, bk.pfx + "g_dXcrop", (size_t)n_out * sizeof(double));
      NEED(dcrop);
      DCGP_TRY(crop_images(ctx, ctx->stream, dXin, 1, o.rows, geo.H - 2 * pad, geo.W - 2 * pad, L.v.C, pad, dcrop));
      dXin = dcrop;
    }
    const bool dedup_below = li - 1 == 0 && dedup_layer0 && !Lb.is_head && o.rows == S * N && S > 1;
    const double *smp = o.sample, *mean = o.mean, *var = o.var;
    if (dil_b > 1) {
      const dcgp_model::Geom gb = m->geom(li - 1);
      const auto& ph = m->dil_out[li - 1];
      if (!ph.sample || !ph.mean || !ph.var) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: layer %d has no phase-layout outputs from the forward pass", who, li - 1);
      double* dsplit = (double*)ws_get(ctx, bk.pfx + "g_dXs2b", (size_t)n_out * sizeof(double));
      NEED(dsplit);
      DCGP_TRY(s2b_images(ctx, ctx->stream, dXin, o.rows, gb.Ho, gb.Wo, Lb.Rout, dil_b, dsplit));
      dXin = dsplit;
      smp = ph.sample; mean = ph.mean; var = ph.var;
    }
    const double* dF = dXin;
    bk.mix_gF = bk.mix_gF_all = nullptr; bk.mix_cols = 0;
    if (!Lb.is_head && Lb.mix_W) {   // a mixed layer (mix.hip): gu = gF W^T on every replica's columns, then the sample's adjoint on its latent triple
      const long cols = rows_b * Lb.v.P;
      double* gu = (double*)ws_get(ctx, mp + std::to_string(li - 1) + "_g_gu", (size_t)n * sizeof(double));
      NEED(gu);
      DCGP_TRY(mix_backward_latent(ctx, Lb.mix_W, Lb.R, Lb.Rout, dXin, cols, gu));
      bk.mix_gF_all = dXin; bk.mix_cols = cols; bk.mix_gF = dXin;
      if (dedup_below && Lb.mean_W) {   // the mean filter sees the N distinct images: its adjoint takes the replicas' sum
        const long n0 = n_out / S;
        double* gF0 = (double*)ws_get(ctx, mp + std::to_string(li - 1) + "_g_gF0", (size_t)n0 * sizeof(double));
        NEED(gF0);
        hipLaunchKernelGGL(reduce_replicas1_kernel, dim3(blocks_for(n0)), dim3(256), 0, ctx->stream, dXin, S, n0, gF0);
        LAUNCH_CHECK(ctx);
        bk.mix_gF = gF0;
      }
      dF = gu; smp = Lb.lat_sample; mean = Lb.lat_mean; var = Lb.lat_var;
    }
    if (dedup_below) {   // S gradients per element of the shared conditional: summed here
      const long n0 = n / S;
      hipLaunchKernelGGL(sample_backward_dedup_kernel, dim3(blocks_for(n0)), dim3(256), 0, ctx->stream, dF, smp, mean, var, m->jitter, S, n0, gm, gv);
      dedup_done = true;
    } else {
      hipLaunchKernelGGL(sample_backward_kernel, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, dF, smp, mean, var, m->jitter, n, gm, gv);
    }
    LAUNCH_CHECK(ctx);
  }
  return DCGP_OK;
}

int model_backward(dcgp_model* m, const Targets& targets, const double* X, int N, double scale, int dedup_layer0) {
  dcgp_ctx* ctx = m->ctx;
  const int nl = (int)m->layers.size(), S = m->S;
  bool prepped = false;
  for (int f : m->prep_early) prepped = prepped || f != 0;
  if (prepped) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_kl2, 0));   // fills and parameter-only operands from the side stream (grad_kl_early)
  Bk bk;
  bk.m = m; bk.ctx = ctx;
  bk.klw = kl_weight(m);
  const std::string mp = "m" + std::to_string(m->id) + "_";
  LayerState& H = *m->layers[nl - 1];
  auto& oh = m->outs[nl - 1];
  const int rows = oh.rows;
  const double weight = scale * ((rows == S * N) ? 1.0 / S : 1.0);
  const Likelihood lik = m->lik();
  double* gm = (double*)ws_get(ctx, mp + "g_gm_head", (size_t)rows * H.R * sizeof(double));
  double* gv = (double*)ws_get(ctx, mp + "g_gv_head", (size_t)rows * H.R * sizeof(double));
  NEED(gm); NEED(gv);
  double* gs2 = nullptr;   // Gaussian likelihood: d / d variance (StudentT: d / d scale), moved into the head's block (glik) once its zero fill is behind us
  if (lik.n_params()) { gs2 = (double*)ws_get(ctx, mp + "g_lik", sizeof(double)); NEED(gs2); }
  DCGP_TRY(lik_grad_seeds(ctx, lik, oh.mean, oh.var, targets, rows, N, H.R, weight, gm, gv, gs2));
  DCGP_TRY(backward_walk(bk, X, N, S, dedup_layer0, gm, gv, nullptr, "grad"));
  if (bk.side_pending) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_kl, 0));   // the one join of the step: every layer's side-stream tail
  if (gs2) HIP_TRY(ctx, hipMemcpyAsync(H.glik, gs2, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));   // (behind every fill of the block)
  m->grad_scattered = false;
  if (ctx->comm) {
    // One in-stream collective per layer over its contiguous gradient block (RCCL over xGMI).  A training step in exchange mode 1: a
    // reduce-scatter -- this rank's shard of the block summed over the ranks, 1 / ranks of an all-reduce's receive volume -- followed (opt_enqueue)
    // by the update of that shard alone and an all-gather of the parameters; otherwise the all-reduce every rank follows with the full update.
    const bool scatter = m->grad_exchange == 1 && m->adam_follows && ctx->nranks > 1;
    for (auto& l : m->layers) {
      const size_t n = l->grad_block_count();
      if (n > 0x7fffffffUL) return ctx_fail(ctx, DCGP_ERR_ARG, "grad: gradient block too large for one collective");
      if (scatter) {
        long lo, hi, sh;
        DCGP_TRY(dcgp_shard_range((long)n, ctx->nranks, ctx->rank, &lo, &hi, &sh));
        if ((size_t)sh * ctx->nranks > n + LayerState::kGradBlockPad) return ctx_fail(ctx, DCGP_ERR_ARG, "grad: more ranks than the gradient block is padded for");
        DCGP_TRY(reduce_scatter_sum_f64_async(ctx, l->gZ, (size_t)sh));
      } else {
        DCGP_TRY(allreduce_sum_f64_async(ctx, l->gZ, (int)n));
      }
    }
    m->grad_scattered = scatter;
  }
  return DCGP_OK;
}

// the input gradient's reverse pass (input_grad.hip): the walk's data path alone, no gradient block is touched
int model_backward_data(dcgp_model* m, const double* X, int N, int S, int dedup_layer0, double* gm, double* gv, double* out_dX) {
  Bk bk;
  bk.m = m; bk.ctx = m->ctx; bk.data_only = true;
  return backward_walk(bk, X, N, S, dedup_layer0, gm, gv, out_dX, "input_grad");
}

// Adam step enqueued behind the reverse pass (dcgp_model_train_step_adam): lr is the bias-corrected rate
struct AdamReq { double lr_t, beta1, beta2, eps; };

static int elbo_grad_run(dcgp_model* model, const double* X, const int32_t* y, int N, double scale, const double* const* z_per_layer_host,
                         uint64_t seed, int dedup_layer0, double* out_host, int* info_host, const AdamReq* adam, const double* yf = nullptr) {
  dcgp_ctx* ctx = model->ctx;
  const bool keep = model->keep_outputs;
  model->keep_outputs = true;   // the reverse pass reads every layer's (sample, mean, var)
  model->keep_state = true;     // ... and K_uf / A1 of every conv layer
  model->adam_follows = adam != nullptr;
  model->grad_follows = true;   // ... and marks where the parameter-only part of the reverse pass may start (grad_kl_early)
  // The forward pass is ENQUEUED, the reverse pass behind it, and only then is the forward's result collected: the host does not wait for
  // the ELBO before it feeds the ~110 launches of the reverse pass (a failed factorisation is reported all the same; the reverse pass then
  // ran on NaNs, which nothing reads).
  uint64_t ticket = 0;
  if (info_host) *info_host = 0;
  const auto host_t0 = std::chrono::steady_clock::now();
  int rc = model->enq_seq != model->col_seq ? ctx_fail(ctx, DCGP_ERR_ARG, "elbo_grad: enqueued steps are still to be collected")
                                             : elbo_forward_enqueue_impl(model, X, y, N, scale, z_per_layer_host, seed, dedup_layer0, &ticket, false, yf);
  const bool enqueued = rc == DCGP_OK;
  if (rc == DCGP_OK && model->gkl_state) rc = grad_kl_early(model, true, model->gkl_state == 2);
  if (rc == DCGP_OK) rc = model_backward(model, Targets::of(y, yf, model->layers.back()->R), X, N, scale, dedup_layer0);
  // (the update reads the step's factorisation status word on the device: a failed step leaves the parameters as they were)
  if (rc == DCGP_OK && adam)
    rc = opt_enqueue(model, "train_step_adam", false, adam->lr_t, adam->beta1, adam->beta2, adam->eps, model->d_scal + 64 * model->bank + 43, 0);
  if (ctx->timing) {   // host time to enqueue the whole step, forward pass included (reported beside the kernel timers)
    auto& acc = ctx->tim["grad_host_enqueue"];
    acc.launches += 1;
    acc.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count();
  }
  if (enqueued) {
    const int rc_f = elbo_forward_collect_impl(model, ticket, out_host, info_host);
    if (rc == DCGP_OK) rc = rc_f;
  }
  model->keep_outputs = keep;
  model->keep_state = false;
  model->grad_follows = false;
  model->gkl_state = 0;
  if (rc != DCGP_OK) {
    model->norm_pending = false;   // (a failed step records no norm)
    for (bool& f : model->kl_early) f = false;
    for (int& f : model->prep_early) f = 0;
    hipStreamSynchronize(ctx->stream);
    if (ctx->stream2) hipStreamSynchronize(ctx->stream2);
    if (ctx->stream_aux) hipStreamSynchronize(ctx->stream_aux);
  }
  DCGP_TRY(rc);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (adam) DCGP_TRY(opt_readback(model));
  return DCGP_OK;
}

extern "C" {

int dcgp_elbo_grad(dcgp_model* model, const double* X, const int32_t* y, int N, double scale, const double* const* z_per_layer_host,
                   uint64_t seed, int dedup_layer0, double* out_host, int* info_host) {
  if (!model || !X || !y || N <= 0 || !out_host) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "elbo_grad: bad args") : DCGP_ERR_ARG;
  return elbo_grad_run(model, X, y, N, scale, z_per_layer_host, seed, dedup_layer0, out_host, info_host, nullptr);
}

int dcgp_elbo_grad_f64y(dcgp_model* model, const double* X, const double* y, int N, double scale, const double* const* z_per_layer_host,
                        uint64_t seed, int dedup_layer0, double* out_host, int* info_host) {
  if (!model || !X || !y || N <= 0 || !out_host) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "elbo_grad_f64y: bad args") : DCGP_ERR_ARG;
  return elbo_grad_run(model, X, nullptr, N, scale, z_per_layer_host, seed, dedup_layer0, out_host, info_host, nullptr, y);
}

int dcgp_model_train_step_adam_f64y(dcgp_model* model, const double* X, const double* y, int N, double scale, const double* const* z_per_layer_host,
                                    uint64_t seed, int dedup_layer0, double lr, double beta1, double beta2, double eps, int t, double* out_host,
                                    int* info_host) {
  if (!model || !X || !y || N <= 0 || !out_host) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "train_step_adam_f64y: bad args") : DCGP_ERR_ARG;
  model->grad_norms.clear();   // (a run clears once, in front of its first step)
  return train_step_adam_run(model, X, nullptr, N, scale, z_per_layer_host, seed, dedup_layer0, lr, beta1, beta2, eps, t, out_host, info_host, y);
}

int dcgp_model_train_step_adam(dcgp_model* model, const double* X, const int32_t* y, int N, double scale, const double* const* z_per_layer_host,
                               uint64_t seed, int dedup_layer0, double lr, double beta1, double beta2, double eps, int t, double* out_host,
                               int* info_host) {
  if (!model || !X || !y || N <= 0 || !out_host) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "train_step_adam: bad args") : DCGP_ERR_ARG;
  model->grad_norms.clear();   // (a run clears once, in front of its first step)
  return train_step_adam_run(model, X, y, N, scale, z_per_layer_host, seed, dedup_layer0, lr, beta1, beta2, eps, t, out_host, info_host, nullptr);
}

}  // extern "C"

// One training step in one call: value, gradient and the Adam update (dcgp_model_adam_step's arguments; t == 0: the model's own step
// count), enqueued back to back with one wait at the end -- what session.run(minimise_op) is to the reference (conv_gp/experiment.py:84-108).
// A step whose factorisation fails returns DCGP_ERR_NOT_PD and leaves parameters, moments and step count untouched.
// (also the step of dcgp_model_train_run_adam, train_run.hip)
int train_step_adam_run(dcgp_model* model, const double* X, const int32_t* y, int N, double scale, const double* const* z_per_layer_host,
                        uint64_t seed, int dedup_layer0, double lr, double beta1, double beta2, double eps, int t, double* out_host,
                        int* info_host, const double* yf) {
  if (t < 0 || !(lr > 0) || !(beta1 >= 0 && beta1 < 1) || !(beta2 >= 0 && beta2 < 1) || !(eps > 0))
    return ctx_fail(model->ctx, DCGP_ERR_ARG, "train_step_adam: bad optimiser arguments");
  const int t_use = t == 0 ? model->adam_t + 1 : t;
  AdamReq a;
  a.lr_t = lr * sqrt(1.0 - pow(beta2, (double)t_use)) / (1.0 - pow(beta1, (double)t_use));
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
  for (auto& l : model->layers) DCGP_TRY(l->ensure_grads());   // (the optimiser's group table is built before the first reverse pass has run)
  DCGP_TRY(elbo_grad_run(model, X, y, N, scale, z_per_layer_host, seed, dedup_layer0, out_host, info_host, &a, yf));
  model->adam_t = t_use;
  return DCGP_OK;
}

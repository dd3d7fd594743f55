// bernoulli.hip -- the Bernoulli likelihood's tails (gpflow 1.x likelihoods.Bernoulli(invlink=probit) under doubly_stochastic_dgp's
// BroadcastingLikelihood): every output an independent binary label, targets y [N][D] float64, y == 1.0 positive, anything else negative
// (gpflow's logdensities.bernoulli: tf.equal(x, 1)).
//
//   p(f) = Phi(f) (1 - 2e-3) + 1e-3                              (gpflow's jittered probit: every log finite)
//   logp(f, y) = log p(f) if y == 1 else log(1 - p(f))
//   variational expectation per (row, d):  sum_i w_i / sqrt(pi) logp(mu + sqrt(2 v) x_i, y)     (ndiagquad, 20 Gauss-Hermite nodes)
//   predictive mean per (row, d):          p = probit(mu / sqrt(1 + v)), variance p - p^2
//   predictive density per (image, d):     logsumexp_s logp(y; p_s) - log S
//
// The reverse tail differentiates the 20-node sum as written (through sqrt(2 v), clamped as robustmax_node clamps it), as TF autodiff
// of gpflow does: not the E[g''] / 2 identity, which differs at finite order.  Sums run in a fixed order (index order per thread, a tree
// per workgroup, the last workgroup to arrive over the rows): results are bitwise reproducible, no float atomics.  One thread per
// element (forward, reverse, predictions) or image (evaluation): at cfg2 sizes these tails are latency-bound.
#include "layer_impl.h"
#include "tail_dev.h"

namespace {

constexpr double kInvSqrt2 = 0.70710678118654752440, kInvSqrtPi = 0.56418958354775628695, kInvSqrt2Pi = 0.39894228040143267794;

__device__ __forceinline__ double probit(double x) { return 0.5 * (1.0 + erf(x * kInvSqrt2)) * (1.0 - 2e-3) + 1e-3; }
__device__ __forceinline__ double bern_logp(double p, bool pos) { return pos ? log(p) : log(1.0 - p); }

// sum_i w_i / sqrt(pi) logp(mu + s x_i, y), s = sqrt(max(2 v, 1e-10)); gh = {20 nodes, 20 weights}
__device__ __forceinline__ double bern_ve(double mu, double v, bool pos, const double* gh) {
  const double s = sqrt(fmax(2.0 * v, 1e-10));
  double acc = 0.0;
  for (int g = 0; g < 20; ++g) acc += gh[20 + g] * kInvSqrtPi * bern_logp(probit(mu + s * gh[g]), pos);
  return acc;
}

struct BernTailArgs {
  TailArgs t;                      // mu / var [n_rows][K], gh, ve [n_rows], inv_s, ticket, scal, fin (t.y, t.eps unused)
  const double* y = nullptr;       // [n_labels][K]: row r reads y[(r % n_labels) * K ..]
};

// ELBO tail: one thread per element.  A workgroup takes rows_per_block(K) = max(1, 256 / K) whole rows, thread e of it element
// (e / K, e % K) of its rows; each row's K expectations go through LDS and are summed in index order by the row's first thread.  Then the
// KlTail workgroups; the last workgroup to arrive sums the rows (per-thread strides, then a tree) and assembles the ELBO as elbo_tail_kernel
// does.  (One thread per row ran its K quadratures back to back: 92 us at K = 10 against 12 us for elbo_tail_kernel.)
__host__ __device__ constexpr int rows_per_block(int K) { return K >= 256 ? 1 : 256 / K; }
constexpr int kTailMaxK = 1024;   // (a row's K expectations in the kernel's 1024-double LDS)

__global__ __launch_bounds__(256) void bern_tail_kernel(BernTailArgs a, KlTail kl, int nb_rows) {
  __shared__ double red[4 * 256];
  __shared__ unsigned last;
  const TailArgs& t = a.t;
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= nb_rows) {
    const int l = blockIdx.x - nb_rows;
    kl_pieces_block(kl.l[l], t.scal + 4 + 4 * l, red);
  } else {
    const int rpb = rows_per_block(t.K), row0 = blockIdx.x * rpb;
    const int nrows = min(rpb, t.n_rows - row0);
    for (int e = tid; e < nrows * t.K; e += 256) {
      const int row = row0 + e / t.K, d = e % t.K;
      const double yd = a.y[(long)(row % t.n_labels) * t.K + d];
      red[e] = bern_ve(t.mu[(long)row * t.K + d], t.var[(long)row * t.K + d], yd == 1.0, t.gh);
    }
    __syncthreads();
    if (tid < nrows) {
      double s = 0.0;
      for (int d = 0; d < t.K; ++d) s += red[tid * t.K + d];
      t.ve[row0 + tid] = s;
    }
  }
  if (!last_to_arrive(t.ticket, gridDim.x, &last)) return;
  double s = 0.0;
  for (int i = tid; i < t.n_rows; i += 256) s += __hip_atomic_load(t.ve + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) elbo_assemble(t.scal, t.fin, red[0] * t.inv_s);
}

// Reverse tail: d (weight * ve) / d mu and / d v per element of [rows][K], one thread each.  With f_i = mu + s x_i:
//   d/dmu = sum_i c_i logp'(f_i),  d/dv = sum_i c_i logp'(f_i) x_i ds/dv,  ds/dv = 1 / s (0 where the clamp holds),
//   logp'(f) = Phi'(f) (1 - 2e-3) / p  (y == 1)  or  -Phi'(f) (1 - 2e-3) / (1 - p)  (otherwise),  c_i = w_i / sqrt(pi).
__global__ __launch_bounds__(256) void bern_grad_kernel(const double* __restrict__ mu, const double* __restrict__ var, const double* __restrict__ y,
                                                        long n, int K, int n_labels, const double* __restrict__ gh, double weight,
                                                        double* __restrict__ gm, double* __restrict__ gv) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long row = i / K;
  const int d = (int)(i - row * K);
  const bool pos = y[(row % n_labels) * K + d] == 1.0;
  const double m = mu[i], v = var[i];
  const bool live = 2.0 * v > 1e-10;
  const double s = sqrt(fmax(2.0 * v, 1e-10));
  double am = 0.0, av = 0.0;
  for (int g = 0; g < 20; ++g) {
    const double f = m + s * gh[g];
    const double p = probit(f);
    const double dp = exp(-0.5 * f * f) * kInvSqrt2Pi * (1.0 - 2e-3);
    const double q = gh[20 + g] * kInvSqrtPi * (pos ? dp / p : -dp / (1.0 - p));
    am += q;
    av += q * gh[g];
  }
  gm[i] = weight * am;
  gv[i] = live ? weight * av / s : 0.0;
}

// predict_y: (p, p - p^2), p = probit(mu / sqrt(1 + v))
__global__ void bern_predict_kernel(const double* __restrict__ mu, const double* __restrict__ var, long n, double* __restrict__ out_mean,
                                    double* __restrict__ out_var) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double p = probit(mu[i] / sqrt(1.0 + var[i]));
  if (out_mean) out_mean[i] = p;
  if (out_var) out_var[i] = p - p * p;
}

// Evaluation tail of one batch (head rows [S*n][K], row s*n + i): one thread per image, its K outputs in index order.  Per image at
// index lo + i of the whole set: the log density summed over the outputs (and per output where ld_nd is given), the sample-mean p
// (p_mean, may be nullptr) and the number of outputs whose label is 1 exactly where that mean is > 0.5 (as a double: gauss_eval_sum
// adds it up).
__global__ __launch_bounds__(256) void bern_eval_tail_kernel(const double* __restrict__ mu, const double* __restrict__ var, const double* __restrict__ y,
                                                             int n, int S, int K, long lo, double* __restrict__ logdens, double* __restrict__ ld_nd,
                                                             double* __restrict__ p_mean, double* __restrict__ correct) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long gi = lo + i;
  double ld = 0.0, ok = 0.0;
  for (int d = 0; d < K; ++d) {
    const bool pos = y[(long)i * K + d] == 1.0;
    double mx = -__builtin_inf(), psum = 0.0;
    for (int s = 0; s < S; ++s) {
      const long r = ((long)s * n + i) * K + d;
      const double p = probit(mu[r] / sqrt(1.0 + var[r]));
      mx = fmax(mx, bern_logp(p, pos));
      psum += p;
    }
    double acc = 0.0;
    for (int s = 0; s < S; ++s) {
      const long r = ((long)s * n + i) * K + d;
      acc += exp(bern_logp(probit(mu[r] / sqrt(1.0 + var[r])), pos) - mx);
    }
    const double l = mx + log(acc) - log((double)S);
    if (ld_nd) ld_nd[gi * K + d] = l;
    ld += l;
    const double pm = psum / (double)S;
    if (p_mean) p_mean[gi * K + d] = pm;
    if ((pm > 0.5) == pos) ok += 1.0;
  }
  logdens[gi] = ld;
  correct[gi] = ok;
}

}  // namespace

int bern_elbo_tail(dcgp_ctx* ctx, const double* mu, const double* var, const double* y, int n_rows, int n_labels, int K, double* ve_rows,
                   double inv_s, double* scal, const ElboFinish& fin, const KlTail* kl) {
  BernTailArgs a;
  DCGP_TRY(elbo_tail_prepare(ctx, &a.t));   // (Gauss-Hermite table; the same arrival counter as elbo_tail: the two never share a launch)
  a.t.mu = mu; a.t.var = var; a.t.n_rows = n_rows; a.t.n_labels = n_labels; a.t.K = K; a.t.ve = ve_rows;
  a.t.inv_s = inv_s; a.t.scal = scal; a.t.fin = fin;
  a.y = y;
  if (K < 1 || K > kTailMaxK) return ctx_fail(ctx, DCGP_ERR_ARG, "bernoulli: the head has %d outputs, the ELBO tail takes 1 to %d", K, kTailMaxK);
  const int rpb = rows_per_block(K), nb_rows = (n_rows + rpb - 1) / rpb;
  ScopedTimer tm(ctx, "bern_tail");
  KlTail k;
  if (kl) k = *kl;
  hipLaunchKernelGGL(bern_tail_kernel, dim3((unsigned)(nb_rows + k.nl)), dim3(256), 0, ctx->stream, a, k, nb_rows);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int bern_grad(dcgp_ctx* ctx, const double* mu, const double* var, const double* y, int rows, int K, int n_labels, double weight, double* gm,
              double* gv) {
  const double* gh = gauss_hermite_table(ctx);
  if (!gh) return DCGP_ERR_ALLOC;
  const long n = (long)rows * K;
  if (n <= 0) return DCGP_OK;
  ScopedTimer tm(ctx, "bern_grad");
  hipLaunchKernelGGL(bern_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, mu, var, y, n, K, n_labels, gh, weight, gm, gv);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int bern_predict(dcgp_ctx* ctx, const double* mu, const double* var, long n, double* out_mean, double* out_var) {
  if (n <= 0) return DCGP_OK;
  hipLaunchKernelGGL(bern_predict_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, mu, var, n, out_mean, out_var);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int bern_eval_tail(dcgp_ctx* ctx, const double* mu, const double* var, const double* y, int n, int S, int K, long lo, double* logdens,
                   double* ld_nd, double* p_mean, double* correct) {
  ScopedTimer tm(ctx, "bern_eval_tail");
  hipLaunchKernelGGL(bern_eval_tail_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, mu, var, y, n, S, K, lo, logdens,
                     ld_nd, p_mean, correct);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// gaussian.hip -- the Gaussian likelihood's tails (gpflow 1.x likelihoods.Gaussian under doubly_stochastic_dgp's
// BroadcastingLikelihood): one scalar variance s2 shared by every output, targets y [N][D] float64.
//
//   variational expectation per (row, d):  -0.5 log(2 pi s2) - 0.5 ((y - mu)^2 + v) / s2
//   predictive density per (image, d):     logsumexp_s log N(y; mu_s, v_s + s2) - log S
//
// Every kernel reads s2 from its device word (the optimiser moves it there), so steps enqueued back to back see the value the
// previous step left.  Sums run in a fixed order (a tree per workgroup, then the last workgroup to arrive over the partials in
// index order): results are bitwise reproducible, no float atomics.  The RobustMax tails (cond.hip, grad.hip, evaluate.hip) are
// untouched; likelihood.hip picks these by the model's Likelihood.
#include "layer_impl.h"
#include "tail_dev.h"

namespace {

constexpr double kLog2Pi = 1.83787706640934548356;

struct GaussTailArgs {
  TailArgs t;                      // mu / var [n_rows][K], ve [n_rows], inv_s, ticket, scal, fin (t.y, t.gh, t.eps unused)
  const double* y = nullptr;       // [n_labels][K]: row r reads y[(r % n_labels) * K ..]
  const double* s2 = nullptr;      // the likelihood variance (device word)
};

// ELBO tail: one thread per row (its D expectations summed in index order), ceil(rows / 256) workgroups, then the KlTail workgroups;
// the last workgroup to arrive sums the rows (per-thread strides, then a tree) and assembles the ELBO as elbo_tail_kernel does.
__global__ __launch_bounds__(256) void gauss_tail_kernel(GaussTailArgs a, KlTail kl) {
  __shared__ double red[4 * 256];
  __shared__ unsigned last;
  const TailArgs& t = a.t;
  const int tid = threadIdx.x;
  const int nb_rows = (t.n_rows + 255) / 256;
  if ((int)blockIdx.x >= nb_rows) {
    const int l = blockIdx.x - nb_rows;
    kl_pieces_block(kl.l[l], t.scal + 4 + 4 * l, red);
  } else {
    const int row = blockIdx.x * 256 + tid;
    if (row < t.n_rows) {
      const double s2 = *a.s2, inv = 1.0 / s2, c = -0.5 * (kLog2Pi + log(s2));
      const double* m = t.mu + (long)row * t.K;
      const double* v = t.var + (long)row * t.K;
      const double* yy = a.y + (long)(row % t.n_labels) * t.K;
      double s = 0.0;
      for (int d = 0; d < t.K; ++d) {
        const double e = yy[d] - m[d];
        s += c - 0.5 * (e * e + v[d]) * inv;
      }
      t.ve[row] = s;
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

// Reverse tail: d (w sum ve) / d(mu, var) per element and d / d s2 of the whole sum.  One thread per element of [rows][K]; each
// workgroup's share of the s2 gradient is a tree sum into part[blockIdx], the last to arrive adds the partials in index order.
__global__ __launch_bounds__(256) void gauss_grad_kernel(const double* __restrict__ mu, const double* __restrict__ var, const double* __restrict__ y,
                                                         long n, int K, int n_labels, const double* __restrict__ s2p, double weight,
                                                         double* __restrict__ gm, double* __restrict__ gv, double* part, unsigned* ticket,
                                                         double* __restrict__ gs2) {
  __shared__ double red[256];
  __shared__ unsigned last;
  const int tid = threadIdx.x;
  const long i = (long)blockIdx.x * 256 + tid;
  const double s2 = *s2p, inv = 1.0 / s2;
  double ts = 0.0;
  if (i < n) {
    const long row = i / K;
    const int d = (int)(i - row * K);
    const double e = y[(row % n_labels) * K + d] - mu[i];
    gm[i] = weight * e * inv;
    gv[i] = -0.5 * weight * inv;
    ts = -0.5 * inv + 0.5 * (e * e + var[i]) * inv * inv;
  }
  red[tid] = ts;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = red[0];
  if (!last_to_arrive(ticket, gridDim.x, &last)) return;
  double s = 0.0;
  for (int b = tid; b < (int)gridDim.x; b += 256) s += __hip_atomic_load(part + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) gs2[0] = weight * red[0];
}

// predict_y: (Fmean, Fvar + s2)
__global__ void gauss_predict_kernel(const double* __restrict__ mu, const double* __restrict__ var, long n, const double* __restrict__ s2p,
                                     double* __restrict__ out_mean, double* __restrict__ out_var) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (out_mean) out_mean[i] = mu[i];
  if (out_var) out_var[i] = var[i] + *s2p;
}

// Evaluation tail of one batch (head rows [S*n][K], row s*n + i): one thread per image, its K outputs in index order.  Per image at
// index lo + i of the whole set: the log density summed over the outputs (and per output where ld_nd is given), the sample-mean
// prediction and its squared error summed over the outputs.
__global__ __launch_bounds__(256) void gauss_eval_tail_kernel(const double* __restrict__ mu, const double* __restrict__ var, const double* __restrict__ y,
                                                              int n, int S, int K, const double* __restrict__ s2p, long lo,
                                                              double* __restrict__ logdens, double* __restrict__ ld_nd, double* __restrict__ y_mean,
                                                              double* __restrict__ sqerr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double s2 = *s2p;
  const long gi = lo + i;
  double ld = 0.0, se = 0.0;
  for (int d = 0; d < K; ++d) {
    const double yd = y[(long)i * K + d];
    double mx = -__builtin_inf(), msum = 0.0;
    for (int s = 0; s < S; ++s) {
      const long r = ((long)s * n + i) * K + d;
      const double vv = var[r] + s2, e = yd - mu[r];
      mx = fmax(mx, -0.5 * (kLog2Pi + log(vv)) - 0.5 * e * e / vv);
      msum += mu[r];
    }
    double acc = 0.0;
    for (int s = 0; s < S; ++s) {
      const long r = ((long)s * n + i) * K + d;
      const double vv = var[r] + s2, e = yd - mu[r];
      acc += exp(-0.5 * (kLog2Pi + log(vv)) - 0.5 * e * e / vv - mx);
    }
    const double l = mx + log(acc) - log((double)S);
    if (ld_nd) ld_nd[gi * K + d] = l;
    ld += l;
    const double ym = msum / (double)S, e = ym - yd;
    if (y_mean) y_mean[gi * K + d] = ym;
    se += e * e;
  }
  logdens[gi] = ld;
  sqerr[gi] = se;
}

// One workgroup behind the last batch: res[0] = sum of the squared errors, res[1] = sum of the log densities (strided per thread, then
// a tree), res[2] = first non-positive pivot of the factorisations the batches used.
__global__ __launch_bounds__(1024) void gauss_eval_sum_kernel(const double* __restrict__ logdens, const double* __restrict__ sqerr, long n,
                                                              FactorStatus st, double* __restrict__ res) {
  __shared__ double red[2][1024];
  const int tid = threadIdx.x;
  double s = 0.0, e = 0.0;
  for (long i = tid; i < n; i += 1024) { s += logdens[i]; e += sqerr[i]; }
  red[0][tid] = e; red[1][tid] = s;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
    __syncthreads();
  }
  if (tid != 0) return;
  const int pivot = first_bad_pivot(st);
  res[0] = red[0][0];
  res[1] = red[1][0];
  res[2] = (double)pivot;
  res[3] = 0.0;
}

}  // namespace

int gauss_elbo_tail(dcgp_ctx* ctx, const double* mu, const double* var, const double* y, int n_rows, int n_labels, int K, const double* s2,
                    double* ve_rows, double inv_s, double* scal, const ElboFinish& fin, const KlTail* kl) {
  GaussTailArgs a;
  DCGP_TRY(elbo_tail_prepare(ctx, &a.t));   // (the same arrival counter as elbo_tail: the two never share a launch)
  a.t.mu = mu; a.t.var = var; a.t.n_rows = n_rows; a.t.n_labels = n_labels; a.t.K = K; a.t.ve = ve_rows;
  a.t.inv_s = inv_s; a.t.scal = scal; a.t.fin = fin;
  a.y = y; a.s2 = s2;
  ScopedTimer tm(ctx, "gauss_tail");
  KlTail k;
  if (kl) k = *kl;
  hipLaunchKernelGGL(gauss_tail_kernel, dim3((unsigned)((n_rows + 255) / 256 + k.nl)), dim3(256), 0, ctx->stream, a, k);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int gauss_grad(dcgp_ctx* ctx, const double* mu, const double* var, const double* y, int rows, int K, int n_labels, const double* s2,
               double weight, double* gm, double* gv, double* gs2) {
  const long n = (long)rows * K;
  const unsigned nb = (unsigned)((n + 255) / 256);
  double* part = (double*)ws_get(ctx, "gauss_grad_part", (size_t)nb * sizeof(double));
  if (!part) return DCGP_ERR_ALLOC;
  auto it = ctx->ws.find("gauss_grad_ticket");
  unsigned* ticket = it != ctx->ws.end() ? (unsigned*)it->second.first : nullptr;
  if (!ticket) {
    ticket = (unsigned*)ws_get(ctx, "gauss_grad_ticket", 256);
    if (!ticket) return DCGP_ERR_ALLOC;
    HIP_TRY(ctx, hipMemsetAsync(ticket, 0, 256, ctx->stream));
  }
  ScopedTimer tm(ctx, "gauss_grad");
  hipLaunchKernelGGL(gauss_grad_kernel, dim3(nb), dim3(256), 0, ctx->stream, mu, var, y, n, K, n_labels, s2, weight, gm, gv, part, ticket, gs2);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int gauss_predict(dcgp_ctx* ctx, const double* mu, const double* var, long n, const double* s2, double* out_mean, double* out_var) {
  if (n <= 0) return DCGP_OK;
  hipLaunchKernelGGL(gauss_predict_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, mu, var, n, s2, out_mean, out_var);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int gauss_eval_tail(dcgp_ctx* ctx, const double* mu, const double* var, const double* y, int n, int S, int K, const double* s2, long lo,
                    double* logdens, double* ld_nd, double* y_mean, double* sqerr) {
  ScopedTimer tm(ctx, "gauss_eval_tail");
  hipLaunchKernelGGL(gauss_eval_tail_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, mu, var, y, n, S, K, s2, lo, logdens,
                     ld_nd, y_mean, sqerr);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int gauss_eval_sum(dcgp_ctx* ctx, const double* logdens, const double* sqerr, long n, const FactorStatus& st, double* res) {
  hipLaunchKernelGGL(gauss_eval_sum_kernel, dim3(1), dim3(1024), 0, ctx->stream, logdens, sqerr, n, st, res);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// pointwise.hip -- the tails of the per-output likelihoods (gpflow 1.x Likelihood.variational_expectations / predict_mean_and_var /
// predict_density, through ndiagquad where there is no closed form, under doubly_stochastic_dgp's BroadcastingLikelihood): one set of kernels,
// templated on a log-density functor of pointwise_dev.h, instantiated for Gaussian, Bernoulli (probit), StudentT and Poisson.
//
// With x_i, w_i the table's nodes and weights, c_i = w_i / sqrt(pi), s = sqrt(max(2 v, 1e-10)) and f_i = m + s x_i, per element (row, d) with
// mean m, variance v and target y -- or the functor's closed form, where it has one:
//   variational expectation  VE  = sum_i c_i logp(f_i, y)
//   predictive mean          E_y = sum_i c_i cm(f_i)
//   predictive variance      V_y = sum_i c_i (cv(f_i) + cm(f_i)^2) - E_y^2
//   log density              ld  = logsumexp_i (logp(f_i, y) + log c_i);  per (image, output) logsumexp_s ld_s - log S
// The reverse tail differentiates what the forward computes (the 20-node sum through sqrt(2 v), or the closed form), as TF autodiff of gpflow
// does -- not the E[g''] / 2 identity, which differs at finite order.  A trainable parameter (the Gaussian variance, the StudentT scale) is a
// device word (the optimiser moves it there), so steps enqueued back to back see the value the previous step left.  Sums run in a fixed
// order (index order per thread, a tree per workgroup, the last workgroup to arrive over the partials): results are bitwise reproducible, no
// float atomics.  One thread per element (forward, reverse, predictions) or image (evaluation): at cfg2 sizes these tails are latency-bound
// (DESIGN 4j.2, 4n, 4t).
#include "layer_impl.h"
#include "tail_dev.h"
#include "pointwise_dev.h"

namespace {

// logp at one node (b0 = the functor's base term, where it has one)
template <class D>
__device__ __forceinline__ double node_logp(const D& dn, double b0, double f, double y, double p) {
  if constexpr (D::kHasBase) return b0 + dn.tail(f, y, p);
  else return dn.tail(f, y, p);
}
template <class D>
__device__ __forceinline__ double base_of(const D& dn, double y, double p) {
  if constexpr (D::kHasBase) return dn.base(y, p);
  else return 0.0;
}

// sum_i c_i logp(m + s x_i, y), s = sqrt(max(2 v, 1e-10)); gh = {20 nodes, 20 weights}
template <class D>
__device__ __forceinline__ double quad_ve(const D& dn, double m, double v, double y, double p, const double* gh) {
  if constexpr (D::kClosedVe) return dn.ve(m, v, y, p);
  else {
    const double s = sqrt(fmax(2.0 * v, 1e-10)), b0 = base_of(dn, y, p);
    double acc = 0.0;
    for (int g = 0; g < 20; ++g) acc += gh[20 + g] * kInvSqrtPi * node_logp(dn, b0, m + s * gh[g], y, p);
    return acc;
  }
}

// log density of one sample: closed, or logsumexp_i (logp(m + s x_i, y) + log c_i) -- the maximum first, then the sum, both in node order
template <class D>
__device__ __forceinline__ double quad_logdens(const D& dn, double m, double v, double y, double p, const double* gh) {
  if constexpr (D::kClosedLogdens) return dn.logdens(m, v, y, p);
  else {
    const double s = sqrt(fmax(2.0 * v, 1e-10)), b0 = base_of(dn, y, p);
    double t[20], mx = -__builtin_inf();
#pragma unroll
    for (int g = 0; g < 20; ++g) {
      t[g] = node_logp(dn, b0, m + s * gh[g], y, p) + log(gh[20 + g] * kInvSqrtPi);
      mx = fmax(mx, t[g]);
    }
    double acc = 0.0;
#pragma unroll
    for (int g = 0; g < 20; ++g) acc += exp(t[g] - mx);
    return mx + log(acc);
  }
}

// (E_y, V_y) of one element
template <class D>
__device__ __forceinline__ void quad_mean_var(const D& dn, double m, double v, double p, const double* gh, double* e, double* vy) {
  if constexpr (D::kClosedPredict) dn.predict(m, v, p, e, vy);
  else {
    const double s = sqrt(fmax(2.0 * v, 1e-10));
    double a1 = 0.0, a2 = 0.0;
    for (int g = 0; g < 20; ++g) {
      const double f = m + s * gh[g], c = gh[20 + g] * kInvSqrtPi, mean = dn.cm(f, p);
      a1 += c * mean;
      a2 += c * (dn.cv(f, p) + mean * mean);
    }
    *e = a1; *vy = a2 - a1 * a1;
  }
}

template <class D>
struct QuadTailArgs {
  TailArgs t;                      // mu / var [n_rows][K], gh, ve [n_rows], inv_s, ticket, scal, fin (t.y, t.eps unused)
  const double* y = nullptr;       // [n_labels][K]: row r reads y[(r % n_labels) * K ..]
  D dn;
};

// The element mapping: a workgroup takes rows_per_block(K) whole rows, thread e of it element (e / K, e % K); a row wider than the
// kernel's LDS goes through it in chunks of kTailChunk outputs (then a workgroup has one row).
__host__ __device__ constexpr int rows_per_block(int K) { return K >= 256 ? 1 : 256 / K; }
constexpr int kTailChunk = 1024;

// ELBO tail: one thread per element, each row's K expectations through LDS and summed in index order by the row's first thread (across the
// chunks of a wide row too); then the KlTail workgroups; the last workgroup to arrive sums the rows (per-thread strides, then a tree) and
// assembles the ELBO as elbo_tail_kernel does.  (One thread per row ran its K quadratures back to back: 92 us at K = 10 against 12 us for
// elbo_tail_kernel.)
template <class D>
__global__ __launch_bounds__(256) void quad_tail_kernel(QuadTailArgs<D> a, KlTail kl, int nb_rows) {
  __shared__ double red[kTailChunk];
  __shared__ unsigned last;
  const TailArgs& t = a.t;
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= nb_rows) {
    const int l = blockIdx.x - nb_rows;
    kl_pieces_block(kl.l[l], t.scal + 4 + 4 * l, red);
  } else {
    const int rpb = rows_per_block(t.K), row0 = blockIdx.x * rpb;
    const int nrows = min(rpb, t.n_rows - row0);
    const double p = a.dn.param();
    double s = 0.0;
    for (int k0 = 0; k0 < t.K; k0 += kTailChunk) {
      const int kc = min(kTailChunk, t.K - k0);
      for (int e = tid; e < nrows * kc; e += 256) {
        const int row = row0 + e / kc, d = k0 + e % kc;
        const double yd = a.y[(long)(row % t.n_labels) * t.K + d];
        red[e] = quad_ve(a.dn, t.mu[(long)row * t.K + d], t.var[(long)row * t.K + d], yd, p, t.gh);
      }
      __syncthreads();
      if (tid < nrows)
        for (int d = 0; d < kc; ++d) s += red[tid * kc + d];
      __syncthreads();   // (the next chunk overwrites red)
    }
    if (tid < nrows) t.ve[row0 + tid] = s;
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

// Reverse tail: d (weight * ve) / d mu and / d v per element of [rows][K], one thread each.  With f_i = mu + s x_i and g_i = logp'(f_i):
//   d/dmu = sum_i c_i g_i,  d/dv = sum_i c_i g_i x_i / s (0 where the clamp holds)          (closed form: the functor's ve_grad)
// and, for a likelihood with a parameter, d / d p = sum over the elements of sum_i c_i d logp(f_i) / d p (closed form: ve_grad's): each
// workgroup's share is a tree sum into part[blockIdx], the last to arrive adds the partials in index order.
template <class D>
__global__ __launch_bounds__(256) void quad_grad_kernel(D dn, const double* __restrict__ mu, const double* __restrict__ var, const double* __restrict__ y,
                                                        long n, int K, int n_labels, const double* __restrict__ gh, double weight,
                                                        double* __restrict__ gm, double* __restrict__ gv, double* part, unsigned* ticket,
                                                        double* __restrict__ gpar) {
  __shared__ double red[256];
  __shared__ unsigned last;
  const int tid = threadIdx.x;
  const long i = (long)blockIdx.x * 256 + tid;
  const double p = dn.param();
  double tp = 0.0;
  if (i < n) {
    const long row = i / K;
    const int d = (int)(i - row * K);
    const double yd = y[(row % n_labels) * K + d];
    const double m = mu[i], v = var[i];
    if constexpr (D::kClosedVe) {
      dn.ve_grad(m, v, yd, p, weight, gm + i, gv + i, &tp);
    } else {
      const bool live = 2.0 * v > 1e-10;
      const double s = sqrt(fmax(2.0 * v, 1e-10));
      double am = 0.0, av = 0.0;
      for (int g = 0; g < 20; ++g) {
        const double f = m + s * gh[g], c = gh[20 + g] * kInvSqrtPi;
        const double q = c * dn.dtail(f, yd, p);
        am += q;
        av += q * gh[g];
        if constexpr (D::kHasParam) tp += c * dn.dparam(f, yd, p);
      }
      gm[i] = weight * am;
      gv[i] = live ? weight * av / s : 0.0;
    }
  }
  if (!D::kHasParam) return;
  red[tid] = tp;
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
  if (tid == 0) gpar[0] = weight * red[0];
}

// Per element of [n] (rows x K flattened; y, where read, has the same shape): what = 0 the variational expectation (out_a), 1 (E_y, V_y)
// (out_a, out_b; either may be nullptr), 2 the log density of the one sample (out_a).
template <class D>
__global__ __launch_bounds__(256) void quad_elem_kernel(D dn, int what, const double* __restrict__ mu, const double* __restrict__ var,
                                                        const double* __restrict__ y, long n, const double* __restrict__ gh,
                                                        double* __restrict__ out_a, double* __restrict__ out_b) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double p = dn.param();
  if (what == 0) {
    out_a[i] = quad_ve(dn, mu[i], var[i], y[i], p, gh);
  } else if (what == 2) {
    out_a[i] = quad_logdens(dn, mu[i], var[i], y[i], p, gh);
  } else {
    double e, vy;
    quad_mean_var(dn, mu[i], var[i], p, gh, &e, &vy);
    if (out_a) out_a[i] = e;
    if (out_b) out_b[i] = vy;
  }
}

// Evaluation tail of one batch (head rows [S*n][K], row s*n + i): one thread per image, its K outputs in index order.  Per image at
// index lo + i of the whole set: the log density summed over the outputs (and per output where ld_nd is given), the sample-mean E_y
// (y_mean, may be nullptr; Bernoulli: the mean p) and the functor's score of that mean summed over the outputs (the squared error;
// Bernoulli: the outputs whose label is 1 exactly where the mean is > 0.5); quad_eval_sum_kernel adds those up.
template <class D>
__global__ __launch_bounds__(256) void quad_eval_tail_kernel(D dn, const double* __restrict__ mu, const double* __restrict__ var,
                                                        const double* __restrict__ y, int n, int S, int K, const double* __restrict__ gh,
                                                        long lo, double* __restrict__ logdens, double* __restrict__ ld_nd,
                                                        double* __restrict__ y_mean, double* __restrict__ score) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double p = dn.param();
  const long gi = lo + i;
  double ld = 0.0, sc = 0.0;
  for (int d = 0; d < K; ++d) {
    const double yd = y[(long)i * K + d];
    double mx = -__builtin_inf(), msum = 0.0;
    for (int s = 0; s < S; ++s) {
      const long r = ((long)s * n + i) * K + d;
      double e, vy;
      quad_mean_var(dn, mu[r], var[r], p, gh, &e, &vy);
      mx = fmax(mx, quad_logdens(dn, mu[r], var[r], yd, p, gh));
      msum += e;
    }
    double acc = 0.0;
    for (int s = 0; s < S; ++s) {
      const long r = ((long)s * n + i) * K + d;
      acc += exp(quad_logdens(dn, mu[r], var[r], yd, p, gh) - mx);
    }
    const double l = mx + log(acc) - log((double)S);
    if (ld_nd) ld_nd[gi * K + d] = l;
    ld += l;
    const double ym = msum / (double)S;
    if (y_mean) y_mean[gi * K + d] = ym;
    sc += dn.score(ym, yd);
  }
  logdens[gi] = ld;
  score[gi] = sc;
}

// One workgroup behind the last batch: res[0] = sum of the scores, res[1] = sum of the log densities (strided per thread, then a tree),
// res[2] = first non-positive pivot of the factorisations the batches used.
__global__ __launch_bounds__(1024) void quad_eval_sum_kernel(const double* __restrict__ logdens, const double* __restrict__ score, long n,
                                                        FactorStatus st, double* __restrict__ res) {
  __shared__ double red[2][1024];
  const int tid = threadIdx.x;
  double s = 0.0, e = 0.0;
  for (long i = tid; i < n; i += 1024) { s += logdens[i]; e += score[i]; }
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

// f(functor) of the descriptor's kind
template <class F>
int with_density(dcgp_ctx* ctx, const QuadLik& q, const char* who, F&& f) {
  switch (q.kind) {
    case 1: return f(GaussianDensity{q.par, q.par_val});
    case 2: return f(BernoulliDensity{});
    case 4: return f(StudentTDensity{q.par, q.par_val, q.nu, q.c_nu});
    case 5: return f(PoissonDensity{q.binsize, log(q.binsize)});
    default: return ctx_fail(ctx, DCGP_ERR_ARG, "%s: kind 1 (Gaussian), 2 (Bernoulli), 4 (StudentT) or 5 (Poisson), got %d", who, q.kind);
  }
}

}  // namespace

int quad_elbo_tail(dcgp_ctx* ctx, const QuadLik& q, const double* mu, const double* var, const double* y, int n_rows, int n_labels, int K,
                   double* ve_rows, double inv_s, double* scal, const ElboFinish& fin, const KlTail* kl) {
  if (K < 1) return ctx_fail(ctx, DCGP_ERR_ARG, "elbo tail: the head has %d outputs", K);
  return with_density(ctx, q, "elbo tail", [&](auto dn) {
    QuadTailArgs<decltype(dn)> a;
    DCGP_TRY(elbo_tail_prepare(ctx, &a.t));   // (Gauss-Hermite table; the same arrival counter as elbo_tail: the two never share a launch)
    a.t.mu = mu; a.t.var = var; a.t.n_rows = n_rows; a.t.n_labels = n_labels; a.t.K = K; a.t.ve = ve_rows;
    a.t.inv_s = inv_s; a.t.scal = scal; a.t.fin = fin;
    a.y = y; a.dn = dn;
    const int rpb = rows_per_block(K), nb_rows = (n_rows + rpb - 1) / rpb;
    ScopedTimer tm(ctx, "quad_tail");
    KlTail k;
    if (kl) k = *kl;
    hipLaunchKernelGGL(quad_tail_kernel<decltype(dn)>, dim3((unsigned)(nb_rows + k.nl)), dim3(256), 0, ctx->stream, a, k, nb_rows);
    LAUNCH_CHECK(ctx);
    return DCGP_OK;
  });
}

int quad_grad(dcgp_ctx* ctx, const QuadLik& q, const double* mu, const double* var, const double* y, int rows, int K, int n_labels, double weight,
              double* gm, double* gv, double* gpar) {
  const double* gh = gauss_hermite_table(ctx);
  if (!gh) return DCGP_ERR_ALLOC;
  const long n = (long)rows * K;
  if (n <= 0) return DCGP_OK;
  return with_density(ctx, q, "grad", [&](auto dn) {
    const unsigned nb = (unsigned)((n + 255) / 256);
    double* part = nullptr;
    unsigned* ticket = nullptr;
    if (dn.kHasParam) {
      if (!gpar) return ctx_fail(ctx, DCGP_ERR_ARG, "grad: the %s likelihood needs a slot for its %s's gradient", q.kind == 1 ? "Gaussian" : "StudentT",
                                 q.kind == 1 ? "variance" : "scale");
      part = (double*)ws_get(ctx, "quad_grad_part", (size_t)nb * sizeof(double));
      if (!part) return DCGP_ERR_ALLOC;
      auto it = ctx->ws.find("quad_grad_ticket");
      ticket = it != ctx->ws.end() ? (unsigned*)it->second.first : nullptr;
      if (!ticket) {
        ticket = (unsigned*)ws_get(ctx, "quad_grad_ticket", 256);
        if (!ticket) return DCGP_ERR_ALLOC;
        HIP_TRY(ctx, hipMemsetAsync(ticket, 0, 256, ctx->stream));
      }
    }
    ScopedTimer tm(ctx, "quad_grad");
    hipLaunchKernelGGL(quad_grad_kernel<decltype(dn)>, dim3(nb), dim3(256), 0, ctx->stream, dn, mu, var, y, n, K, n_labels, gh, weight, gm, gv, part,
                       ticket, gpar);
    LAUNCH_CHECK(ctx);
    return DCGP_OK;
  });
}

int quad_elementwise(dcgp_ctx* ctx, const QuadLik& q, int what, const double* mu, const double* var, const double* y, long n, double* out_a,
                     double* out_b) {
  const double* gh = gauss_hermite_table(ctx);
  if (!gh) return DCGP_ERR_ALLOC;
  if (n <= 0) return DCGP_OK;
  return with_density(ctx, q, "elementwise", [&](auto dn) {
    hipLaunchKernelGGL(quad_elem_kernel<decltype(dn)>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, dn, what, mu, var, y, n, gh, out_a,
                       out_b);
    LAUNCH_CHECK(ctx);
    return DCGP_OK;
  });
}

int quad_eval_tail(dcgp_ctx* ctx, const QuadLik& q, const double* mu, const double* var, const double* y, int n, int S, int K, long lo,
                   double* logdens, double* ld_nd, double* y_mean, double* score) {
  const double* gh = gauss_hermite_table(ctx);
  if (!gh) return DCGP_ERR_ALLOC;
  return with_density(ctx, q, "evaluate", [&](auto dn) {
    ScopedTimer tm(ctx, "quad_eval_tail");
    hipLaunchKernelGGL(quad_eval_tail_kernel<decltype(dn)>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, dn, mu, var, y, n, S, K, gh, lo,
                       logdens, ld_nd, y_mean, score);
    LAUNCH_CHECK(ctx);
    return DCGP_OK;
  });
}

int quad_eval_sum(dcgp_ctx* ctx, const double* logdens, const double* score, long n, const FactorStatus& st, double* res) {
  hipLaunchKernelGGL(quad_eval_sum_kernel, dim3(1), dim3(1024), 0, ctx->stream, logdens, score, n, st, res);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// ---- the stand-alone entry points (StudentT and Poisson) -----------------------------------------------------------------------------------
namespace {
// params_host of the C ABI: kind 4 {scale, deg_free}, kind 5 {binsize}
int quad_from_params(dcgp_ctx* ctx, int kind, const double* params, const char* who, QuadLik* q) {
  if (!params) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: params is NULL", who);
  q->kind = kind;
  if (kind == 4) {
    if (!(params[0] > 1e-6) || !(params[1] > 2.0) || !std::isfinite(params[0]) || !std::isfinite(params[1]))
      return ctx_fail(ctx, DCGP_ERR_ARG, "%s: StudentT needs scale > 1e-6 and deg_free > 2, got %g, %g", who, params[0], params[1]);
    q->par_val = params[0]; q->nu = params[1]; q->c_nu = student_t_const(params[1]);
  } else if (kind == 5) {
    if (!(params[0] > 0) || !std::isfinite(params[0])) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: Poisson needs binsize > 0, got %g", who, params[0]);
    q->binsize = params[0];
  } else {
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: kind 4 (StudentT) or 5 (Poisson), got %d", who, kind);
  }
  return DCGP_OK;
}
}  // namespace

double student_t_const(double nu) { return std::lgamma(0.5 * (nu + 1.0)) - std::lgamma(0.5 * nu) - 0.5 * std::log(nu * 3.14159265358979323846); }

extern "C" {

int dcgp_quad_varexp(dcgp_ctx* ctx, int kind, const double* params_host, const double* mu, const double* var, const double* y, int n, int K,
                     double* out) {
  if (!ctx) return DCGP_ERR_ARG;
  if (!mu || !var || !y || !out || n <= 0 || K <= 0) return ctx_fail(ctx, DCGP_ERR_ARG, "quad_varexp: bad args");
  QuadLik q;
  DCGP_TRY(quad_from_params(ctx, kind, params_host, "quad_varexp", &q));
  DCGP_TRY(quad_elementwise(ctx, q, 0, mu, var, y, (long)n * K, out, nullptr));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

int dcgp_quad_predict(dcgp_ctx* ctx, int kind, const double* params_host, const double* mu, const double* var, int n, int K, double* out_mean,
                      double* out_var) {
  if (!ctx) return DCGP_ERR_ARG;
  if (!mu || !var || (!out_mean && !out_var) || n <= 0 || K <= 0) return ctx_fail(ctx, DCGP_ERR_ARG, "quad_predict: bad args");
  QuadLik q;
  DCGP_TRY(quad_from_params(ctx, kind, params_host, "quad_predict", &q));
  DCGP_TRY(quad_elementwise(ctx, q, 1, mu, var, nullptr, (long)n * K, out_mean, out_var));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

int dcgp_quad_logdensity(dcgp_ctx* ctx, int kind, const double* params_host, const double* mu, const double* var, const double* y, int n, int K,
                         double* out) {
  if (!ctx) return DCGP_ERR_ARG;
  if (!mu || !var || !y || !out || n <= 0 || K <= 0) return ctx_fail(ctx, DCGP_ERR_ARG, "quad_logdensity: bad args");
  QuadLik q;
  DCGP_TRY(quad_from_params(ctx, kind, params_host, "quad_logdensity", &q));
  DCGP_TRY(quad_elementwise(ctx, q, 2, mu, var, y, (long)n * K, out, nullptr));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

int dcgp_quad_grad_seeds(dcgp_ctx* ctx, int kind, const double* params_host, const double* mu, const double* var, const double* y, int n, int K,
                         double weight, double* out_gm, double* out_gv, double* out_gparam) {
  if (!ctx) return DCGP_ERR_ARG;
  if (!mu || !var || !y || !out_gm || !out_gv || n <= 0 || K <= 0 || (kind == 4 && !out_gparam)) return ctx_fail(ctx, DCGP_ERR_ARG, "quad_grad_seeds: bad args");
  QuadLik q;
  DCGP_TRY(quad_from_params(ctx, kind, params_host, "quad_grad_seeds", &q));
  DCGP_TRY(quad_grad(ctx, q, mu, var, y, n, K, n, weight, out_gm, out_gv, out_gparam));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

}  // extern "C"

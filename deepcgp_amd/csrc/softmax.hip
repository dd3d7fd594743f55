// softmax.hip -- the Softmax multi-class likelihood's tails (gpflow 1.x likelihoods.SoftMax / MonteCarloLikelihood with the per-call random
// draw replaced by a FIXED table of nodes e [Q][K], standard-normal draws shared by every row: a Q-node rule used the way the 20 Gauss-Hermite
// nodes are used for RobustMax and Bernoulli).  int32 labels y in [0, K).  Per head row with mean mu [K], variance v [K]:
//
//   s_k   = sqrt(max(v_k, 1e-10))                      (d / d v_k = 0 where the clamp holds, as quad_grad_kernel)
//   f_q   = mu + s o e_q,  lse_q = logsumexp_k f_q[k]  (max-subtracted),  sig_q = exp(f_q - lse_q)
//   variational expectation  ve = 1/Q sum_q (f_q[y] - lse_q)
//     d ve / d mu_k = 1/Q sum_q ([k == y] - sig_q[k]),   d ve / d v_k = 1/Q sum_q ([k == y] - sig_q[k]) e_q[k] / (2 s_k)
//   predictive mean  p[k] = 1/Q sum_q sig_q[k], variance p - p^2;  density of a sample log p[y];  per image log(1/S sum_s p_s[y])
//
// Layout.  The table is staged in LDS once per workgroup.  A workgroup takes a GROUP of rows (whole rows of the batch, or samples of one
// image) in three phases: (row, q) items leave lse_q in LDS; (row, k, c) items add the terms of the 16 nodes of chunk c in index order;
// (row, k) items add the chunk sums in index order.  No cross-lane reduction, no float atomics, and which thread runs an item does not
// change what it computes: two calls give the same bits, and every kernel here gives the same bits for the same row (predict_y,
// evaluate, evaluate_uncertainty and the density objective of input_grad agree on p to the bit).  The price is two exps per (q, k).
// Groups are small -- sm_group_rows: at most 256 / K rows (the Bernoulli tail's rows per workgroup), 512 / Q and 1024 / (K chunks) -- so
// a cfg2 step (320 rows, K = 10, Q = 100) is 64 workgroups of ~2 lse items and ~1.4 chunk items per thread, not 320 threads running
// 1000 exps back to back (the trap pointwise.hip's comment measures).
#include "model_state.h"
#include "tail_dev.h"
#include "unc_dev.h"

namespace {

constexpr int kSmChunk = 16;        // nodes per chunk sum
constexpr int kSmMaxTable = 4096;   // Q * K doubles of LDS (32 KB)
constexpr int kSmMaxLds = 8000;     // doubles of dynamic LDS a launch may ask for (64 KB less the kernels' static words)

__host__ __device__ inline int sm_chunks(int Q) { return (Q + kSmChunk - 1) / kSmChunk; }
// doubles of chunk sums of a group of G rows (one chunk: the items emit at once, nothing is kept)
__host__ __device__ inline long sm_part(int G, int K, int Q) { return sm_chunks(Q) > 1 ? (long)G * K * sm_chunks(Q) : 0; }
// rows of a group: lse [G][Q] and the chunk sums [G][K][chunks] stay small, and G <= `cap`
inline int sm_group_rows(int K, int Q, int cap) {
  int g = cap;
  g = std::min(g, 512 / Q);
  g = std::min(g, 1024 / (K * sm_chunks(Q)));
  return std::max(g, 1);
}

__device__ __forceinline__ double sm_sd(double v) { return sqrt(fmax(v, 1e-10)); }
__device__ __forceinline__ double sm_sig(double m, double s, double e, double lse) { return exp(m + s * e - lse); }

// logsumexp_k (m[k] + s_k e[k]), max-subtracted
__device__ __forceinline__ double sm_lse(const double* __restrict__ m, const double* __restrict__ v, const double* e, int K) {
  double mx = -__builtin_inf();
  for (int k = 0; k < K; ++k) mx = fmax(mx, m[k] + sm_sd(v[k]) * e[k]);
  double acc = 0.0;
  for (int k = 0; k < K; ++k) acc += exp(m[k] + sm_sd(v[k]) * e[k] - mx);
  return mx + log(acc);
}

__device__ __forceinline__ void sm_stage(const double* __restrict__ nodes, int QK, double* tab) {
  for (int i = threadIdx.x; i < QK; i += blockDim.x) tab[i] = nodes[i];
}

// rows row_base + r * row_stride, r < g: lse[r * Q + q]; with wy also wy[r * Q + q] = sig_q[y_r] (y_r = lab[r], inside [0, K))
__device__ __forceinline__ void sm_group_lse(const double* __restrict__ mu, const double* __restrict__ var, long row_base, long row_stride, int g, int K,
                                             const double* tab, int Q, double* lse, double* wy = nullptr, const int* lab = nullptr) {
  for (int it = threadIdx.x; it < g * Q; it += blockDim.x) {
    const int r = it / Q, q = it - r * Q;
    const long o = (row_base + r * row_stride) * K;
    const double l = sm_lse(mu + o, var + o, tab + q * K, K);
    lse[it] = l;
    if (wy) wy[it] = sm_sig(mu[o + lab[r]], sm_sd(var[o + lab[r]]), tab[q * K + lab[r]], l);
  }
}

// p[k] = 1/Q sum_q sig_q[k] of the group's rows -> emit(r * K + k, p): chunk sums in index order, then the chunks in index order
template <class Emit>
__device__ __forceinline__ void sm_group_probs(const double* __restrict__ mu, const double* __restrict__ var, long row_base, long row_stride, int g, int K,
                                               const double* tab, int Q, const double* lse, double* part, Emit emit) {
  const int nc = sm_chunks(Q);
  for (int it = threadIdx.x; it < g * K * nc; it += blockDim.x) {
    const int c = it % nc, rk = it / nc, r = rk / K, k = rk - r * K;
    const long o = (row_base + r * row_stride) * K + k;
    const double m = mu[o], s = sm_sd(var[o]);
    const int q1 = min(Q, kSmChunk * (c + 1));
    double a = 0.0;
    for (int q = kSmChunk * c; q < q1; ++q) a += sm_sig(m, s, tab[q * K + k], lse[r * Q + q]);
    if (nc == 1) emit(rk, a / (double)Q);
    else part[it] = a;
  }
  if (nc == 1) return;
  __syncthreads();
  for (int rk = threadIdx.x; rk < g * K; rk += blockDim.x) {
    double a = 0.0;
    for (int c = 0; c < nc; ++c) a += part[rk * nc + c];
    emit(rk, a / (double)Q);
  }
}

// A = sum_q w_q ([k == y] - sig_q[k]), B = sum_q w_q ([k == y] - sig_q[k]) e_q[k] of the group's rows -> emit(r * K + k, A, B), the same
// two levels.  w_q = 1 (DENS false: the variational expectation's terms) or wy[r * Q + q] = sig_q[y] (DENS: the terms of d p[y]).
template <bool DENS, class Emit>
__device__ __forceinline__ void sm_group_grad(const double* __restrict__ mu, const double* __restrict__ var, long row_base, long row_stride, int g, int K,
                                              const double* tab, int Q, const double* lse, const double* wy, const int* lab, double* part, Emit emit) {
  const int nc = sm_chunks(Q);
  const int n_items = g * K * nc;
  for (int it = threadIdx.x; it < n_items; it += blockDim.x) {
    const int c = it % nc, rk = it / nc, r = rk / K, k = rk - r * K;
    const long o = (row_base + r * row_stride) * K + k;
    const double m = mu[o], s = sm_sd(var[o]), ind = k == lab[r] ? 1.0 : 0.0;
    const int q1 = min(Q, kSmChunk * (c + 1));
    double a = 0.0, b = 0.0;
    for (int q = kSmChunk * c; q < q1; ++q) {
      const double e = tab[q * K + k];
      double d = ind - sm_sig(m, s, e, lse[r * Q + q]);
      if (DENS) d *= wy[r * Q + q];
      a += d;
      b += d * e;
    }
    if (nc == 1) emit(rk, a, b);
    else { part[it] = a; part[n_items + it] = b; }
  }
  if (nc == 1) return;
  __syncthreads();
  for (int rk = threadIdx.x; rk < g * K; rk += blockDim.x) {
    double a = 0.0, b = 0.0;
    for (int c = 0; c < nc; ++c) { a += part[rk * nc + c]; b += part[n_items + rk * nc + c]; }
    emit(rk, a, b);
  }
}

// ---- ELBO tail ------------------------------------------------------------------------------------------------------------------------
struct SmRowsArgs {
  const double* mu = nullptr; const double* var = nullptr;   // [n_rows][K]
  const int32_t* y = nullptr; int n_rows = 0, n_labels = 0, K = 0;   // row r reads y[r % n_labels]
  const double* nodes = nullptr; int Q = 0;
  int G = 1;                                                  // rows per workgroup
};

// ve of the rows row0 .. row0 + nrows of a workgroup (sm: tab [Q K], term [G Q], part [G 16]): (row, q) items leave f_q[y] - lse_q, (row, c)
// items add Q / 16 of them in index order, the row's thread the 16 sums.  A label outside [0, K) gives NaN; nothing is read at it.
__device__ __forceinline__ void sm_ve_rows(const SmRowsArgs& a, int row0, int nrows, double* sm, double* __restrict__ ve) {
  double* tab = sm;
  double* term = sm + a.Q * a.K;
  double* part = term + a.G * a.Q;
  const int tid = threadIdx.x, K = a.K, Q = a.Q;
  sm_stage(a.nodes, Q * K, tab);
  __syncthreads();
  for (int it = tid; it < nrows * Q; it += 256) {
    const int r = it / Q, q = it - r * Q;
    const long row = row0 + r, o = row * K;
    const int yi = a.y[row % a.n_labels];
    const double* e = tab + q * K;
    const double l = sm_lse(a.mu + o, a.var + o, e, K);
    term[it] = (yi >= 0 && yi < K) ? a.mu[o + yi] + sm_sd(a.var[o + yi]) * e[yi] - l : __builtin_nan("");
  }
  __syncthreads();
  const int cl = (Q + 15) / 16;
  for (int it = tid; it < nrows * 16; it += 256) {
    const int r = it >> 4, c = it & 15;
    const int q1 = min(Q, cl * (c + 1));
    double s = 0.0;
    for (int q = cl * c; q < q1; ++q) s += term[r * Q + q];
    part[it] = s;
  }
  __syncthreads();
  if (tid < nrows) {
    double s = 0.0;
    for (int c = 0; c < 16; ++c) s += part[tid * 16 + c];
    ve[row0 + tid] = s / (double)Q;
  }
}

// The rows' workgroups, then the KlTail workgroups; the last workgroup to arrive sums the rows and assembles the ELBO as quad_tail_kernel and
// elbo_tail_kernel do.  Dynamic LDS: the rows' buffers, at least the 1024 doubles of kl_pieces_block.
__global__ __launch_bounds__(256) void softmax_tail_kernel(SmRowsArgs a, TailArgs t, KlTail kl, int nb_rows) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ unsigned last;
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= nb_rows) {
    const int l = blockIdx.x - nb_rows;
    kl_pieces_block(kl.l[l], t.scal + 4 + 4 * l, sm);
  } else {
    const int row0 = blockIdx.x * a.G;
    sm_ve_rows(a, row0, min(a.G, a.n_rows - row0), sm, t.ve);
  }
  if (!last_to_arrive(t.ticket, gridDim.x, &last)) return;
  double s = 0.0;
  for (int i = tid; i < t.n_rows; i += 256) s += __hip_atomic_load(t.ve + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  sm[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sm[tid] += sm[tid + o];
    __syncthreads();
  }
  if (tid == 0) elbo_assemble(t.scal, t.fin, sm[0] * t.inv_s);
}

// dcgp_softmax_varexp: the rows alone; bad[0] = labels outside [0, K) (counted by workgroup 0, one thread per stride)
__global__ __launch_bounds__(256) void softmax_varexp_kernel(SmRowsArgs a, double* __restrict__ ve, int* __restrict__ bad) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ int cnt[256];
  const int row0 = blockIdx.x * a.G;
  sm_ve_rows(a, row0, min(a.G, a.n_rows - row0), sm, ve);
  if (blockIdx.x) return;
  int c = 0;
  for (int i = threadIdx.x; i < a.n_labels; i += 256) c += (a.y[i] < 0 || a.y[i] >= a.K) ? 1 : 0;
  cnt[threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) cnt[threadIdx.x] += cnt[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) bad[0] = cnt[0];
}

// ---- reverse tail and predictions: one workgroup per group of G rows -------------------------------------------------------------------
// sm: tab [Q K], lse [G Q], part [2 G K chunks], lab [G] (ints)
__global__ __launch_bounds__(256) void softmax_grad_kernel(SmRowsArgs a, double weight, double* __restrict__ gm, double* __restrict__ gv) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int K = a.K, Q = a.Q;
  double* tab = sm;
  double* lse = tab + Q * K;
  double* part = lse + a.G * Q;
  int* lab = (int*)(part + 2 * sm_part(a.G, K, Q));
  const int row0 = blockIdx.x * a.G, g = min(a.G, a.n_rows - row0);
  sm_stage(a.nodes, Q * K, tab);
  if ((int)threadIdx.x < g) lab[threadIdx.x] = a.y[(row0 + threadIdx.x) % a.n_labels];   // (outside [0, K): no class carries the indicator)
  __syncthreads();
  sm_group_lse(a.mu, a.var, row0, 1, g, K, tab, Q, lse);
  __syncthreads();
  const double w = weight / (double)Q;
  sm_group_grad<false>(a.mu, a.var, row0, 1, g, K, tab, Q, lse, nullptr, lab, part, [&](int rk, double A, double B) {
    const long o = (long)row0 * K + rk;
    const double v = a.var[o];
    gm[o] = w * A;
    gv[o] = v > 1e-10 ? w * B / (2.0 * sm_sd(v)) : 0.0;
  });
}

__global__ __launch_bounds__(256) void softmax_predict_kernel(SmRowsArgs a, double* __restrict__ out_mean, double* __restrict__ out_var) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int K = a.K, Q = a.Q;
  double* tab = sm;
  double* lse = tab + Q * K;
  double* part = lse + a.G * Q;
  const int row0 = blockIdx.x * a.G, g = min(a.G, a.n_rows - row0);
  sm_stage(a.nodes, Q * K, tab);
  __syncthreads();
  sm_group_lse(a.mu, a.var, row0, 1, g, K, tab, Q, lse);
  __syncthreads();
  sm_group_probs(a.mu, a.var, row0, 1, g, K, tab, Q, lse, part, [&](int rk, double p) {
    const long o = (long)row0 * K + rk;
    if (out_mean) out_mean[o] = p;
    if (out_var) out_var[o] = p - p * p;
  });
}

// ---- per-image tails: one workgroup per image, its S samples in groups of G ---------------------------------------------------------------
// p [S][K] (LDS) of image i: rows s n + i
__device__ __forceinline__ void sm_image_probs(const double* __restrict__ mu, const double* __restrict__ var, int n, int i, int S, int K, const double* tab,
                                               int Q, int G, double* lse, double* part, double* p) {
  for (int s0 = 0; s0 < S; s0 += G) {
    const int g = min(G, S - s0);
    sm_group_lse(mu, var, (long)s0 * n + i, n, g, K, tab, Q, lse);
    __syncthreads();
    sm_group_probs(mu, var, (long)s0 * n + i, n, g, K, tab, Q, lse, part, [&](int rk, double v) { p[s0 * K + rk] = v; });
    __syncthreads();
  }
}

// log (1/S sum_s p_s) = max_s l_s + log sum_s exp(l_s - max) - log S,  l_s = log p_s  (eval_tail_kernel's statements), p_s = p[s * stride];
// -inf where every p_s has underflowed to 0 (a label ~1600 nats below the favoured class: RobustMax's eps keeps its p away from there)
__device__ __forceinline__ double sm_logdens(const double* p, int stride, int S) {
  double mx = -__builtin_inf();
  for (int s = 0; s < S; ++s) mx = fmax(mx, log(p[s * stride]));
  if (mx == -__builtin_inf()) return mx;
  double se = 0.0;
  for (int s = 0; s < S; ++s) se += exp(log(p[s * stride]) - mx);
  return mx + log(se) - log((double)S);
}

struct SmImgArgs {
  const double* nodes = nullptr; int Q = 0, G = 1;
};

// eval_tail_kernel's outputs from the softmax rule.  sm: tab, lse [G Q], part [G K chunks], p [S K], pbar [K]
__global__ __launch_bounds__(kUncThreads) void softmax_eval_tail_kernel(SmImgArgs g, const double* __restrict__ mu, const double* __restrict__ var,
                                                                        const int32_t* __restrict__ y, int n, int S, int K, long lo,
                                                                        double* __restrict__ logdens, double* __restrict__ p_mean, int* __restrict__ ok) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int Q = g.Q;
  double* tab = sm;
  double* lse = tab + Q * K;
  double* part = lse + g.G * Q;
  double* p = part + sm_part(g.G, K, Q);
  double* pbar = p + S * K;
  const int i = blockIdx.x, tid = threadIdx.x;
  sm_stage(g.nodes, Q * K, tab);
  __syncthreads();
  sm_image_probs(mu, var, n, i, S, K, tab, Q, g.G, lse, part, p);
  const long gi = lo + i;
  for (int k = tid; k < K; k += kUncThreads) {
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += p[s * K + k];
    pbar[k] = acc / (double)S;
    if (p_mean) p_mean[gi * K + k] = pbar[k];
  }
  __syncthreads();
  if (tid != 0) return;
  const int yi = y[i];
  if (yi < 0 || yi >= K) {   // reported by the sum kernel as an argument error; nothing is read at the label
    logdens[gi] = __builtin_nan("");
    ok[gi] = -1;
    return;
  }
  logdens[gi] = sm_logdens(p + yi, K, S);
  int best = 0;   // first index of the largest: numpy's argmax on ties
  for (int k = 1; k < K; ++k)
    if (pbar[k] > pbar[best]) best = k;
  ok[gi] = best == yi ? 1 : 0;
}

// unc_tail_kernel with the probabilities of the softmax rule: everything behind them is unc_tail_finish.  sm: as above, then part3 [48]
__global__ __launch_bounds__(kUncThreads) void softmax_unc_tail_kernel(SmImgArgs g, UncTailArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int Q = g.Q;
  double* tab = sm;
  double* lse = tab + Q * a.K;
  double* part = lse + g.G * Q;
  double* p = part + sm_part(g.G, a.K, Q);
  double* pbar = p + a.S * a.K;
  double* part3 = pbar + a.K;
  sm_stage(g.nodes, Q * a.K, tab);
  __syncthreads();
  sm_image_probs(a.mu, a.var, a.n, blockIdx.x, a.S, a.K, tab, Q, g.G, lse, part, p);
  unc_tail_finish(a, p, pbar, part3);
}

// The density objective's tail (input_grad.hip): J[n] = log pbar_n[y] with eval_tail's bits, (gm, gv) = d J[n] / d(mean, var) of the image's S rows:
//   d p_s[y] / d mu_k = 1/Q sum_q sig_q[y] ([k == y] - sig_q[k]),  d p_s[y] / d v_k = 1/Q sum_q sig_q[y] ([k == y] - sig_q[k]) e_q[k] / (2 s_k),
// stored unscaled by the group that formed them, then scaled by 1 / (S pbar_n[y]) once all S samples are in (rm_density_grad_kernel's order of
// events).  y is the clamped copy (labels_clamp_kernel).  sm: tab, lse [G Q], wy [G Q], part [2 G K chunks], ps [S], lab [G] (ints)
__global__ __launch_bounds__(256) void softmax_density_grad_kernel(SmImgArgs g, const double* __restrict__ mu, const double* __restrict__ var,
                                                                   const int32_t* __restrict__ y, int n_img, int S, int K, double* __restrict__ J,
                                                                   double* __restrict__ gm, double* __restrict__ gv) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ double coef;
  const int Q = g.Q, nc = sm_chunks(Q), G = g.G;
  double* tab = sm;
  double* lse = tab + Q * K;
  double* wy = lse + G * Q;
  double* part = wy + G * Q;
  double* ps = part + 2 * sm_part(G, K, Q);
  int* lab = (int*)(ps + S);
  const int n = blockIdx.x, tid = threadIdx.x;
  const int yi = y[n];
  sm_stage(g.nodes, Q * K, tab);
  if (tid < G) lab[tid] = yi;
  __syncthreads();
  for (int s0 = 0; s0 < S; s0 += G) {
    const int gr = min(G, S - s0);
    const long base = (long)s0 * n_img + n;
    sm_group_lse(mu, var, base, n_img, gr, K, tab, Q, lse, wy, lab);
    __syncthreads();
    // p_s[y]: sm_group_probs' sums for class y (chunks of 16 in index order, then the chunks)
    if (tid < gr) {
      double a = 0.0;
      for (int c = 0; c < nc; ++c) {
        const int q1 = min(Q, kSmChunk * (c + 1));
        double ac = 0.0;
        for (int q = kSmChunk * c; q < q1; ++q) ac += wy[tid * Q + q];
        a += ac;
      }
      ps[s0 + tid] = a / (double)Q;
    }
    sm_group_grad<true>(mu, var, base, n_img, gr, K, tab, Q, lse, wy, lab, part, [&](int rk, double A, double B) {
      const int r = rk / K, k = rk - r * K;
      const long o = (base + (long)r * n_img) * K + k;
      const double v = var[o];
      gm[o] = A / (double)Q;
      gv[o] = v > 1e-10 ? B / (double)Q / (2.0 * sm_sd(v)) : 0.0;
    });
    __syncthreads();
  }
  if (tid == 0) {
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += ps[s];
    if (J) J[n] = sm_logdens(ps, 1, S);
    coef = acc > 0.0 ? 1.0 / acc : 0.0;   // 1 / (S pbar); pbar underflowed to 0: J = -inf, and no direction is reported
  }
  __syncthreads();   // (also orders this workgroup's own stores to gm / gv in front of the loads below)
  const double c = coef;
  for (int idx = tid; idx < S * K; idx += 256) {
    const long o = ((long)(idx / K) * n_img + n) * K + idx % K;
    gm[o] *= c;
    gv[o] *= c;
  }
}

int sm_check(dcgp_ctx* ctx, int K, int Q, const char* who) {
  if (K < 2) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: the Softmax likelihood needs K >= 2 classes, got %d", who, K);
  if (Q < 1) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: the Softmax likelihood needs Q >= 1 nodes, got %d", who, Q);
  if ((long)Q * K > kSmMaxTable)
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: Q * K = %d * %d = %ld > %d (the node table's 32 KB of LDS)", who, Q, K, (long)Q * K, kSmMaxTable);
  return DCGP_OK;
}
int sm_check_lds(dcgp_ctx* ctx, long doubles, const char* who) {
  if (doubles <= kSmMaxLds) return DCGP_OK;
  return ctx_fail(ctx, DCGP_ERR_ARG, "%s: %ld doubles of LDS for the node table and the rows' sums, at most %d", who, doubles, kSmMaxLds);
}

SmRowsArgs sm_rows(const double* mu, const double* var, const int32_t* y, int n_rows, int n_labels, int K, const double* nodes, int Q) {
  SmRowsArgs a;
  a.mu = mu; a.var = var; a.y = y; a.n_rows = n_rows; a.n_labels = n_labels; a.K = K; a.nodes = nodes; a.Q = Q;
  a.G = sm_group_rows(K, Q, std::max(1, 256 / K));
  return a;
}

}  // namespace

int softmax_elbo_tail(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n_rows, int n_labels, int K, const double* nodes, int Q,
                      double* ve_rows, double inv_s, double* scal, const ElboFinish& fin, const KlTail* kl) {
  DCGP_TRY(sm_check(ctx, K, Q, "softmax"));
  TailArgs t;
  DCGP_TRY(elbo_tail_prepare(ctx, &t));   // (the same arrival counter as elbo_tail: the two never share a launch)
  t.n_rows = n_rows; t.ve = ve_rows; t.inv_s = inv_s; t.scal = scal; t.fin = fin;
  SmRowsArgs a = sm_rows(mu, var, y, n_rows, n_labels, K, nodes, Q);
  a.G = std::min(a.G, 32);
  const long lds = std::max((long)Q * K + (long)a.G * Q + 16L * a.G, 1024L);
  DCGP_TRY(sm_check_lds(ctx, lds, "softmax"));
  const int nb_rows = (n_rows + a.G - 1) / a.G;
  ScopedTimer tm(ctx, "softmax_tail");
  KlTail k;
  if (kl) k = *kl;
  hipLaunchKernelGGL(softmax_tail_kernel, dim3((unsigned)(nb_rows + k.nl)), dim3(256), (size_t)lds * sizeof(double), ctx->stream, a, t, k, nb_rows);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int softmax_grad(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int rows, int n_labels, int K, const double* nodes, int Q,
                 double weight, double* gm, double* gv) {
  DCGP_TRY(sm_check(ctx, K, Q, "softmax"));
  if (rows <= 0) return DCGP_OK;
  const SmRowsArgs a = sm_rows(mu, var, y, rows, n_labels, K, nodes, Q);
  const long lds = (long)Q * K + (long)a.G * Q + 2 * sm_part(a.G, K, Q) + (a.G + 1) / 2;
  DCGP_TRY(sm_check_lds(ctx, lds, "softmax"));
  ScopedTimer tm(ctx, "softmax_grad");
  hipLaunchKernelGGL(softmax_grad_kernel, dim3((unsigned)((rows + a.G - 1) / a.G)), dim3(256), (size_t)lds * sizeof(double), ctx->stream, a, weight, gm, gv);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int softmax_predict(dcgp_ctx* ctx, const double* mu, const double* var, int rows, int K, const double* nodes, int Q, double* out_mean, double* out_var) {
  DCGP_TRY(sm_check(ctx, K, Q, "softmax"));
  if (rows <= 0) return DCGP_OK;
  const SmRowsArgs a = sm_rows(mu, var, nullptr, rows, 1, K, nodes, Q);
  const long lds = (long)Q * K + (long)a.G * Q + sm_part(a.G, K, Q);
  DCGP_TRY(sm_check_lds(ctx, lds, "softmax"));
  hipLaunchKernelGGL(softmax_predict_kernel, dim3((unsigned)((rows + a.G - 1) / a.G)), dim3(256), (size_t)lds * sizeof(double), ctx->stream, a, out_mean, out_var);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int softmax_eval_tail(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n, int S, int K, const double* nodes, int Q, long lo,
                      double* logdens, double* p_mean, int* ok) {
  DCGP_TRY(sm_check(ctx, K, Q, "evaluate"));
  SmImgArgs g;
  g.nodes = nodes; g.Q = Q; g.G = sm_group_rows(K, Q, S);
  const long lds = (long)Q * K + (long)g.G * Q + sm_part(g.G, K, Q) + (long)S * K + K;
  if (lds > kSmMaxLds) return ctx_fail(ctx, DCGP_ERR_ARG, "evaluate: S = %d samples of %d classes at Q = %d nodes exceed the tail's LDS", S, K, Q);
  ScopedTimer tm(ctx, "softmax_eval_tail");
  hipLaunchKernelGGL(softmax_eval_tail_kernel, dim3((unsigned)n), dim3(kUncThreads), (size_t)lds * sizeof(double), ctx->stream, g, mu, var, y, n, S, K, lo,
                     logdens, p_mean, ok);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int softmax_unc_tail(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n, int S, int K, const double* nodes, int Q, long lo,
                     const UncOut& o) {
  DCGP_TRY(sm_check(ctx, K, Q, "evaluate_uncertainty"));
  SmImgArgs g;
  g.nodes = nodes; g.Q = Q; g.G = sm_group_rows(K, Q, S);
  const long lds = (long)Q * K + (long)g.G * Q + sm_part(g.G, K, Q) + (long)S * K + K + kUncExtraSlots;
  if (lds > kSmMaxLds)
    return ctx_fail(ctx, DCGP_ERR_ARG, "evaluate_uncertainty: S = %d samples of %d classes at Q = %d nodes exceed the tail's LDS", S, K, Q);
  UncTailArgs a;
  a.mu = mu; a.var = var; a.y = y; a.n = n; a.S = S; a.K = K; a.lo = lo;
  a.logdens = o.logdens; a.p_mean = o.p_mean; a.ok = o.ok; a.brier = o.brier;
  a.pred_ent = o.pred_ent; a.exp_ent = o.exp_ent; a.mi = o.mi; a.conf = o.conf; a.pred = o.pred;
  ScopedTimer tm(ctx, "softmax_unc_tail");
  hipLaunchKernelGGL(softmax_unc_tail_kernel, dim3((unsigned)n), dim3(kUncThreads), (size_t)lds * sizeof(double), ctx->stream, g, a);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int softmax_density_grad(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n_img, int S, int K, const double* nodes, int Q,
                         double* J, double* gm, double* gv) {
  DCGP_TRY(sm_check(ctx, K, Q, "input_grad"));
  SmImgArgs g;
  g.nodes = nodes; g.Q = Q; g.G = sm_group_rows(K, Q, std::min(S, 256));
  const long lds = (long)Q * K + 2L * g.G * Q + 2 * sm_part(g.G, K, Q) + S + (g.G + 1) / 2;
  if (lds > kSmMaxLds) return ctx_fail(ctx, DCGP_ERR_ARG, "input_grad: S = %d samples exceed the tail's LDS", S);
  hipLaunchKernelGGL(softmax_density_grad_kernel, dim3((unsigned)n_img), dim3(256), (size_t)lds * sizeof(double), ctx->stream, g, mu, var, y, n_img, S, K,
                     J, gm, gv);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// ---- the model's node table and the stand-alone entry points ------------------------------------------------------------------------------
extern "C" {

int dcgp_model_set_likelihood_nodes(dcgp_model* model, const double* nodes_host, int Q) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (model->lik_kind != 3) return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood_nodes: not a Softmax-likelihood model (dcgp_model_set_likelihood kind 3)");
  if (!nodes_host) return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood_nodes: nodes is NULL");
  if (model->enq_seq != model->col_seq) return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood_nodes: enqueued steps are still to be collected");
  const int K = model->layers.back()->R;
  DCGP_TRY(sm_check(ctx, K, Q, "set_likelihood_nodes"));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (no launch still reads the table this call replaces)
  const size_t count = (size_t)Q * K;
  if (count > model->nodes_cap) {
    double* fresh = nullptr;
    if (dev_alloc(ctx, (void**)&fresh, count * sizeof(double), "lik_nodes") != hipSuccess) return ctx_fail(ctx, DCGP_ERR_ALLOC, "set_likelihood_nodes: device allocation failed");
    dev_free(ctx, model->d_nodes);
    model->d_nodes = fresh;
    model->nodes_cap = count;
  }
  HIP_TRY(ctx, hipMemcpyAsync(model->d_nodes, nodes_host, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  model->lik_Q = Q;   // (no new parameter version: the factor chain does not depend on the table)
  return DCGP_OK;
}

int dcgp_softmax_varexp(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n, int K, const double* nodes, int Q, double* out_n) {
  if (!ctx) return DCGP_ERR_ARG;
  if (!mu || !var || !y || !nodes || !out_n || n <= 0) return ctx_fail(ctx, DCGP_ERR_ARG, "softmax_varexp: bad args");
  DCGP_TRY(sm_check(ctx, K, Q, "softmax_varexp"));
  SmRowsArgs a = sm_rows(mu, var, y, n, n, K, nodes, Q);
  a.G = std::min(a.G, 32);
  const long lds = (long)Q * K + (long)a.G * Q + 16L * a.G;
  DCGP_TRY(sm_check_lds(ctx, lds, "softmax_varexp"));
  int* bad = (int*)ws_get(ctx, "softmax_bad", sizeof(int));
  if (!bad) return DCGP_ERR_ALLOC;
  hipLaunchKernelGGL(softmax_varexp_kernel, dim3((unsigned)((n + a.G - 1) / a.G)), dim3(256), (size_t)lds * sizeof(double), ctx->stream, a, out_n, bad);
  LAUNCH_CHECK(ctx);
  int h = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&h, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h > 0) return ctx_fail(ctx, DCGP_ERR_ARG, "softmax_varexp: %d labels outside [0, %d)", h, K);
  return DCGP_OK;
}

int dcgp_softmax_predict(dcgp_ctx* ctx, const double* mu, const double* var, int n, int K, const double* nodes, int Q, double* out_p) {
  if (!ctx) return DCGP_ERR_ARG;
  if (!mu || !var || !nodes || !out_p || n <= 0) return ctx_fail(ctx, DCGP_ERR_ARG, "softmax_predict: bad args");
  DCGP_TRY(softmax_predict(ctx, mu, var, n, K, nodes, Q, out_p, nullptr));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

}  // extern "C"

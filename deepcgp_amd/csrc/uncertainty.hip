// uncertainty.hip -- the uncertainty tails of a test-set batch and the calibration sums behind the last batch: what DS-DGP's
// DGP_Base.predict_y leaves to its caller (the S samples of the class probabilities) reduced on the device to the predictive entropy,
// its expected-entropy / mutual-information (BALD) split, the confidence and the reliability table of the sample-mean prediction.
//
//   p[s][k]   the per-sample probabilities of eval_tail_kernel (RobustMax) / quad_eval_tail_kernel<BernoulliDensity> (jittered probit), term for term
//   pbar      their mean, summed in sample order
//   H(pbar) = -sum_k pbar[k] log pbar[k]                    predictive entropy      (Bernoulli: the binary entropy h(pbar) per output)
//   E H     = 1/S sum_s -sum_k p[s][k] log p[s][k]          expected entropy
//   I       = H(pbar) - E H                                 mutual information, the raw difference (not clipped)
//   confidence = max_k pbar[k] (Bernoulli: max(pbar, 1 - pbar)), prediction = its first index (Bernoulli: pbar > 0.5)
// Every probability is >= eps / (K - 1) or 1e-3 by construction: no clamp is added here, every log is finite.
//
// Sums run in a fixed order (index order per thread, a xor-shuffle tree per wave, the waves in index order; in the dataset kernel
// eval_sum_kernel's strides and tree), and nothing is accumulated with atomics: two calls agree bit for bit.
#include "layer_impl.h"
#include "tail_dev.h"
#include "unc_dev.h"
#include "pointwise_dev.h"

namespace {

// One workgroup per image, eval_tail_kernel's geometry: the probabilities are its statements, so pbar, the log density and ok come out
// with its bits.  Everything behind the probabilities is unc_tail_finish (unc_dev.h), shared with the Softmax tail.
__global__ __launch_bounds__(kUncThreads) void unc_tail_kernel(UncTailArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* p = sm;                    // [S][K]
  double* pbar = sm + a.S * a.K;     // [K]
  double* part = pbar + a.K;         // [3][16] wave partials
  const int i = blockIdx.x, tid = threadIdx.x, g = tid & 31;
  const int SK = a.S * a.K;
  for (int base = 0; base < SK; base += kUncThreads / 32) {   // (uniform trip count: every lane of the workgroup takes part in the shuffles)
    const int slot = base + (tid >> 5);
    const bool live = slot < SK;
    const int s = live ? slot / a.K : 0, k = live ? slot - s * a.K : 0;
    const long row = (long)s * a.n + i;
    double contrib = live ? robustmax_node(a.mu + row * a.K, a.var + row * a.K, k, a.K, a.gh, g) : 0.0;
    for (int o = 1; o < 32; o <<= 1) contrib += __shfl_xor(contrib, o);
    if (live && g == 0) p[slot] = contrib * (1.0 - a.eps) + (1.0 - contrib) * (a.eps / (a.K - 1.0));
  }
  __syncthreads();
  unc_tail_finish(a, p, pbar, part);
}

__device__ __forceinline__ double binary_entropy(double q) { return -q * log(q) - (1.0 - q) * log(1.0 - q); }

struct BernUncArgs {
  const double* mu = nullptr; const double* var = nullptr;   // [S*n][K], row s*n + i
  const double* y = nullptr;                                  // [n][K] targets of the batch, or nullptr
  int n = 0, S = 0, K = 0;
  long lo = 0;
  double* logdens = nullptr;                                  // [N_total], summed over the K outputs    (labels only)
  double* p_mean = nullptr;                                   // [N_total][K] or nullptr
  int* ok = nullptr; double* brier = nullptr;                 // [N_total][K]: label == prediction, (pbar - y)^2   (labels only)
  double* pred_ent = nullptr; double* mi = nullptr; double* conf = nullptr;   // [N_total][K]
  double* exp_ent = nullptr;                                  // [N_total][K] or nullptr
  int* pred = nullptr;                                        // [N_total][K]
};

// The Bernoulli counterpart with quad_eval_tail_kernel's geometry: one thread per image, its K outputs and their S samples in index
// order -- the per-image log density is that kernel's sum over the outputs, statement for statement.
__global__ __launch_bounds__(256) void bern_unc_tail_kernel(BernUncArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const long gi = a.lo + i;
  double ld = 0.0;
  for (int d = 0; d < a.K; ++d) {
    const bool pos = a.y ? a.y[(long)i * a.K + d] == 1.0 : false;
    double mx = -__builtin_inf(), psum = 0.0, esum = 0.0;
    for (int s = 0; s < a.S; ++s) {
      const long r = ((long)s * a.n + i) * a.K + d;
      const double p = probit(a.mu[r] / sqrt(1.0 + a.var[r]));
      mx = fmax(mx, bern_logp(p, pos));
      psum += p;
      esum += binary_entropy(p);
    }
    const double pm = psum / (double)a.S;
    const long ge = gi * a.K + d;
    if (a.p_mean) a.p_mean[ge] = pm;
    const double h = binary_entropy(pm), e = esum / (double)a.S;
    a.pred_ent[ge] = h;
    if (a.exp_ent) a.exp_ent[ge] = e;
    a.mi[ge] = h - e;
    a.conf[ge] = fmax(pm, 1.0 - pm);
    a.pred[ge] = pm > 0.5 ? 1 : 0;
    if (!a.y) continue;
    double acc = 0.0;
    for (int s = 0; s < a.S; ++s) {
      const long r = ((long)s * a.n + i) * a.K + d;
      acc += exp(bern_logp(probit(a.mu[r] / sqrt(1.0 + a.var[r])), pos) - mx);
    }
    ld += mx + log(acc) - log((double)a.S);
    const double res = pm - (pos ? 1.0 : 0.0);
    a.brier[ge] = res * res;
    a.ok[ge] = (pm > 0.5) == pos ? 1 : 0;
  }
  if (a.y) a.logdens[gi] = ld;
}

// One workgroup behind the last batch.  Over the n_img images the sum of the log densities, over the n_ent entries (images; Bernoulli:
// (image, output) pairs) the correct and out-of-range counts and the sums of the Brier terms, the predictive entropies and the mutual
// informations: eval_sum_kernel's order (strided per thread, then a tree).  The reliability table [bins][3] = {count, sum of
// confidences, correct count}: wave w owns bins w, w + 16, ..; its lane l adds the entries l, l + 64, .. that fall into the bin in
// index order, then a xor-shuffle tree.  Thread 0 then reads the table back for ECE and MCE.
// res[9] = {correct, sum of log densities, first non-positive pivot, labels outside [0, K), ECE, MCE, Brier score, mean predictive
// entropy, mean mutual information}; without labels (ok == nullptr) words 0, 1, 4, 5, 6 are NaN.
__global__ __launch_bounds__(1024) void unc_sum_kernel(UncSumArgs a, FactorStatus st, double* __restrict__ res) {
  __shared__ double red[6][1024];
  const int tid = threadIdx.x;
  double s = 0.0, c = 0.0, bad = 0.0, br = 0.0, pe = 0.0, mi = 0.0;
  if (a.ok)
    for (long i = tid; i < a.n_img; i += 1024) s += a.logdens[i];
  for (long i = tid; i < a.n_ent; i += 1024) {
    if (a.ok) {
      const int o = a.ok[i];
      c += o > 0 ? 1.0 : 0.0;
      bad += o < 0 ? 1.0 : 0.0;
      br += a.brier[i];
    }
    pe += a.pred_ent[i];
    mi += a.mi[i];
  }
  red[0][tid] = c; red[1][tid] = s; red[2][tid] = bad; red[3][tid] = br; red[4][tid] = pe; red[5][tid] = mi;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o)
      for (int q = 0; q < 6; ++q) red[q][tid] += red[q][tid + o];
    __syncthreads();
  }
  const int lane = tid & 63;
  for (int b = tid >> 6; b < a.bins; b += 16) {
    double cnt = 0.0, sf = 0.0, sc = 0.0;
    for (long i = lane; i < a.n_ent; i += 64) {
      const double f = a.conf[i];
      const int bi = min(a.bins - 1, (int)floor(f * (double)a.bins));
      if (bi != b) continue;
      cnt += 1.0;
      sf += f;
      if (a.ok) sc += a.ok[i] > 0 ? 1.0 : 0.0;
    }
    cnt = wave_sum(cnt); sf = wave_sum(sf); sc = wave_sum(sc);
    if (lane == 0) { a.table[3 * b] = cnt; a.table[3 * b + 1] = sf; a.table[3 * b + 2] = sc; }
  }
  __syncthreads();   // (the table's words are this workgroup's own stores)
  if (tid != 0) return;
  const int pivot = first_bad_pivot(st);
  const double n = (double)a.n_ent, nan = __builtin_nan("");
  double ece = 0.0, mce = 0.0;
  for (int b = 0; b < a.bins; ++b) {
    const double cnt = a.table[3 * b];
    if (cnt == 0.0) continue;
    const double gap = fabs(a.table[3 * b + 2] / cnt - a.table[3 * b + 1] / cnt);   // |accuracy - mean confidence| of the bin
    ece += (cnt / n) * gap;
    mce = fmax(mce, gap);
  }
  res[0] = a.ok ? red[0][0] : nan;
  res[1] = a.ok ? red[1][0] : nan;
  res[2] = (double)pivot;
  res[3] = red[2][0];
  res[4] = a.ok ? ece : nan;
  res[5] = a.ok ? mce : nan;
  res[6] = a.ok ? red[3][0] / n : nan;
  res[7] = red[4][0] / n;
  res[8] = red[5][0] / n;
}

}  // namespace

int unc_tail(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n, int S, int K, double eps, long lo,
             const UncOut& o) {
  static_assert(kUncExtraSlots == 3 * kUncWaves, "three sums per wave");
  if ((long)S * K + K + kUncExtraSlots > kEvalMaxSlots)
    return ctx_fail(ctx, DCGP_ERR_ARG, "evaluate_uncertainty: S * K + K + %d = %ld > %d", kUncExtraSlots, (long)S * K + K + kUncExtraSlots, kEvalMaxSlots);
  const double* gh = gauss_hermite_table(ctx);
  if (!gh) return DCGP_ERR_ALLOC;
  UncTailArgs a;
  a.mu = mu; a.var = var; a.y = y; a.n = n; a.S = S; a.K = K; a.eps = eps; a.gh = gh; a.lo = lo;
  a.logdens = o.logdens; a.p_mean = o.p_mean; a.ok = o.ok; a.brier = o.brier;
  a.pred_ent = o.pred_ent; a.exp_ent = o.exp_ent; a.mi = o.mi; a.conf = o.conf; a.pred = o.pred;
  ScopedTimer tm(ctx, "unc_tail");
  const size_t lds = (size_t)(S * K + K + kUncExtraSlots) * sizeof(double);
  hipLaunchKernelGGL(unc_tail_kernel, dim3((unsigned)n), dim3(kUncThreads), lds, ctx->stream, a);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int bern_unc_tail(dcgp_ctx* ctx, const double* mu, const double* var, const double* y, int n, int S, int K, long lo, const UncOut& o) {
  BernUncArgs a;
  a.mu = mu; a.var = var; a.y = y; a.n = n; a.S = S; a.K = K; a.lo = lo;
  a.logdens = o.logdens; a.p_mean = o.p_mean; a.ok = o.ok; a.brier = o.brier;
  a.pred_ent = o.pred_ent; a.exp_ent = o.exp_ent; a.mi = o.mi; a.conf = o.conf; a.pred = o.pred;
  ScopedTimer tm(ctx, "bern_unc_tail");
  hipLaunchKernelGGL(bern_unc_tail_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, a);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int unc_sum(dcgp_ctx* ctx, const UncSumArgs& a, const FactorStatus& st, double* res) {
  hipLaunchKernelGGL(unc_sum_kernel, dim3(1), dim3(1024), 0, ctx->stream, a, st, res);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

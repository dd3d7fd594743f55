// evaluate.hip -- the evaluation tail of a test-set batch (doubly_stochastic_dgp DGP_Base.predict_density with the RobustMax
// likelihood; the arg-max of conv_gp/utils/log.py:62-67) and the dataset sums behind the last batch.
//
// One launch per batch reads the head's mean / var rows [S*n][K] that forward_all leaves in model->outs and writes, per image,
// the log predictive density, the sample-mean class probabilities and whether their arg-max is the label, at the image's index in
// the whole set.  Nothing comes back to the host between batches; one small launch behind the last batch adds the per-image
// values up in a fixed order (model.hip: dcgp_model_evaluate).
#include "layer_impl.h"
#include "tail_dev.h"

namespace {

struct EvalTailArgs {
  const double* mu = nullptr; const double* var = nullptr;   // [S*n][K], row s*n + i
  const int32_t* y = nullptr;                                 // [n] labels of the batch
  int n = 0, S = 0, K = 0;
  double eps = 0.0;
  const double* gh = nullptr;                                 // [40] Gauss-Hermite nodes, weights
  long lo = 0;                                                // the batch's first image in the whole set
  double* logdens = nullptr;                                  // [N_total]
  double* p_mean = nullptr;                                   // [N_total][K] or nullptr
  int* ok = nullptr;                                          // [N_total]: 1 arg-max == label, 0 not, -1 label outside [0, K)
};

// 32 (sample, class) slots per pass; a pass is one dependent chain of K - 1 erf's, so S K = 50 slots take two.  A batch of 32 images
// at S = 5 (cfg2): 24 us with 1024 threads, 37.7 us with 256 (seven passes) -- 32 workgroups on 256 CUs, latency-bound either way.
constexpr int kEvalThreads = 1024;

// One workgroup per image.  The class probabilities p[s][k] are varexp_kernel's predict mode (cond.hip) slot for slot: 32 lanes per
// (sample, class), the same node terms (robustmax_node), the same shuffle-sum order and the same epsilon mix -- so that the sample mean
// below is bit-identical to dcgp_model_predict_y's out_p_mean (sample_mean_kernel, model.hip).
__global__ __launch_bounds__(kEvalThreads) void eval_tail_kernel(EvalTailArgs a) {
  extern __shared__ double sm[];
  double* p = sm;                    // [S][K]
  double* pbar = sm + a.S * a.K;     // [K]
  const int i = blockIdx.x, tid = threadIdx.x, g = tid & 31;
  const int SK = a.S * a.K;
  for (int base = 0; base < SK; base += kEvalThreads / 32) {   // (uniform trip count: every lane of the workgroup takes part in the shuffles)
    const int slot = base + (tid >> 5);
    const bool live = slot < SK;
    const int s = live ? slot / a.K : 0, k = live ? slot - s * a.K : 0;
    const long row = (long)s * a.n + i;
    double contrib = live ? robustmax_node(a.mu + row * a.K, a.var + row * a.K, k, a.K, a.gh, g) : 0.0;
    for (int o = 1; o < 32; o <<= 1) contrib += __shfl_xor(contrib, o);
    if (live && g == 0) p[slot] = contrib * (1.0 - a.eps) + (1.0 - contrib) * (a.eps / (a.K - 1.0));
  }
  __syncthreads();
  const long gi = a.lo + i;
  for (int k = tid; k < a.K; k += kEvalThreads) {
    double acc = 0.0;
    for (int s = 0; s < a.S; ++s) acc += p[s * a.K + k];
    pbar[k] = acc / (double)a.S;
    if (a.p_mean) a.p_mean[gi * a.K + k] = pbar[k];
  }
  __syncthreads();
  if (tid != 0) return;
  const int yi = a.y[i];
  if (yi < 0 || yi >= a.K) {   // reported by the sum kernel as an argument error; nothing is read at the label
    a.logdens[gi] = __builtin_nan("");
    a.ok[gi] = -1;
    return;
  }
  // log (1/S sum_s p[s][y]) = max_s l_s + log sum_s exp(l_s - max) - log S,  l_s = log p[s][y]  (DS-DGP: reduce_logsumexp(l - log S))
  double mx = -__builtin_inf();
  for (int s = 0; s < a.S; ++s) mx = fmax(mx, log(p[s * a.K + yi]));
  double se = 0.0;
  for (int s = 0; s < a.S; ++s) se += exp(log(p[s * a.K + yi]) - mx);
  a.logdens[gi] = mx + log(se) - log((double)a.S);
  int best = 0;   // first index of the largest: numpy's argmax on ties
  for (int k = 1; k < a.K; ++k)
    if (pbar[k] > pbar[best]) best = k;
  a.ok[gi] = best == yi ? 1 : 0;
}

// One workgroup: res[0] = number of correct arg-maxes, res[1] = sum of the log densities (strided per thread, then a tree: the same
// order from run to run), res[2] = first non-positive pivot of the factorisations the batches used (0: none), res[3] = labels
// outside [0, K).
__global__ __launch_bounds__(1024) void eval_sum_kernel(const double* __restrict__ logdens, const int* __restrict__ ok, long n,
                                                        FactorStatus st, double* __restrict__ res) {
  __shared__ double red[3][1024];
  const int tid = threadIdx.x;
  double s = 0.0, c = 0.0, bad = 0.0;
  for (long i = tid; i < n; i += 1024) {
    s += logdens[i];
    const int o = ok[i];
    c += o > 0 ? 1.0 : 0.0;
    bad += o < 0 ? 1.0 : 0.0;
  }
  red[0][tid] = c; red[1][tid] = s; red[2][tid] = bad;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o)
      for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + o];
    __syncthreads();
  }
  if (tid != 0) return;
  const int pivot = first_bad_pivot(st);
  res[0] = red[0][0];
  res[1] = red[1][0];
  res[2] = (double)pivot;
  res[3] = red[2][0];
}

}  // namespace

int eval_tail(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n, int S, int K, double eps, long lo,
              double* logdens, double* p_mean, int* ok) {
  if ((long)S * K + K > kEvalMaxSlots) return ctx_fail(ctx, DCGP_ERR_ARG, "evaluate: S * K + K = %ld > %d", (long)S * K + K, kEvalMaxSlots);
  const double* gh = gauss_hermite_table(ctx);
  if (!gh) return DCGP_ERR_ALLOC;
  EvalTailArgs a;
  a.mu = mu; a.var = var; a.y = y; a.n = n; a.S = S; a.K = K; a.eps = eps; a.gh = gh; a.lo = lo;
  a.logdens = logdens; a.p_mean = p_mean; a.ok = ok;
  ScopedTimer tm(ctx, "eval_tail");
  const size_t lds = (size_t)(S * K + K) * sizeof(double);
  hipLaunchKernelGGL(eval_tail_kernel, dim3((unsigned)n), dim3(kEvalThreads), lds, ctx->stream, a);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

int eval_sum(dcgp_ctx* ctx, const double* logdens, const int* ok, long n, const FactorStatus& st, double* res) {
  hipLaunchKernelGGL(eval_sum_kernel, dim3(1), dim3(1024), 0, ctx->stream, logdens, ok, n, st, res);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

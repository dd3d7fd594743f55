// unc_dev.h -- what the uncertainty tails of the label likelihoods share (uncertainty.hip: RobustMax, softmax.hip: Softmax): the launch
// geometry, the argument block and everything behind the per-sample class probabilities p[s][k] -- their mean, the entropies, the Brier
// term, the confidence, the prediction and the log density.  Only how p is filled differs between the two likelihoods.
#pragma once
#include "layer.h"

constexpr int kUncThreads = 1024, kUncWaves = kUncThreads / 64;

struct UncTailArgs {
  const double* mu = nullptr; const double* var = nullptr;   // [S*n][K], row s*n + i
  const int32_t* y = nullptr;                                 // [n] labels of the batch, or nullptr: no density, ok, Brier term
  int n = 0, S = 0, K = 0;
  double eps = 0.0;
  const double* gh = nullptr;                                 // [40] Gauss-Hermite nodes, weights
  long lo = 0;                                                // the batch's first image in the whole set
  double* logdens = nullptr;                                  // [N_total]                       (labels only)
  double* p_mean = nullptr;                                   // [N_total][K] or nullptr
  int* ok = nullptr;                                          // [N_total]: 1 / 0 / -1 as eval_tail  (labels only)
  double* brier = nullptr;                                    // [N_total] sum_k (pbar[k] - [y == k])^2   (labels only)
  double* pred_ent = nullptr; double* mi = nullptr; double* conf = nullptr;   // [N_total]
  double* exp_ent = nullptr;                                  // [N_total] or nullptr
  int* pred = nullptr;                                        // [N_total]
};

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// The workgroup of image i = blockIdx.x (kUncThreads threads), behind the barrier that follows the last store to p [S][K] (LDS): pbar [K]
// and part [3][16] are LDS.  The sample mean in sample order, then every thread takes the slots tid, tid + 1024, .. of -p log p, thread
// k < K the class's -pbar log pbar and squared Brier residual; three wave sums and one pass over the 16 wave partials finish them.
__device__ __forceinline__ void unc_tail_finish(const UncTailArgs& a, const double* p, double* pbar, double* part) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const int SK = a.S * a.K;
  const long gi = a.lo + i;
  for (int k = tid; k < a.K; k += kUncThreads) {
    double acc = 0.0;
    for (int s = 0; s < a.S; ++s) acc += p[s * a.K + k];
    pbar[k] = acc / (double)a.S;
    if (a.p_mean) a.p_mean[gi * a.K + k] = pbar[k];
  }
  __syncthreads();
  const int yi = a.y ? a.y[i] : -1;
  const bool labelled = a.y && yi >= 0 && yi < a.K;
  double e = 0.0, h = 0.0, b = 0.0;
  for (int slot = tid; slot < SK; slot += kUncThreads) e -= p[slot] * log(p[slot]);
  for (int k = tid; k < a.K; k += kUncThreads) {
    h -= pbar[k] * log(pbar[k]);
    const double r = pbar[k] - (k == yi ? 1.0 : 0.0);
    b += r * r;
  }
  e = wave_sum(e); h = wave_sum(h); b = wave_sum(b);
  if ((tid & 63) == 0) { part[tid >> 6] = e; part[kUncWaves + (tid >> 6)] = h; part[2 * kUncWaves + (tid >> 6)] = b; }
  __syncthreads();
  if (tid != 0) return;
  e = h = b = 0.0;
  for (int w = 0; w < kUncWaves; ++w) { e += part[w]; h += part[kUncWaves + w]; b += part[2 * kUncWaves + w]; }
  e /= (double)a.S;
  int best = 0;   // first index of the largest: numpy's argmax on ties
  for (int k = 1; k < a.K; ++k)
    if (pbar[k] > pbar[best]) best = k;
  a.pred_ent[gi] = h;
  if (a.exp_ent) a.exp_ent[gi] = e;
  a.mi[gi] = h - e;
  a.conf[gi] = pbar[best];
  a.pred[gi] = best;
  if (!a.y) return;
  if (!labelled) {   // reported by the sum kernel as an argument error; nothing is read at the label
    a.logdens[gi] = __builtin_nan("");
    a.brier[gi] = __builtin_nan("");
    a.ok[gi] = -1;
    return;
  }
  // log (1/S sum_s p[s][y]) = max_s l_s + log sum_s exp(l_s - max) - log S,  l_s = log p[s][y]  (eval_tail_kernel's statements)
  double mx = -__builtin_inf();
  for (int s = 0; s < a.S; ++s) mx = fmax(mx, log(p[s * a.K + yi]));
  double se = 0.0;
  for (int s = 0; s < a.S; ++s) se += exp(log(p[s * a.K + yi]) - mx);
  a.logdens[gi] = mx + log(se) - log((double)a.S);
  a.brier[gi] = b;
  a.ok[gi] = best == yi ? 1 : 0;
}

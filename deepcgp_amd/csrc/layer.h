// Internal: device-resident state of one GP layer and the shared forward building blocks.
#pragma once
#include "common.h"
#include "rng.h"

// Geometry of a patch view (FullView, conv_gp/views.py:20-30,56-68)
struct ViewGeom {
  int H = 0, W = 0, C = 0, f = 0, s = 0, Ho = 0, Wo = 0, P = 0, L = 0;
  void set(int H_, int W_, int C_, int f_, int s_) {
    H = H_; W = W_; C = C_; f = f_; s = s_;
    Ho = (H - f) / s + 1; Wo = (W - f) / s + 1; P = Ho * Wo; L = f * f * C;
  }
};

// Padded M x M operands of one layer ([Mp x Mp], ld = Mp) living in device memory.
struct GpMats {
  int M = 0, Mp = 0, R = 0, Rp = 0;   // Rp = R rounded up to 16 (column padding of qmu)
  double* K = nullptr;      // Kuu (live Z) -> overwritten by its Cholesky factor L
  double* Linv = nullptr;   // inv(L)
  double* LinvT = nullptr;  // inv(L)^T
  double* Kp = nullptr;     // prior Kuu(Z0) -> its factor (conv layers, non-white); may alias K
  double* Lpinv = nullptr;
  double* LpinvT = nullptr;
  double* Lq = nullptr;     // [R][Mp][Mp] lower-masked q_sqrt, zero padded
  double* qmu = nullptr;    // [Mp][Rp], zero padded rows and columns
  // derived by cond_prep after the factorisation (alias Lq / qmu in the whitened case):
  double* G = nullptr;      // [R][Mp][Mp]  G_r = inv(L) Lq_r   (lower triangular)
  double* alpha = nullptr;  // [Mp][Rp]     alpha = inv(L) q_mu
  double* klp = nullptr;    // [(R + 1)][Mp / 16] sums of squares of the 16-column strips of G_r and (row R, entry 0) of alpha,
                            // left by prep_solve: the KL's trace and Mahalanobis terms when its prior factor is L itself
  bool klp_valid = false;   // set by prep_solve_all for the launch that filled klp
  double* klpp = nullptr;   // the same sums with the PRIOR factor inv(Lp) in place of inv(L) (layers with a prior Kuu(Z0)): nothing
                            // but the sums is kept of those products
  bool klpp_valid = false;
  int kl_ns = 0, kl_nsa = 0;   // layout of klp / klpp: 0 = prep_solve's 16-column strips ([(R + 1)][Mp / 16], one alpha entry); else [(R + 1)][kl_ns] with
                               // kl_nsa alpha entries (the right-hand sides rode the factorisation chain: chain_rhs_slots)
  // M > 256 (cond_prep's generic GEMMs): the same column sums of squares, per row block, from the G / alpha products' epilogues
  double* prep_tp = nullptr; long prep_tp_count = 0;   // [R][nrb][Mp] sums of squares of G
  double* prep_ap = nullptr; long prep_ap_count = 0;   // [nrb][Rp] of alpha
  bool prep_sums_valid = false;
};

// parameter-only preparation of all layers in one launch (prep.hip)
struct PrepLayerArgs {
  const double *Z = nullptr, *Z0 = nullptr, *q_sqrt = nullptr, *q_mu = nullptr;
  double *K = nullptr, *Kp = nullptr, *ZT = nullptr, *zn = nullptr, *Lq = nullptr, *qmu = nullptr;
  int M = 0, Mp = 0, L = 0, Lp = 0, R = 0, Rp = 0;
  BaseKernel bk; double jitter = 0.0;
  const double* in_scale = nullptr;   // [L] or nullptr: Z is read as Z * in_scale (ARD lengthscales)
  double* ZS = nullptr; int Lz = 0;   // the sweeps' scaled operand (sweep_dev.h); nullptr: not an RBF layer
};
struct PrepArgs {
  int nl = 0;
  PrepLayerArgs l[8];
};
// task_mask: bit t = task t of prep.hip (0 / 1: Kuu of the live / prior Z, 2: Z^T and |z|^2, 3: masked q_sqrt, 4: padded q_mu, 5: the sweeps' scaled Z)
constexpr unsigned kPrepSweepTasks = (1u << 2) | (1u << 5);   // what a patch sweep reads
int prepare_all(dcgp_ctx* ctx, const PrepArgs& a, unsigned task_mask = ~0u);

// A = inv(L) Kuf etc. on a k-major Kuf matrix B [Mp x ldb] with Kc columns.
// Produces partial column sums s1p [nrb1][ldb], s2p [R][nrb3][ldb], and mu [R][ldb].
struct CondScratch {
  double *A1 = nullptr, *s1p = nullptr, *s2p = nullptr, *mu = nullptr;
  int nrb1 = 0, nrb3 = 0;
  long ldb = 0;
};
// G and alpha of a layer (two small GEMMs on the current stream); must run after the factorisation of g.K
int cond_prep(dcgp_ctx* ctx, GpMats& g, int white, bool have_qsqrt);
int cond_core(dcgp_ctx* ctx, const GpMats& g, const double* B, long ldb, int Kc, int white, bool have_qsqrt,
              const char* ws_prefix, CondScratch* out, hipEvent_t prep_done = nullptr, bool head = false);   // head: timer labels only

// KL pieces offered to the head's one-launch conditional (an ELBO step whose chain left their ingredients, model.hip): head_cond_fused carries them as extra
// workgroups of its launch where that pays and sets `carried`; a head on another route leaves them to the tail launch
struct KlTail;
struct KlOffer { const KlTail* tail = nullptr; double* scal = nullptr; bool carried = false; };
// head_cond.hip: the whole conditional of a few-column problem in one launch (M <= 256): mean / var [Kc][R]
bool head_cond_fused_ok(const GpMats& g);
int head_cond_fused(dcgp_ctx* ctx, const GpMats& g, const double* B, long ldb, int Kc, bool have_qsqrt, const double* kd,
                    double* out_mean, double* out_var, int kd_n = 1, double kd_scale = 1.0, double* A1_out = nullptr, long lda1 = 0, KlOffer* kl = nullptr);   // Knn[j] = kd_scale * sum_{i < kd_n} kd[j * kd_n + i]

// head_cond.hip: G / alpha of every layer in one launch; done[i] = false where layer i still needs cond_prep
int prep_solve_all(dcgp_ctx* ctx, GpMats* const* gs, const int* white, const bool* have_qsqrt, int nl, bool* done, const bool* skip = nullptr);

struct FinalizeArgs {
  const double* s1p = nullptr; int nrb1 = 0;
  const double* s2p = nullptr; int nrb3 = 0;    // nullptr -> no q_sqrt term
  const double* mu = nullptr;
  long ldk = 0;                  // leading dimension (padded column count) of the above
  int Kc = 0, R = 0;
  long col0 = 0;                 // first column of a chunk: outputs, noise and the identity mean are indexed by col0 + j
  double knn_scalar = 0.0; const double* knn_vec = nullptr;   // Knn per column (vector wins if set)
  // output: element (j, r) of replica s at  s*rep_stride + j*R + r
  int rep = 1; long rep_stride = 0;
  const double* z = nullptr;     // same indexing as the output; nullptr + want sample -> device RNG
  uint64_t seed = 0; uint32_t stream_id = 0;
  RngMap rmap;                    // device RNG: the element's counter in the un-sharded batch
  double jitter = 0.0;
  double *out_sample = nullptr, *out_mean = nullptr, *out_var = nullptr;
  // Conv2dMean (conv_gp/mean_functions.py:28-41): adds the centre pixel of channel 0 to map r == 0
  const double* X = nullptr; int idm = 0; int n_mod = 0; int H = 0, W = 0, C = 0, f = 0, s = 0, Wo = 0, P = 0;
};
int finalize_layer(dcgp_ctx* ctx, const FinalizeArgs& a);

// conv_fused.hip: the whole conv layer (patch sweep, both triangular products, mean, var, sample) of a column strip in one
// workgroup; K_uf and A1 never leave the chip unless the training step asks for them
struct ConvFusedArgs {
  const double* X = nullptr; int n_mod = 0;               // [n_mod, H, W, C]; image of row n is X[n % n_mod]
  int H = 0, W = 0, C = 0, f = 0, s = 0, Wo = 0, P = 0, L = 0, Lp = 0, HWC = 0;
  const double* ZT = nullptr; const double* zn = nullptr; int M = 0, Mp = 0;
  const double* ZS = nullptr; int Lz = 0; double csq = 1.0;   // RBF: the sweep's scaled operand [Lz][Mp] and image scale sqrt(c) (sweep_dev.h)
  BaseKernel bk;
  const double* LinvT = nullptr;                           // [Mp][Mp]
  const double* G = nullptr;                               // [R][Mp][Mp] or nullptr (no q_sqrt term)
  const double* alpha = nullptr; int R = 0, Rp = 0;        // [Mp][Rp]
  int Kc = 0;                                              // columns = rows * P
  double knn = 0.0;
  int rep = 1; long rep_stride = 0;
  const double* z = nullptr; uint64_t seed = 0; uint32_t stream_id = 0; double jitter = 0.0;
  RngMap rmap;                                             // device RNG: the element's counter in the un-sharded batch
  double *out_sample = nullptr, *out_mean = nullptr, *out_var = nullptr;
  int idm = 0;
  double *Kuf_out = nullptr, *A1_out = nullptr; long ldk = 0;   // training step: k-major [Mp][ldk] copies for the reverse pass
  int lds_main = 0, lds_img = 0;                           // set by the launcher
  float inv_HWC = 0, inv_nmod = 0, inv_P = 0, inv_Wo = 0, inv_R = 0;   // set by the launcher: reciprocals of the kernel's divisors (fdiv)
  int split_first = 1 << 30, split_q = 1;                  // set by the launcher: strips >= split_first are shared by split_q workgroups (outputs r = q, q + split_q, ...)
  long long* trace = nullptr;                              // debugging aid: phase timestamps (dcgp_debug_set_fused_trace)
  // set by the launcher: a persistent launch -- one workgroup per slot of the chip, each walking the strips blockIdx, blockIdx + grid, ... < n_strips
  int persist = 0, n_strips = 0;
  int stagger = 0;                                         // the second workgroup to arrive on a CU starts this many 100 MHz ticks late
  int* dyn = nullptr;                                      // [2] {strips dealt beyond the first of every workgroup, workgroups that have left}: zero between launches
  int* cu_slots = nullptr;                                 // [1024] arrival counters per CU (zero between launches: every workgroup gives its count back)
  // set by the launcher: prologues ahead (conv_fused.hip) -- pre_n strips from pre_first on get phases 0 - 2 from the spare workgroups of the partial FIRST
  // round, A1 handed over through pre_buf ([pre_n][pre_stride]: the strip's LDS image, then the partial sums of A1^2) behind pre_flag[slot] == pre_epoch
  // pre_sq > 1 (a launch of few strips, all of them handed over: pre_first = 0, pre_n = n_strips): a handed-over strip is taken up by pre_sq items, part q
  // running the outputs r = q, q + pre_sq, ... of the second product
  int no_rows = 0;                                         // set by the launcher (ctx option sweep_no_rows): 5 x 5 x 10 patches on the generic in-kernel sweep (A/B)
  int pre_n = 0, pre_first = 0, pre_sq = 1; long pre_stride = 0;
  double* pre_buf = nullptr; unsigned* pre_flag = nullptr; unsigned pre_epoch = 0;
  // set by the launcher: items the counter deals in a persistent launch (n_strips + pre_n * pre_sq; n_strips where replicas share a prologue)
  int n_items = 0;
  // set by the launcher: replicas share a prologue (conv_fused.hip) -- the rows are n_mod images tiled and n_mod * P columns are pre_D whole strips: strip i < pre_D
  // runs whole and leaves A1 in slot i (pre_n = pre_D slots), strips in [pre_D, pre_whole) run whole, strip i >= pre_whole fetches slot i % pre_D
  int pre_D = 0, pre_whole = 0;
  // head rows riding the launch (fused_plan.h: plan_head_ride; conv_fused.hip: HEAD).  The caller sets head_n = the rows that ride (0 .. head_n - 1) and `head` = the head's sweep
  // arguments (out_sample is its X, row for row); the launcher makes `head` a plan of one workgroup per row that runs the Kzx units only, and sets the flags.
  int head_n = 0;
  // ... and the rest of the head's sweep behind them (fused_plan.h: plan_head_tail).  The caller sets tail_parts = Tail::parts (0: no tail; head_n is then Tail::n_rows, which
  // may be 0) and leaves the sweep plan's Kdiag segments, `kd` and `n_kd` in `head`; the launcher sets tail_n = the tail items and tail_upp = the units of a sub-row item.
  int tail_parts = 0, tail_upp = 0, tail_n = 0;
  unsigned* head_flag = nullptr; unsigned head_epoch = 0;   // [n_strips]: a strip's samples are written once its word is the launch's epoch
  HeadUnitsArgs head;
};
// the reverse pass of the same strip (conv_bwd_fused.hip): dK_uf = inv(L)^T [sum_r (S_r A1) o (2 gv_r) + alpha gm^T - 2 A1 o gvs]
struct ConvBwdArgs {
  const double* A1 = nullptr; long ld = 0; int Kc = 0;   // [Mp][ld], k-major (left by the forward's training form)
  const double* S = nullptr;                              // [R][Mp][Mp]  S_r = G_r G_r^T, zero beyond M
  const double* alpha = nullptr; int Rp = 0;              // [Mp][Rp]
  const double* Linv = nullptr;                           // [Mp][Mp] inv(L), row-major
  const double *gv = nullptr, *gm = nullptr, *gvs = nullptr;   // d var [Kc][R], d mean [Kc][R], row sums of d var [Kc]
  int M = 0, Mp = 0, R = 0;
  double* dKuf = nullptr;                                 // [Mp][ld]
};
bool conv_bwd_fused_ok(const dcgp_ctx* ctx, const ConvBwdArgs& a);
int conv_bwd_fused(dcgp_ctx* ctx, const ConvBwdArgs& a);
bool conv_fused_ok(const dcgp_ctx* ctx, const ConvFusedArgs& a);
int conv_fused(dcgp_ctx* ctx, const ConvFusedArgs& a);
// how many rows of the head's sweep described by head_* that launch carries (a: with n_mod and rep set; keeps_state: it leaves K_uf / A1 for a reverse
// pass); 0: none (fused_plan.h: plan_head_ride -- the one place that decides)
int conv_fused_rides_head(const dcgp_ctx* ctx, const ConvFusedArgs& a, bool keeps_state, bool head_form, long head_HWC, long head_lds, long head_nfm, bool in_flight,
                           bool chain_beside);
// whether that launch carries the head's WHOLE sweep, so that no sweep launch follows it (head_n_kd: the Kdiag slots per row of the sweep's plan): the sub-row
// items per row (0: no -- the answer of conv_fused_rides_head holds), and in *n_rows the whole rows in front of them (fused_plan.h: plan_head_tail)
int conv_fused_head_tail(const dcgp_ctx* ctx, const ConvFusedArgs& a, bool keeps_state, bool head_form, long head_HWC, long head_lds, long head_nfm, long head_n_kd,
                         bool in_flight, bool chain_beside, int* n_rows);

// KL pieces of one layer -> kl4[0..3] = {mahalanobis, logdet_q, logdet_p, trace} (device)
int kl_layer(dcgp_ctx* ctx, const GpMats& g, const double* Lp, const double* LpinvT, int white, const char* ws_prefix,
             double* kl4);

// the status words of a model's factorisations: one device scan finds the first non-positive pivot (first_bad_pivot, tail_dev.h)
struct FactorStatus {
  const int* info[16];   // per factor group: potrf status words (0 or the 1-based failing column)
  int ninfo[16];
  int ngroups = 0;
};
// the ELBO assembly the tail kernel performs after the data term (nl == 0: data term only -> scal[0])
struct ElboFinish {
  int nl = 0;
  int M[8], R[8], white[8];
  double scale = 1.0;
  FactorStatus st;
  double* host_out = nullptr;   // pinned host slot (device-visible address): the four result words are also written there,
                                // so no copy command follows the launch
  double host_seq = 0.0;        // written to host_out[4] behind them (system-scope release): the word the host polls for (ticket + 1)
};
// RobustMax expectations of every row -> ve_rows, scal[0] = inv_s * their sum, and (fin.nl > 0) scal[40..43] = ELBO, data term,
// KL, potrf status from the KL pieces at scal[4 + 4 l ..]: one launch (cond.hip)
struct TailArgs;   // tail_dev.h
// The KL pieces of the layers inside the tail launch (one extra workgroup per layer): everything they read is parameter-only
// state the chain left behind -- the strip sums of prep_solve and the factors' diagonals.
struct KlTailLayer {
  const double* Lfac = nullptr; long ldf = 0;   // the KL prior's Cholesky factor (diagonal read: log-determinant)
  const double* Lq = nullptr;                   // [R][Mp][Mp] (diagonal read)
  const double* sums = nullptr;                 // [(R + 1)][ns] partial sums of squares (GpMats::klp / klpp): rows r < R all ns, row R the first nsa
  int ns = 0, nsa = 0;                          // 0: prep_solve's layout (ns = Mp / 16 strips, nsa = 1)
  int M = 0, Mp = 0, R = 0;
};
struct KlTail { int nl = 0; KlTailLayer l[8]; };
int elbo_tail_prepare(dcgp_ctx* ctx, TailArgs* t);   // Gauss-Hermite table and arrival counters of a TailArgs
int elbo_tail(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n_rows, int n_labels, int K, double eps,
              double* ve_rows, double inv_s, double* scal, const ElboFinish& fin, const KlTail* kl = nullptr);
int varexp_rows(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n_rows, int n_labels, int K,
                double eps, double* out_rows, int predict);
const double* gauss_hermite_table(dcgp_ctx* ctx);   // [40]: 20 nodes then 20 weights (device)

// evaluate.hip: the test-set evaluation tail.  eval_tail: one launch per batch of n images x S samples (head mean / var rows [S*n][K]):
// per image at index lo + i of the whole set the log predictive density, the sample-mean probabilities (p_mean may be nullptr) and
// ok = 1 / 0 (arg-max == label) or -1 (label outside [0, K)).  eval_sum: one launch behind the last batch, res[4] = {correct count,
// sum of the log densities, first non-positive pivot of the status words in st, labels outside [0, K)}.
constexpr int kEvalMaxSlots = 8192;   // S * K + K doubles of LDS per workgroup (64 KB)
int eval_tail(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n, int S, int K, double eps, long lo,
              double* logdens, double* p_mean, int* ok);
int eval_sum(dcgp_ctx* ctx, const double* logdens, const int* ok, long n, const FactorStatus& st, double* res);

// pointwise.hip: the tails of the per-output likelihoods -- kind 1 Gaussian(s2), 2 Bernoulli (probit; y == 1 positive), 4 StudentT(scale, deg_free nu;
// c_nu = student_t_const(nu)), 5 Poisson(exp link, binsize) -- targets y [n_labels][K] float64, row r reads y[r % n_labels].  The trainable parameter
// (the Gaussian variance, the StudentT scale) is read from its device word `par` where that is set (a model's), else from par_val (the stand-alone
// entry points).  quad_elbo_tail: elbo_tail's counterpart (same scal / fin / KlTail contract; any K >= 1).  quad_grad: gm, gv [rows][K] and, kinds 1 and 4,
// gpar[0] = d / d par, all times weight.  quad_elementwise: per element of [n] what = 0 the variational expectation (out_a), 1 (E_y, V_y) (out_a, out_b;
// either may be nullptr; y unused), 2 the log density of one sample (out_a).  quad_eval_tail / quad_eval_sum: eval_tail / eval_sum's counterparts -- per
// image the log density summed over K, per (image, k) the log density (ld_nd, may be nullptr) and the sample-mean E_y (y_mean, may be nullptr), per image
// the score summed over K (the squared error of that mean; Bernoulli: the correct outputs); res[4] = {sum of scores, sum of log densities, first
// non-positive pivot, 0}.
struct QuadLik {
  int kind = 0;                       // 1 Gaussian, 2 Bernoulli, 4 StudentT, 5 Poisson
  const double* par = nullptr;        // Gaussian: the variance's device word, StudentT: the scale's; nullptr: par_val
  double par_val = 1.0, nu = 3.0, c_nu = 0.0, binsize = 1.0;
};
double student_t_const(double nu);    // lgamma((nu + 1) / 2) - lgamma(nu / 2) - log(nu pi) / 2
int quad_elbo_tail(dcgp_ctx* ctx, const QuadLik& q, const double* mu, const double* var, const double* y, int n_rows, int n_labels, int K,
                   double* ve_rows, double inv_s, double* scal, const ElboFinish& fin, const KlTail* kl = nullptr);
int quad_grad(dcgp_ctx* ctx, const QuadLik& q, const double* mu, const double* var, const double* y, int rows, int K, int n_labels, double weight,
              double* gm, double* gv, double* gpar);
int quad_elementwise(dcgp_ctx* ctx, const QuadLik& q, int what, const double* mu, const double* var, const double* y, long n, double* out_a,
                     double* out_b);
int quad_eval_tail(dcgp_ctx* ctx, const QuadLik& q, const double* mu, const double* var, const double* y, int n, int S, int K, long lo,
                   double* logdens, double* ld_nd, double* y_mean, double* score);
int quad_eval_sum(dcgp_ctx* ctx, const double* logdens, const double* score, long n, const FactorStatus& st, double* res);

// softmax.hip: the Softmax likelihood's tails (int32 labels y; nodes [Q][K] on the device, the same table for every row; 2 <= K, 1 <= Q,
// Q * K <= 4096, else DCGP_ERR_ARG).  softmax_elbo_tail: elbo_tail's counterpart (same scal / fin / KlTail contract); a label outside [0, K) leaves
// NaN.  softmax_grad: gm, gv [rows][K] times weight.  softmax_predict: out_mean = p, out_var = p - p^2 (either may be nullptr).  softmax_eval_tail /
// softmax_unc_tail: eval_tail / unc_tail with the probabilities of the softmax rule (eval_sum / unc_sum add them up).  softmax_density_grad: the
// density objective's tail of dcgp_model_input_grad.  Every one of them gives the same bits for the probabilities of the same row.
int softmax_elbo_tail(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n_rows, int n_labels, int K, const double* nodes, int Q,
                      double* ve_rows, double inv_s, double* scal, const ElboFinish& fin, const KlTail* kl = nullptr);
int softmax_grad(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int rows, int n_labels, int K, const double* nodes, int Q,
                 double weight, double* gm, double* gv);
int softmax_predict(dcgp_ctx* ctx, const double* mu, const double* var, int rows, int K, const double* nodes, int Q, double* out_mean, double* out_var);
int softmax_eval_tail(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n, int S, int K, const double* nodes, int Q, long lo,
                      double* logdens, double* p_mean, int* ok);
struct UncOut;
int softmax_unc_tail(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n, int S, int K, const double* nodes, int Q, long lo,
                     const UncOut& o);
int softmax_density_grad(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n_img, int S, int K, const double* nodes, int Q,
                         double* J, double* gm, double* gv);

// uncertainty.hip: the uncertainty tails (dcgp_model_evaluate_uncertainty).  unc_tail / bern_unc_tail: eval_tail / quad_eval_tail (Bernoulli) with the same
// bits for logdens, p_mean and the correct count, plus per entry (image; Bernoulli: (image, output)) at its index in the whole set the
// predictive entropy, the expected entropy (may be nullptr), their difference, the confidence and the prediction.  y may be nullptr:
// then logdens, ok and brier are not touched.  unc_tail keeps kUncExtraSlots wave partials beside eval_tail's LDS: S * K + K + 48 <= kEvalMaxSlots.
// unc_sum: one launch behind the last batch, res[9] = {correct, sum of the log densities, first non-positive pivot, labels outside
// [0, K), ECE, MCE, Brier score, mean predictive entropy, mean mutual information} and the reliability table [bins][3] = {count, sum of
// confidences, correct count}; ok == nullptr (no labels): words 0, 1, 4, 5, 6 are NaN and the table's third column is 0.
constexpr int kUncExtraSlots = 48;   // three sums x 16 waves
struct UncOut {
  double* logdens = nullptr; double* p_mean = nullptr;   // [N_total], [N_total][K] (p_mean may be nullptr)
  int* ok = nullptr; double* brier = nullptr;            // per entry: 1 / 0 / -1 (label outside [0, K)); the entry's Brier term
  double* pred_ent = nullptr; double* exp_ent = nullptr; double* mi = nullptr; double* conf = nullptr; int* pred = nullptr;
};
struct UncSumArgs {
  const double* logdens = nullptr; long n_img = 0;
  const int* ok = nullptr; const double* brier = nullptr; const double* pred_ent = nullptr; const double* mi = nullptr;
  const double* conf = nullptr; long n_ent = 0;
  int bins = 0; double* table = nullptr;
};
int unc_tail(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n, int S, int K, double eps, long lo, const UncOut& o);
int bern_unc_tail(dcgp_ctx* ctx, const double* mu, const double* var, const double* y, int n, int S, int K, long lo, const UncOut& o);
int unc_sum(dcgp_ctx* ctx, const UncSumArgs& a, const FactorStatus& st, double* res);

// likelihood.hip: which likelihood a model has is decided there and nowhere else.  Likelihood: the kind with its parameters; Targets: int32
// labels [N] or float64 targets [N][K] of a whole set (either pointer may be nullptr where labels are optional: f64 still says which entry
// point they came through).  Each lik_* function dispatches once on the kind to the launchers above and to robustmax_grad (grad.hip: the RobustMax
// seeds gm, gv [rows][K] = weight * d E_q[log p(y | f)] / d(mean, var)); lik_eval_tail / lik_unc_tail take the whole set's targets and batch `lo`.
struct Likelihood {
  int kind = 0;                  // 0 RobustMax, 3 Softmax (labels), 1 Gaussian, 2 Bernoulli (probit), 4 StudentT, 5 Poisson (exp link) (targets)
  double eps = 1e-3;             // RobustMax epsilon
  const double* s2 = nullptr;    // the Gaussian variance's device word; StudentT: the scale's
  const double* nodes = nullptr; int Q = 0;   // Softmax: the node table [Q][K] on the device (nullptr: none set yet)
  double nu = 3.0, c_nu = 0.0;   // StudentT: degrees of freedom (fixed) and student_t_const(nu)
  double binsize = 1.0;          // Poisson
  bool float_targets() const { return kind == 1 || kind == 2 || kind == 4 || kind == 5; }    // the _f64y entry points
  int n_params() const { return kind == 1 || kind == 4 ? 1 : 0; }   // trainable words (the Gaussian variance, the StudentT scale): lik_grad_seeds wants a gs2 for each
  QuadLik quad() const { QuadLik q; q.kind = kind; q.par = s2; q.nu = nu; q.c_nu = c_nu; q.binsize = binsize; return q; }   // kinds 1, 2, 4, 5
};
struct Targets {
  const int32_t* labels = nullptr; const double* values = nullptr; int K = 1; bool f64 = false;
  static Targets of(const int32_t* y, const double* yf, int K) { return Targets{y, yf, K, yf != nullptr}; }
  Targets from(long lo) const { return Targets{labels ? labels + lo : nullptr, values ? values + lo * K : nullptr, K, f64}; }   // the targets from image lo on
};
struct EvalOut {   // per image of the whole set (p_mean, ld_nd per (image, output); either may be nullptr)
  double* logdens = nullptr; double* ld_nd = nullptr; double* p_mean = nullptr;
  int* ok = nullptr;          // RobustMax: eval_tail's ok
  double* score = nullptr;    // Gaussian, StudentT, Poisson: squared error, Bernoulli: correct outputs
};
int robustmax_grad(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int rows, int n_labels, int K, double eps, double weight,
                   double* gm, double* gv);
int lik_check_targets(dcgp_ctx* ctx, const Likelihood& lik, const Targets& t, const char* who);   // targets of the wrong type for this likelihood
int lik_elbo_tail(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, const Targets& t, int n_rows, int n_labels, int K,
                  double* ve_rows, double inv_s, double* scal, const ElboFinish& fin, const KlTail* kl = nullptr);
int lik_grad_seeds(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, const Targets& t, int rows, int n_labels, int K,
                   double weight, double* gm, double* gv, double* gs2);   // gs2[0] = d / d s2 (StudentT: d / d scale) (n_params() > 0, else unused)
int lik_predict(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, long n, double* out_mean, double* out_var);
// the label likelihoods: lik_class_probs -- out_p [rows][K] class probabilities per row (dcgp_model_predict_y); lik_density_max_k -- the classes the
// density objective of dcgp_model_input_grad takes; lik_density_grad -- its tail (rm_density_grad, input_grad.hip / softmax_density_grad): J [n_img] and
// (gm, gv) = d J / d(mean, var) of the rows [S n_img][K], row s n_img + n, labels y already inside [0, K)
int lik_class_probs(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, int rows, int K, double* out_p);
int lik_density_max_k(const Likelihood& lik);
int lik_density_grad(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, const int32_t* y, int n_img, int S, int K, double* J,
                     double* gm, double* gv);
constexpr int kRmDensityMaxK = 16;   // classes of rm_density_grad_kernel's LDS tiles
int rm_density_grad(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n_img, int S, int K, double eps, double* J, double* gm,
                    double* gv);
int lik_eval_tail(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, const Targets& all, int n, int S, int K, long lo,
                  const EvalOut& o);
int lik_eval_sum(dcgp_ctx* ctx, const Likelihood& lik, const EvalOut& o, long n, const FactorStatus& st, double* res);
int lik_unc_tail(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, const Targets& all, int n, int S, int K, long lo,
                 const UncOut& o);

// patch_map.hip: per-patch evidence maps of a patch head with an RBF base kernel, out [rows][P][R] = (w_p / P) sum_m k(z_m, x_n[p]) beta[m][r]
// (row n shows X[n % n_mod]); asynchronous on ctx->stream.  ZS: the sweeps' operand of Z (sweep_dev.h) or nullptr (built from Z).  beta [M][R],
// or nullptr: beta = LinvT alpha from a layer's own factors (alpha [Mp][Rpa] = inv(L) q_mu, q_mu itself when whitened).
int patch_map(dcgp_ctx* ctx, const double* X, long rows, int n_mod, const ViewGeom& v, const double* Z, const double* ZS, int M, double variance,
              double lengthscale, const double* w, const double* beta, const double* LinvT, const double* alpha, int Rpa, int R, double* out,
              const std::string& pfx);

// deterministic single-block sum of n doubles, scaled: out[0] = scale * sum
int reduce_sum(dcgp_ctx* ctx, const double* in, long n, double scale, double* out);
constexpr int REDUCE_JOBS_MAX = 12;
struct ReduceJobs { const double* in[REDUCE_JOBS_MAX]; long n[REDUCE_JOBS_MAX]; double scale[REDUCE_JOBS_MAX]; double* out[REDUCE_JOBS_MAX]; };
int reduce_sum_multi(dcgp_ctx* ctx, const ReduceJobs& jobs, int count);   // out[k][0] = scale[k] * sum(in[k][0..n[k])), one launch

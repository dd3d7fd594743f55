// Internal: the device-resident model (layers + per-step outputs), shared by model.hip (forward), grad.hip (backward) and optim.hip (update).
#pragma once
#include "layer_impl.h"

struct dcgp_model {
  dcgp_ctx* ctx = nullptr;
  int S = 1;
  double jitter = 1e-3;
  double eps = 1e-3;   // RobustMax epsilon (conv_gp/models.py:67 keeps gpflow's default)
  // likelihood (dcgp_model_set_likelihood): 0 RobustMax (labels, int32), 1 Gaussian, 2 Bernoulli (probit) (targets [N][K] float64).  The
  // Gaussian variance lives on the device (d_lik[0]; the tails and the optimiser read and write it there), its Adam moments in d_lik[1],
  // d_lik[2] and its gradient in the last slot of the head's gradient block (LayerState::glik).  Bernoulli has no parameter: no d_lik, no slot.
  // 3 Softmax (labels, int32): no parameter either; its node table [lik_Q][K] lives in d_nodes (dcgp_model_set_likelihood_nodes) and is no
  // part of the parameter state -- replacing it starts no new parameter version.
  // 4 StudentT, 5 Poisson with the exp link (targets [N][K] float64; dcgp_model_set_likelihood_params): the StudentT scale lives where the Gaussian
  // variance does (d_lik[0], moments beside it, gradient in glik), its degrees of freedom are fixed (lik_nu, lik_cnu = student_t_const(lik_nu));
  // Poisson has its bin size (lik_binsize) and no trainable parameter.
  int lik_kind = 0;
  double lik_nu = 3.0, lik_cnu = 0.0, lik_binsize = 1.0;
  Likelihood lik() const { return Likelihood{lik_kind, eps, d_lik, lik_Q > 0 ? d_nodes : nullptr, lik_Q, lik_nu, lik_cnu, lik_binsize}; }   // what likelihood.hip's functions take
  double* d_lik = nullptr;
  double* d_nodes = nullptr; size_t nodes_cap = 0; int lik_Q = 0;
  bool lik_frozen = false;   // dcgp_model_set_trainable(.., "likelihood_variance" / "likelihood_scale", 0)
  std::vector<std::unique_ptr<LayerState>> layers;   // conv layers..., head last (once set)
  bool has_head = false;
  bool keep_outputs = false;
  bool keep_state = false;   // the forward leaves K_uf / A1 of every conv layer in HBM (set around the forward of dcgp_elbo_grad)
  bool data_grad = false;    // set around the forward of dcgp_model_input_grad: keep_state without a training step -- the parameter-only chain is
                             // an evaluation's (it may stand, and it is recorded, as for propagate / predict_y)
  bool grad_follows = false; // set around the forward of dcgp_elbo_grad: forward_all hands the parameter-only part of the reverse pass to the side stream
  int gkl_state = 0;         // forward_all of such a step: 0 nothing to hand over, 1 the side stream itself holds the parameter-only chain, 2 it waits for ctx->ev_fork
  int gkl_prep_wait = 0;     // forward_all: grad_kl_early must also wait for ev_prep[bank][0 .. gkl_prep_wait) (chain on a side stream, mark on the main stream)
  int prep_early[8] = {};    // per layer: bit 0 its zero fills, G^T and the factor's lower triangle, bit 1 S_r = G_r G_r^T were enqueued by grad_kl_early
  bool kl_early[8] = {};     // per layer: grad_kl_early enqueued its kl_products for the step in flight (consumed by model_backward)
  int adam_t = 0;        // Adam steps taken on this model's moment buffers (bias correction; dcgp_model_adam_step with t = 0)
  // clipping by global norm (dcgp_model_set_grad_clip; optim.hip): 0 = off.  d_clip[0]: the step's scale c, read by the update; d_clip[1 ..]: the
  // norm's per-block partial sums (grow-only, allocated with the first clipped step).  grad_norms: the pre-clip norms of the most recent
  // optimiser call's steps (opt_readback appends one per step; the entry points clear it)
  double grad_clip = 0.0;
  double* d_clip = nullptr; size_t clip_cap = 0;
  bool norm_pending = false;   // the step in flight left its norm in the pinned slot
  std::vector<double> grad_norms;
  int shard_lo = 0, shard_global = 0;   // this rank's first image and the global batch (dcgp_model_set_shard): device-RNG counters
  int grad_exchange = 0; // multi-rank training step (dcgp_model_train_step_adam): 0 all-reduce of every layer's gradient block + the full update on every rank,
                         // 1 reduce-scatter -> Adam on this rank's shard -> all-gather of the parameters (dcgp_model_set_grad_exchange)
  bool adam_follows = false, grad_scattered = false;   // the step in flight ends in the optimiser update / its gradient blocks hold this rank's shard only
  int grad_shards = 0;   // KL gradient weight 1 / shards; 0 = number of ranks of the ctx's communicator (1 without one)
  // two banks of parameter-only state (LayerState::use_bank): factor groups, events and ELBO scalars follow the bank
  std::vector<FactorGroup> groups[2];
  bool groups_built[2] = {false, false};
  int bank = 0;                                  // bank of the most recent forward
  hipEvent_t ev_sweep[2] = {}, ev_factor[2] = {}, ev_kl[2] = {}, ev_prep[2][8] = {};
  hipEvent_t done_ev[2] = {};                    // not owned: the event that marks the end of the last step on the bank (a result-ring event)
  hipEvent_t ev_eval[2] = {};                    // per bank: the end of a dcgp_model_evaluate batch (its done_ev while the call enqueues)
  bool done_valid[2] = {false, false};
  bool events_ok = false;
  // the KL pieces computed inside the tail launch (layers whose sums prep_solve left behind): per bank, set by forward_all
  KlTail kl_tail[2];
  bool kl_in_tail[2] = {false, false};
  bool kl_rode[2] = {false, false};   // ... and the head's one-launch conditional of this step carried them (head_cond.hip): the tail launch has none
  // per-layer outputs of the most recent forward
  struct Out { double *sample = nullptr, *mean = nullptr, *var = nullptr; int rows = 0, width = 0; size_t cap = 0; };
  std::vector<Out> outs;
  double* d_scal = nullptr;   // per bank (64 doubles each): [0]=data, [4 + 4l ..] 4 KL pieces of layer l, [40..43] ELBO, data term, KL, potrf status
  double* d_ve = nullptr; size_t ve_cap = 0;
  double* d_kd = nullptr; size_t kd_cap = 0;
  int id = 0;
  // Parameter-only state kept across steps at unchanged parameters.  Every entry point that writes a parameter (set_param, the optimiser
  // steps, the natural-gradient step) bumps param_version; a step that ran the chain records the version and its bank.  factor_reuse: 0 never, 1 the
  // evaluation entry points (propagate, predict_y) reuse a valid chain, 2 the forward ELBO as well (evaluation sweeps at one parameter state: the
  // reference's LogLikelihoodLogger, conv_gp/utils/log.py:55-68) -- never the default for the ELBO step: the reference's step recomputes it.
  uint64_t param_version = 1, chain_version = 0;
  bool chain_with_kl = false;   // the recorded chain ran for an ELBO step (KL pieces / deferred factor copy in place)
  int factor_reuse = 1;
  uint64_t chain_skips = 0;     // steps that reused it (tests, bench)
  // multi-rank training: steps taken with the sharded update (exchange mode 1) leave every rank with the Adam moments of its own shard only
  uint64_t sharded_steps = 0;
  // throughput mode of the forward (dcgp_elbo_forward_enqueue / _collect): results of up to RING steps in flight land in
  // pinned host slots, one event per slot; tickets are handed out and collected in order
  static constexpr int RING = 4;
  double* h_ring = nullptr;            // RING x 8 pinned doubles: ELBO, data term, KL, potrf status, completion word (ticket + 1)
  double* h_ring_dev = nullptr;        // the same slots as the device addresses them (written by the last kernel of a step)
  hipEvent_t ring_ev[RING] = {};
  uint64_t enq_seq = 0, col_seq = 0;   // tickets handed out / collected
  // the training set of dcgp_model_train_run_adam (train_run.hip): uploaded once by dcgp_model_set_dataset, rows gathered per step on the device
  double* ds_X = nullptr;              // [ds_n][ds_len], ds_len = H W C of layer 0
  void* ds_Y = nullptr;                // int32 [ds_n] (ds_D == 0) or float64 [ds_n][ds_D]
  long ds_n = 0, ds_len = 0;
  int ds_D = 0;
  // ... and the run's own buffers (grow-only): the index table of a run, the batch of the step in flight
  int32_t* run_idx = nullptr; size_t run_idx_cap = 0;
  double* run_X = nullptr; size_t run_X_cap = 0;
  void* run_Y = nullptr; size_t run_Y_cap = 0;   // (bytes)
  // augmentation of a run's batches (dcgp_model_set_augmentation; augment.hip): the caller's image geometry, the largest shift and whether to
  // flip.  Off (the default): the run gathers with gather_batch_kernel, exactly as before.
  int aug_H = 0, aug_W = 0, aug_C = 0, aug_shift = 0, aug_hflip = 0;
  bool augmenting() const { return aug_shift > 0 || aug_hflip != 0; }
  // views of an evaluation (dcgp_model_set_eval_views; augment.hip, eval_batches): the table [eval_V][3] of (dy, dx, flip) on the host and on the
  // device, and the caller's image geometry.  Off (eval_V == 0, the default) and the single identity view: the evaluation runs exactly as before.
  std::vector<int32_t> eval_views;
  int32_t* d_eval_views = nullptr; size_t eval_views_cap = 0;
  int eval_V = 0, ev_H = 0, ev_W = 0, ev_C = 0;
  bool eval_views_active() const { return eval_V > 1 || (eval_V == 1 && (eval_views[0] != 0 || eval_views[1] != 0 || eval_views[2] != 0)); }
  // zero padding of a layer's input (dcgp_model_set_input_padding; pad.hip): layer l was added with the PADDED H, W and reads a padded copy of
  // its predecessor's sample (of X for layer 0).  pad_in[l]: that copy as the most recent forward left it (a workspace; layer 0's per bank) --
  // the reverse pass reads it, nothing overwrites it before the model's next forward.  pad_ok: the geometry was checked since the last change.
  int pad[8] = {};
  bool any_pad = false, pad_ok = false;
  const double* pad_in[8] = {};
  // dilation of a conv layer (dcgp_model_set_dilation; dilate.hip): the window's taps sit dil[l] pixels apart.  The layer is added with its true
  // (padded) input size like any other; dcgp_model_set_dilation keeps that size here (dil_H, dil_W) and switches LayerState::v to the PHASE
  // geometry -- H = ceil(Hp / d), W = ceil(Wp / d) -- so v is what the kernels see: the layer runs as an ordinary VALID layer on the rows * d^2
  // phase sub-images of its input (space-to-batch), and its outputs go back to image layout behind it.
  // dil_in[l]: the split input as the most recent forward left it (a workspace; layer 0's per bank), read by the reverse pass like pad_in[l].
  // dil_out[l]: the layer's (sample, mean, var) in phase layout, as its kernels wrote them (outs[l] holds the image layout).
  int dil[8] = {1, 1, 1, 1, 1, 1, 1, 1};
  int dil_H[8] = {}, dil_W[8] = {};   // the true size of a layer with dil[l] > 1
  bool any_dil = false;
  const double* dil_in[8] = {};
  struct PhaseOut { double *sample = nullptr, *mean = nullptr, *var = nullptr; } dil_out[8];
  // A layer's true geometry: its (padded) input H x W and its output Ho x Wo, in pixels of the image -- LayerState::v itself unless the layer is
  // dilated.  Everything that derives the caller's image size or an output width goes through here.  It depends on the layer alone.
  struct Geom { int H = 0, W = 0, Ho = 0, Wo = 0; long P() const { return (long)Ho * Wo; } };
  int dil_of(int li) const { return li >= 0 && li < 8 ? dil[li] : 1; }
  Geom geom(int li) const {
    const ViewGeom& v = layers[li]->v;
    const int d = dil_of(li);
    Geom g;
    if (d <= 1) { g.H = v.H; g.W = v.W; g.Ho = v.Ho; g.Wo = v.Wo; return g; }
    g.H = dil_H[li]; g.W = dil_W[li];
    g.Ho = g.H - d * (v.f - 1); g.Wo = g.W - d * (v.f - 1);
    return g;
  }
  // one image of the caller's X: layer 0's true geometry without its padding
  long image_len() const { const Geom g = geom(0); return (long)(g.H - 2 * pad[0]) * (g.W - 2 * pad[0]) * layers[0]->v.C; }

  ~dcgp_model() {
    for (void* p : {(void*)ds_X, ds_Y, (void*)run_idx, (void*)run_X, run_Y, (void*)d_eval_views, (void*)d_clip}) dev_free(ctx, p);
    if (h_ring) hipHostFree(h_ring);
    for (auto& e : ring_ev) if (e) hipEventDestroy(e);
    for (auto& gs : groups) for (auto& gr : gs) gr.release();
    for (int b = 0; b < 2; ++b) {
      if (ev_sweep[b]) hipEventDestroy(ev_sweep[b]);
      if (ev_factor[b]) hipEventDestroy(ev_factor[b]);
      if (ev_kl[b]) hipEventDestroy(ev_kl[b]);
      if (ev_eval[b]) hipEventDestroy(ev_eval[b]);
      for (auto& e : ev_prep[b]) if (e) hipEventDestroy(e);
    }
    for (auto& o : outs) { dev_free(ctx, o.sample); dev_free(ctx, o.mean); dev_free(ctx, o.var); }
    for (double* p : {d_scal, d_ve, d_kd, d_lik, d_nodes}) dev_free(ctx, p);
  }
};

// model.hip: the forward ELBO of a minibatch; leaves every layer's outputs in model->outs (keep_outputs) and the
// factorisations / conditional operands in the layers' GpMats.  out_host[0..2] = ELBO, data term, KL.
int elbo_forward_impl(dcgp_model* model, const double* X, const int32_t* y, int N, double scale,
                      const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0, double* out_host,
                      int* info_host, const double* yf = nullptr);
// the two halves of it: queue the step's launches and the copy of its result into a ring slot / wait for the oldest slot
int elbo_forward_enqueue_impl(dcgp_model* model, const double* X, const int32_t* y, int N, double scale,
                              const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0, uint64_t* ticket,
                              bool pipelined = false, const double* yf = nullptr);   // yf: Gaussian targets [N][K] (y is then nullptr)
int elbo_forward_collect_impl(dcgp_model* model, uint64_t ticket, double* out_host, int* info_host);
// grad.hip: reverse pass over the state the forward left behind; fills every layer's gradient buffers (the likelihood's seeds, the reverse walk over
// the layers, the join of its side streams, the likelihood's own gradient and the collectives)
int model_backward(dcgp_model* model, const Targets& targets, const double* X, int N, double scale, int dedup_layer0);
// optim.hip: one optimiser launch over every trainable group of the model, behind whatever the stream holds (sgd: plain ascent, otherwise Adam with
// the bias-corrected rate lr; status != null: a non-zero word there leaves every parameter untouched) / once the stream has been synchronised, the
// updated kernel hyper-parameters back into the host-side layer state
int opt_enqueue(dcgp_model* model, const char* who, bool sgd, double lr, double beta1, double beta2, double eps, const double* status, int vranks = 0);
int opt_readback(dcgp_model* model);
// enqueue == false: 1 if a training step's forward should hand the KL adjoint's products to the side stream, else 0;
// enqueue == true: do it (wait_fork: behind ctx->ev_fork, recorded where the parameter-only chain ended)
int grad_kl_early(dcgp_model* model, bool enqueue, bool wait_fork);
// grad.hip: one training step (dcgp_model_train_step_adam / _f64y behind their argument checks; y or yf, the other nullptr)
int train_step_adam_run(dcgp_model* model, const double* X, const int32_t* y, int N, double scale, const double* const* z_per_layer_host,
                        uint64_t seed, int dedup_layer0, double lr, double beta1, double beta2, double eps, int t, double* out_host,
                        int* info_host, const double* yf);

// model.hip: the data path of an evaluation forward (propagate's: no KL, factor reuse as for propagate) on `S` samples, asynchronous on ctx->stream;
// with keep_outputs / keep_state / data_grad set it leaves what model_backward_data reads.  *rows_last: rows of the head's mean / var.
int forward_data_impl(dcgp_model* model, const double* X, int N, int S, const double* const* z_per_layer_host, uint64_t seed,
                      int dedup_layer0, int* rows_last);
// model.hip: the status words of the factorisations of the model's current bank, for the kernel that closes a call (first_bad_pivot, tail_dev.h)
int fill_status(dcgp_model* model, FactorStatus* st);
// grad.hip: the same reverse walk's data path only (Bk::data_only: no gradient block is touched), from the head's seeds gm, gv [rows][R] to out_dX
// [N][H W C] (device)
int model_backward_data(dcgp_model* model, const double* X, int N, int S, int dedup_layer0, double* gm, double* gv, double* out_dX);
// pad.hip: dst [rows][H + 2p][W + 2p][C] <- src [rows][H][W][C] with a zero border / its adjoint, dst [rows][H][W][C] <- the interior of
// src [reps][rows][H + 2p][W + 2p][C] summed over the replicas
int pad_images(dcgp_ctx* ctx, hipStream_t stream, const double* src, long rows, int H, int W, int C, int p, double* dst);
int crop_images(dcgp_ctx* ctx, hipStream_t stream, const double* src, int reps, long rows, int H, int W, int C, int p, double* dst);
// dilate.hip: space-to-batch, dst [rows d^2][ceil(H / d)][ceil(W / d)][C] <- src [rows][H][W][C] with the fill written as zeros / its inverse,
// dst [rows][H][W][C] <- src [reps][rows d^2][..][..][C] summed over the replicas; a fill entry of src is never read
int s2b_images(dcgp_ctx* ctx, hipStream_t stream, const double* src, long rows, int H, int W, int C, int d, double* dst);
int b2s_images(dcgp_ctx* ctx, hipStream_t stream, const double* src, int reps, long rows, int H, int W, int C, int d, double* dst);
// augment.hip: nullptr, or what is wrong with an augmentation's geometry / the augmenting gather of a run's step (rows idx_dev[0 .. batch) of the
// resident set into run_X on ctx->stream, image b with the draw of (seed, b); targets as gather_batch_kernel copies them)
const char* augment_geometry_error(int H, int W, int C, int max_shift);
int gather_augment_batch(dcgp_model* model, const int32_t* idx_dev, int batch, uint64_t seed, const int32_t* y32, const double* yf, int D,
                         int32_t* yb32, double* ybf);
// augment.hip: the model's eval_V views of X [n] images into out [eval_V][n] images (view-major), on ctx->stream
int gather_eval_views(dcgp_model* model, const double* X, int n, double* out);
// input_grad.hip: dX of a scalar-lengthscale RBF patch layer from E / cs in one launch (the product on the matrix pipe, the fold in LDS);
// extra [rows P][L] or nullptr is added to the patch gradients before the fold.  _ok: the shape is covered (otherwise the product + col2im pair)
bool patch_adjoint_fused_ok(const LayerState& L, long rows);
int patch_adjoint_fused(dcgp_ctx* ctx, const LayerState& L, const double* E, long ld, const double* cs, const double* Xin, int rows, int n_mod,
                        const double* extra, double* dXin);

// model.hip -- device-resident layers and the model-level forward (DGP_Base.propagate /
// _build_likelihood of doubly_stochastic_dgp; ConvLayer.conditional_ND of conv_gp/layers.py:96-135;
// SVGP_Layer.conditional_ND with the ConvKernel head of conv_gp/kernels.py:79-136).
//
// Per forward step, nothing cached across steps (main stream = the data path, side stream = the replicated M x M work):
//   1. main: every layer's Kuu(Z) (+ prior Kuu(Z0)), padded q_sqrt / q_mu, Z^T and |z|^2 -- one launch (prep.hip)
//   2. side: ONE batched Cholesky + inverse chain for all M x M matrices of the model (chol_fused.hip), then G / alpha of
//      every layer in one launch (head_cond.hip), then the KL terms; main meanwhile: the first layer's patch sweep
//   3. main, per conv layer: patch sweep -> stage-1 GEMM -> stage-3 GEMM -> mean -> finalize (+ sample)
//   4. main: head Kzx sweep (Kdiag beside it on the side stream), fused head conditional, RobustMax expectations
//   5. (multi-GPU) all-reduce of the data term, ELBO assembly, one 32-byte read-back, one host sync.
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "model_state.h"
#include "tail_dev.h"

namespace {

int g_model_counter = 0;

int build_groups(dcgp_model* m, int bank) {   // the layers must be on `bank` (use_bank)
  if (m->groups_built[bank]) return DCGP_OK;
  auto& groups = m->groups[bank];
  for (auto& gr : groups) gr.release();
  groups.clear();
  auto add = [&](int Mp, double* K, double* Linv, double* LinvT, const ChainRhs& r) {
    FactorGroup* g = nullptr;
    for (auto& gr : groups)
      if (gr.Mp == Mp) g = &gr;
    if (!g) { groups.emplace_back(); g = &groups.back(); g->Mp = Mp; }
    g->K.push_back(K); g->Linv.push_back(Linv); g->LinvT.push_back(LinvT); g->rhs.push_back(r);
    if (r.Lq || r.qmu) { g->ride = true; g->max_R = r.R > g->max_R ? r.R : g->max_R; }
  };
  // G = inv(L) Lq and alpha = inv(L) q_mu ride the chain (chol_fused.hip) where a layer is unwhitened and small enough; with a prior
  // Kuu(Z0) the same right-hand sides ride its chain for the KL's sums of squares
  for (auto& l : m->layers) {
    const GpMats& g = l->g;
    const bool rides = !l->white && g.Mp <= kChainRhsMaxMp && g.Rp <= 32 && g.G && g.alpha && g.klp;
    ChainRhs live{}, prior{};
    live.R = prior.R = g.R; live.Rp = prior.Rp = g.Rp;
    if (rides) { live.Lq = l->has_qsqrt ? g.Lq : nullptr; live.qmu = g.qmu; live.G = g.G; live.alpha = g.alpha; live.sums = g.klp; }
    if (rides && g.Kp && g.klpp && l->has_qsqrt) { prior.Lq = g.Lq; prior.qmu = g.qmu; prior.sums = g.klpp; }
    add(l->Mp, g.K, g.Linv, g.LinvT, live);
    if (g.Kp) add(l->Mp, g.Kp, g.Lpinv, g.LpinvT, prior);
  }
  m->groups_built[bank] = true;
  return DCGP_OK;
}

int ensure_events(dcgp_model* m) {
  if (m->events_ok) return DCGP_OK;
  dcgp_ctx* ctx = m->ctx;
  for (int b = 0; b < 2; ++b) {
    HIP_TRY(ctx, hipEventCreateWithFlags(&m->ev_sweep[b], hipEventDisableTiming));
    HIP_TRY(ctx, hipEventCreateWithFlags(&m->ev_factor[b], hipEventDisableTiming));
    HIP_TRY(ctx, hipEventCreateWithFlags(&m->ev_kl[b], hipEventDisableTiming));
    HIP_TRY(ctx, hipEventCreateWithFlags(&m->ev_eval[b], hipEventDisableTiming));
    for (auto& e : m->ev_prep[b]) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  m->events_ok = true;
  return DCGP_OK;
}

int ensure(dcgp_ctx* ctx, double** p, size_t* cap, size_t n) {
  if (*cap >= n && *p) return DCGP_OK;
  if (*p) { hipDeviceSynchronize(); dev_free(ctx, *p); *p = nullptr; }   // steps in flight on any stream may still use it
  if (dev_alloc(ctx, (void**)p, (n ? n : 2) * sizeof(double), "model_scratch") != hipSuccess) return ctx_fail(ctx, DCGP_ERR_ALLOC, "model: allocation failed");
  *cap = n;
  return DCGP_OK;
}

int ensure_out(dcgp_model* m, int li, int rows, int width) {
  auto& o = m->outs[li];
  size_t n = (size_t)rows * width;
  if (o.cap < n) {
    hipDeviceSynchronize();   // steps in flight on any stream may still use them
    dev_free(m->ctx, o.sample); dev_free(m->ctx, o.mean); dev_free(m->ctx, o.var);
    o.sample = o.mean = o.var = nullptr;
    if (dev_alloc(m->ctx, (void**)&o.sample, n * sizeof(double), "out_sample") != hipSuccess ||
        dev_alloc(m->ctx, (void**)&o.mean, n * sizeof(double), "out_mean") != hipSuccess ||
        dev_alloc(m->ctx, (void**)&o.var, n * sizeof(double), "out_var") != hipSuccess)
      return ctx_fail(m->ctx, DCGP_ERR_ALLOC, "model: output allocation failed");
    o.cap = n;
  }
  o.rows = rows; o.width = width;
  return DCGP_OK;
}

// multi-rank step: the assembly behind the all-reduce of the data term scal[0] -- the tail kernels' own (tail_dev.h), on one thread
__global__ void combine_kernel(double* __restrict__ scal, ElboFinish fin) {
  if (threadIdx.x == 0 && blockIdx.x == 0) elbo_assemble(scal, fin, scal[0]);
}

int read_info(dcgp_model* m, int* info_host) {
  dcgp_ctx* ctx = m->ctx;
  int bad = 0;
  for (auto& gr : m->groups[m->bank]) {
    std::vector<int> h(gr.K.size());
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), gr.d_info, h.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int v : h)
      if (v && !bad) bad = v;
  }
  if (info_host) *info_host = bad;
  if (bad) return ctx_fail(ctx, DCGP_ERR_NOT_PD, "Cholesky: matrix not positive definite at column %d", bad);
  return DCGP_OK;
}
// the end of an inference entry point: everything it enqueued behind forward_data_impl is done, then the factorisations' status
int finish_inference(dcgp_model* m, int* info_host) {
  HIP_TRY(m->ctx, hipStreamSynchronize(m->ctx->stream));
  return read_info(m, info_host);
}

// Restores ctx->stream when a forward step returns, whichever way
struct StreamGuard {
  dcgp_ctx* ctx; hipStream_t saved;
  explicit StreamGuard(dcgp_ctx* c) : ctx(c), saved(c->stream) {}
  ~StreamGuard() { ctx->stream = saved; ctx->ws_tag.clear(); }
};

// what the assembly at the end of a step needs: layer shapes, the status words of the factor groups, the pinned result slot
int fill_finish(dcgp_model* model, double scale, int slot, ElboFinish* fin) {
  const int nl = (int)model->layers.size();
  fin->nl = nl; fin->scale = scale;
  for (int l = 0; l < nl; ++l) { fin->M[l] = model->layers[l]->M; fin->R[l] = model->layers[l]->R; fin->white[l] = model->layers[l]->white; }
  DCGP_TRY(fill_status(model, &fin->st));
  fin->host_out = model->h_ring_dev + 8 * slot;   // the last kernel of the step writes the result words into the pinned slot itself
  fin->host_seq = (double)(model->enq_seq + 1);   // ... and this step's ticket + 1 behind them
  return DCGP_OK;
}

// ---- A forward step (forward_all): its schedule is decided once, in plan_step, and three functions enqueue from that plan ----
//   chain stream: everything that depends on the parameters only, into the bank of this step's parity -- Kuu / prior Kuu /
//                 Z^T / padded q_sqrt, q_mu of every layer, ONE batched Cholesky + inverse chain for all M x M
//                 matrices, G / alpha of every layer (one launch), the KL terms;
//   main stream:  the data path (sweeps, conditionals, sampling), gated per layer by the chain's events.
// pipelined (dcgp_elbo_forward_enqueue): main = 30 CUs of every XCD, side = the other 2, so that the chain of step i + 1 runs
// under the data path of step i without competing for its CUs; otherwise both streams see the whole chip.

// Where the operand preparation (prep.hip) goes.
// OnChain: one launch on the chain's stream, ev_sweep behind it for a first layer that sweeps beside the chain.  Steps kept in flight stay here: the preparation
// runs under the previous step's data path -- on the main stream it waited for that step (head-only model 4830 -> 4590 steps/s in flight).
// Split*: a synchronous step whose first layer's sweep is a launch of its own: that sweep is the step's critical path.  The preparation in TWO launches, each on
// the stream of its reader -- what a sweep reads (Z^T, |z|^2, the scaled Z) on the MAIN stream with the sweep directly behind it, the Gram matrices and
// the padded q_sqrt / q_mu on the chain's -- and no event between the streams at the head of the step: the record was a packet between the preparation
// and the sweep (7.6 us from one to the other), the wait held the chain back.  With the preparation on the chain's stream the sweep started 20.8 us
// into the step (8 us of preparation + the event), now at ~9.  (Option prep_on_chain: back to OnChain, A/B.)
// Which stream's part the host enqueues first is which part gets the chip first.  SplitChainFirst: a conv layer on the sweep + GEMM route (M > 256): the CHAIN is the
// longest path (the first product waits for inv(L) long after the sweep is done) -- enqueued behind the sweep its preparation ran 71 us beside it
// instead of ~15 and the first product of cfg4 started 53 us later (profiles/the first cut of this split)
// SplitSweepFirst: a model that opens with the head: the sweep is the step's longest path (170 us against the chain's ~150 beside it) -- its part and the sweep, then the
// chain's part BEHIND the sweep: at the head of a synchronous step the device waits for the host, ~4 us a launch
enum class PrepPlace { OnChain, SplitChainFirst, SplitSweepFirst };
// Where a training step marks the start of the parameter-only part of its reverse pass (grad.hip, grad_kl_early; ctx->ev_fork).  That part runs beside the
// forward pass on the auxiliary stream; dcgp_elbo_grad enqueues it behind the whole forward pass (in front of the layers the host kept the first layer
// waiting for 170 us, in front of the tail launch the end of the forward pass for 60).
// BehindFirstLayer: that layer's launch fills the chip at the full batch, and forty short launches squeezed in between its rounds cost it more than they
// gained.  BehindChain: a first layer of a few thousand patch columns -- the de-duplicated batch -- leaves half the chip idle: there the mark is behind the chain.
enum class ForkMark { BehindFirstLayer, BehindChain };

struct StepPlan {
  // The chain of the previous step stands if no parameter was written since and this step may use it (model_state.h: factor_reuse): same bank, no
  // preparation, no factorisation, no G / alpha, no KL launches -- the step is its data path.
  bool reuse = false;
  int bank = 0, rows0 = 0;   // rows0: rows entering layer 0; it reads image (row % N): tile(X,[S,1,1]) is never formed
  // Where the parameter-only chain runs.  A synchronous step has nothing else to do until the factorisation is there: the chain
  // sits on the main stream itself (no cross-stream hand-off in front of the first layer, ~15 us each) and only the KL terms
  // fork to the side stream.  A step enqueued beside others: the side stream of its bank, so that it overtakes the step in flight.
  // A first layer that opens with a sweep of its own (the sweep + GEMM route; a model that opens with the head -- the reference's "1-layer") needs Z
  // only for it: the sweep runs on the main stream beside the chain on the side stream, and the step is the longer of the two instead of their sum.
  hipStream_t main_s = nullptr, chain_s = nullptr, kl_s = nullptr;
  bool first_one_launch = true;   // layer 0's route (layer_impl.h: first_layer_one_launch -- the dispatch's own question; conv_forward refuses another answer)
  PrepPlace prep = PrepPlace::OnChain;
  // Layer 0's sweep needs nothing but the preparation: it goes to the main stream in front of the chain's ~12 launches -- enqueued behind
  // them it started when the host was done with those, 60 us after prepare_all had finished (cfg2 head-only: 0.287 -> 0.24 ms).  (Option no_early_sweep: A/B.)
  bool early_sweep = false;
  bool defer = false;   // with a single factor group its "chol_Lout" scratch stays untouched until the deferred copy runs on the KL stream
  ChainMode chain;
  ForkMark mark = ForkMark::BehindFirstLayer;
  // The conv layer whose persistent launch also runs the Kzx units of the head's rows 0 .. ride_rows - 1, in the workgroup time its partial last round
  // leaves (-1: none; fused_plan.h: plan_head_ride decides).  The head's sweep launch is then the other rows' Kzx units and the Kdiag chunks.
  int ride_layer = -1, ride_rows = 0;
  // ... and behind those rows the rest of the head's sweep -- ride_tail sub-row items per row that did not ride whole, every Kdiag chunk -- so that the head
  // launches no sweep at all (0: no; fused_plan.h: plan_head_tail decides, and ride_rows is then its count of whole rows, which may be 0)
  int ride_tail = 0;
  bool chain_beside() const { return chain_s != main_s; }   // events only where another stream waits for them: each record is a packet in front of the next launch
};
// what the caller of a step hands over
struct StepIn { const double* X; int N, S; const double* const* zs; uint64_t seed; int dedup; bool need_kl; };
std::string model_pfx(const dcgp_model* m) { return "m" + std::to_string(m->id) + "_"; }

// No HIP call, nothing written to the model or the ctx.
StepPlan plan_step(const dcgp_model* m, int N, int S, int dedup, bool need_kl, bool pipelined) {
  const dcgp_ctx* ctx = m->ctx;
  const LayerState& L0 = *m->layers[0];
  StepPlan p;
  p.reuse = !pipelined && !m->grad_follows && (!m->keep_state || m->data_grad) && m->chain_version == m->param_version && m->chain_with_kl == need_kl &&
            m->factor_reuse >= (need_kl ? 2 : 1) && !ctx->opt.no_factor_reuse;
  p.bank = p.reuse ? m->bank : m->bank ^ 1;
  const bool part = pipelined && ctx->stream_m && !ctx->no_side;   // (no_side: A/B switch, everything on one stream)
  p.main_s = part ? ctx->stream_m : ctx->stream;
  p.kl_s = ctx->no_side ? p.main_s : (part ? ctx->stream2_m : (pipelined ? (p.bank ? ctx->stream2b : ctx->stream2) : ctx->stream2));
  p.rows0 = dedup ? N : S * N;
  const long rows0k = (long)p.rows0 * m->dil[0] * m->dil[0];   // rows layer 0's kernels see: the phase sub-images of a dilated first layer
  p.first_one_launch = first_layer_one_launch(ctx, L0, (int)rows0k);
  p.chain_s = p.reuse ? p.main_s : ((pipelined || !p.first_one_launch) ? p.kl_s : p.main_s);
  p.early_sweep = p.chain_beside() && !p.first_one_launch && !ctx->opt.no_early_sweep;
  if (p.early_sweep && !pipelined && !ctx->opt.prep_on_chain) p.prep = L0.is_head ? PrepPlace::SplitSweepFirst : PrepPlace::SplitChainFirst;
  bool one_group = true;   // build_groups: one factor group per distinct Mp
  for (auto& l : m->layers) one_group = one_group && l->Mp == L0.Mp;
  p.defer = one_group && need_kl && !m->keep_state;
  p.chain = ChainMode{!p.chain_beside() && !pipelined, p.first_one_launch};
  p.mark = rows0k * L0.v.P >= 8192 ? ForkMark::BehindFirstLayer : ForkMark::BehindChain;
  const int nl = (int)m->layers.size();
  // (a padded head sweeps the padded copy of the sample: the ride reads the sample itself)
  // (a dilated layer completes its sample in the batch-to-space pass behind its launch, dilate.hip: no row of the head rides that launch)
  // (a layer with a mean filter completes its sample in a pass behind its launch, conv_mean.hip: no row may read the sample inside the launch;
  // a mixed layer's launch writes its latent sample, the maps the head reads come out of the pass behind it, mix.hip)
  if (nl >= 2 && m->layers[nl - 1]->is_head && !m->layers[nl - 2]->is_head && m->pad[nl - 1] == 0 && !m->layers[nl - 2]->mean_W && !m->layers[nl - 2]->mix_W &&
      m->dil_of(nl - 2) == 1) {
    const int li = nl - 2;
    const LayerState& Lc = *m->layers[li];
    const LayerState& Lh = *m->layers[nl - 1];
    const bool expand = dedup && li == 0;
    const int rows_in = li == 0 ? p.rows0 : S * N, rows_out = S * N;
    ConvFusedArgs fa = conv_fused_shape(Lc, rows_in);
    fa.n_mod = li == 0 ? N : rows_in; fa.rep = expand ? S : 1;
    HeadUnitsArgs h = head_sweep_shape(ctx, Lh, nullptr, rows_out, rows_out, nullptr, col_ld(rows_out));
    head_units_plan(&h);
    const bool form = head_sweep_rides_form(ctx, Lh, h) && !(m->keep_state && m->grad_follows);
    if (li > 0 || p.first_one_launch) {
      // (the sweep's Kdiag slots per row are those of the plan WITH its Kzx units: the plan head_forward makes)
      static double kzx_placeholder;
      HeadUnitsArgs hk = h;
      hk.kzx = &kzx_placeholder;
      head_units_plan(&hk);
      int tail_rows = 0;
      p.ride_tail = conv_fused_head_tail(ctx, fa, m->keep_state, form, h.HWC, (long)head_units_lds(h), h.nfm, hk.n_kd, pipelined, p.chain_beside() && !p.reuse, &tail_rows);
      if (p.ride_tail > 0) p.ride_rows = tail_rows;
      else p.ride_rows = conv_fused_rides_head(ctx, fa, m->keep_state, form, h.HWC, (long)head_units_lds(h), h.nfm, pipelined, p.chain_beside() && !p.reuse);
    }
    if (p.ride_rows > 0 || p.ride_tail > 0) p.ride_layer = li;
  }
  return p;
}

// The parameter-only part of a step runs on the chain's / KL stream and names its scratch per model and bank: the chains / KL terms of two steps in flight
// may overlap, and with the deferred copy the tail launch reads the prior factor's diagonal out of this scratch at the END of the step -- another model's
// chain on the same ctx must not have overwritten it by then.  Both end here, whichever way that part returns: ctx->stream is the step's main stream and the
// tag is gone before a layer runs.  If the part failed, what it had enqueued on the two streams is waited for before the error goes up.
struct ChainScope {
  dcgp_ctx* ctx; const StepPlan& p; bool ok = false;
  ChainScope(dcgp_model* m, const StepPlan& plan) : ctx(m->ctx), p(plan) { ctx->stream = p.chain_s; ctx->ws_tag = "~m" + std::to_string(m->id) + "b" + std::to_string(p.bank); }
  ~ChainScope() {
    ctx->stream = p.main_s; ctx->ws_tag.clear();
    if (!ok) { hipStreamSynchronize(p.kl_s); hipStreamSynchronize(p.chain_s); }
  }
};

// Zero padding (dcgp_model_set_input_padding): the checks of a model's first forward, before anything is enqueued.  The layers were added with
// their padded H, W; what is checked is that the padded input of layer l is its predecessor's output plus the border.
int check_padding(dcgp_model* m) {
  if (!m->any_pad || m->pad_ok) return DCGP_OK;
  dcgp_ctx* ctx = m->ctx;
  const int nl = (int)m->layers.size();
  for (int li = 0; li < nl && li < 8; ++li) {
    const int p = m->pad[li];
    if (p == 0) continue;
    const LayerState& L = *m->layers[li];
    const dcgp_model::Geom gl = m->geom(li);   // (true sizes: a dilated layer's v is its phase geometry)
    if (p < 0) return ctx_fail(ctx, DCGP_ERR_ARG, "padding: layer %d has a negative padding (%d)", li, p);
    if (L.is_head && L.in_scale)   // (per-dimension lengthscales on the flattened input: --last-kernel rbf)
      return ctx_fail(ctx, DCGP_ERR_ARG, "padding: layer %d is a dense head, only conv layers and patch heads take padding", li);
    if (gl.H - 2 * p < 1 || gl.W - 2 * p < 1)
      return ctx_fail(ctx, DCGP_ERR_ARG, "padding: layer %d was added as %d x %d, smaller than its border of %d (add the layer with the padded size)", li,
                      gl.H, gl.W, p);
    if (li == 0) continue;
    const LayerState& B = *m->layers[li - 1];
    const dcgp_model::Geom gb = m->geom(li - 1);
    if (B.is_head || gb.Ho + 2 * p != gl.H || gb.Wo + 2 * p != gl.W || B.Rout != L.v.C)
      return ctx_fail(ctx, DCGP_ERR_ARG, "padding: layer %d takes %d x %d x %d, layer %d produces %d x %d x %d and the padding is %d", li, gl.H, gl.W, L.v.C,
                      li - 1, gb.Ho, gb.Wo, B.Rout, p);
  }
  m->pad_ok = true;
  return DCGP_OK;
}

// the padded copy of layer li's input (rows images of the predecessor's geometry) on `stream`: a workspace of the model, layer 0's per bank
int pad_input(dcgp_model* m, hipStream_t stream, int li, int bank, const double* src, long rows, const double** out) {
  dcgp_ctx* ctx = m->ctx;
  const LayerState& L = *m->layers[li];
  const int p = m->pad[li];
  const std::string name = "m" + std::to_string(m->id) + "_" + std::to_string(li) + "_Xpad" + (li == 0 ? "_b" + std::to_string(bank) : std::string());
  const dcgp_model::Geom g = m->geom(li);
  double* dst = (double*)ws_get(ctx, name, (size_t)rows * g.H * g.W * L.v.C * sizeof(double));
  if (!dst) return DCGP_ERR_ALLOC;
  DCGP_TRY(pad_images(ctx, stream, src, rows, g.H - 2 * p, g.W - 2 * p, L.v.C, p, dst));
  m->pad_in[li] = dst;
  *out = dst;
  return DCGP_OK;
}

// Dilation (dcgp_model_set_dilation): the checks of every forward of a model with a dilated layer, before anything is enqueued (a handful of
// integers; nothing is remembered, so no later call can make them stale).  The phase geometry in LayerState::v is this file's own doing; what is
// checked is that the layers around a dilated layer take and give its TRUE sizes: they size the split batch, the image-layout outputs and the
// reverse walk's buffers.
int check_dilation(dcgp_model* m) {
  if (!m->any_dil) return DCGP_OK;
  dcgp_ctx* ctx = m->ctx;
  const int nl = (int)m->layers.size();
  if (m->shard_global > 0)
    return ctx_fail(ctx, DCGP_ERR_ARG, "dilation: a sharded model (dcgp_model_set_shard) takes no dilated layer: the noise counters of the un-sharded batch are not laid out for the phase sub-images");
  for (int li = 0; li < nl && li < 8; ++li) {
    const int d = m->dil[li];
    if (d == 1) continue;
    const LayerState& L = *m->layers[li];
    const dcgp_model::Geom g = m->geom(li);
    if (L.is_head || L.v.s != 1 || g.Ho < 1 || g.Wo < 1 || (g.H + d - 1) / d != L.v.H || (g.W + d - 1) / d != L.v.W)   // (set_dilation's own checks)
      return ctx_fail(ctx, DCGP_ERR_ARG, "dilation: layer %d: dilation %d on %d x %d does not match its phase geometry %d x %d", li, d, g.H, g.W, L.v.H, L.v.W);
    const LayerState& A = *m->layers[li + 1];   // (a conv layer is never the last: the model has its head)
    const bool dense = A.is_head && A.v.H == 1 && A.v.W == 1;
    const dcgp_model::Geom ga = m->geom(li + 1);
    const int pa = li + 1 < 8 ? m->pad[li + 1] : 0;
    if (dense ? (long)A.v.C != g.P() * L.Rout : (ga.H - 2 * pa != g.Ho || ga.W - 2 * pa != g.Wo || A.v.C != L.Rout))
      return ctx_fail(ctx, DCGP_ERR_ARG, "dilation: layer %d takes %d x %d x %d with a padding of %d, layer %d (dilation %d) produces %d x %d x %d", li + 1,
                      ga.H, ga.W, A.v.C, pa, li, d, g.Ho, g.Wo, L.Rout);
    if (li == 0) continue;
    const LayerState& B = *m->layers[li - 1];
    const dcgp_model::Geom gb = m->geom(li - 1);
    const int p = m->pad[li];
    if (B.is_head || gb.Ho + 2 * p != g.H || gb.Wo + 2 * p != g.W || B.Rout != L.v.C)
      return ctx_fail(ctx, DCGP_ERR_ARG, "dilation: layer %d reads %d x %d x %d, layer %d produces %d x %d x %d and the padding is %d", li, g.H, g.W, L.v.C,
                      li - 1, gb.Ho, gb.Wo, B.Rout, p);
  }
  return DCGP_OK;
}

// the phase sub-images of layer li's (padded) input (rows images) on `stream`: a workspace of the model, layer 0's per bank
int split_input(dcgp_model* m, hipStream_t stream, int li, int bank, const double* src, long rows, const double** out) {
  dcgp_ctx* ctx = m->ctx;
  const LayerState& L = *m->layers[li];
  const int d = m->dil[li];
  const std::string name = "m" + std::to_string(m->id) + "_" + std::to_string(li) + "_Xs2b" + (li == 0 ? "_b" + std::to_string(bank) : std::string());
  const dcgp_model::Geom g = m->geom(li);
  double* dst = (double*)ws_get(ctx, name, (size_t)rows * d * d * L.v.H * L.v.W * L.v.C * sizeof(double));
  if (!dst) return DCGP_ERR_ALLOC;
  DCGP_TRY(s2b_images(ctx, stream, src, rows, g.H, g.W, L.v.C, d, dst));
  m->dil_in[li] = dst;
  *out = dst;
  return DCGP_OK;
}

// A dilated conv layer of the data path (run_layer's arguments; F: the phase sub-images split_input left, `rows` and `n_mod` still count images).
// conv_forward runs on rows * d^2 sub-images into phase-layout buffers (m->dil_out[li]; a mixed layer's latent triple stays in phase layout, the
// reverse pass reads it there), batch-to-space then writes outs[li] in image layout: what the next layer, the head and keep_outputs see.  The replicas
// of a de-duplicated first layer are phase-layout batches of N d^2 rows each, and [S][N d^2] is [S N][d^2]: one batch-to-space call covers them.
// Explicit noise arrives in image layout [rows][P R] and is split the same way, a phantom output's noise being zero.
int run_dilated_layer(dcgp_model* m, const StepPlan& p, const StepIn& in, int li, const double* F, int rows, int n_mod, int phase, int* out_rows_p) {
  dcgp_ctx* ctx = m->ctx;
  LayerState& L = *m->layers[li];
  const std::string pfx = model_pfx(m) + std::to_string(li) + "_";
  const int d = m->dil[li], dd = d * d;
  const dcgp_model::Geom g = m->geom(li);
  const bool expand = in.dedup && li == 0;
  const int out_rows = expand ? in.S * in.N : rows;
  if ((long)out_rows * dd > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "dilation: layer %d: %d rows x %d phases exceed 2^31 - 1", li, out_rows, dd);
  const long lat_width = (long)L.v.P * L.R;                       // per sub-image
  const size_t n_ph = (size_t)out_rows * dd * L.v.P * L.Rout;     // phase layout, phantoms included
  DCGP_TRY(ensure_out(m, li, out_rows, (int)(g.P() * L.Rout)));
  if (L.mix_W) DCGP_TRY(L.ensure_latent((size_t)out_rows * dd * lat_width));
  auto& o = m->outs[li];
  auto& ph = m->dil_out[li];
  ph.sample = (double*)ws_get(ctx, pfx + "dil_sample", n_ph * sizeof(double));
  if (!ph.sample) return DCGP_ERR_ALLOC;
  ph.mean = ph.var = nullptr;
  if (m->keep_outputs) {
    ph.mean = (double*)ws_get(ctx, pfx + "dil_mean", n_ph * sizeof(double));
    ph.var = (double*)ws_get(ctx, pfx + "dil_var", n_ph * sizeof(double));
    if (!ph.mean || !ph.var) return DCGP_ERR_ALLOC;
  }
  const double* z = in.zs ? in.zs[li] : nullptr;
  if (z && (phase & 2)) {
    double* zs = (double*)ws_get(ctx, pfx + "dil_z", (size_t)out_rows * dd * lat_width * sizeof(double));
    if (!zs) return DCGP_ERR_ALLOC;
    DCGP_TRY(s2b_images(ctx, ctx->stream, z, out_rows, g.Ho, g.Wo, L.R, d, zs));
    z = zs;
  }
  hipEvent_t fdone = (li == 0 && p.chain_beside()) ? m->ev_factor[p.bank] : nullptr;
  hipEvent_t pdone = p.chain_beside() ? m->ev_prep[p.bank][li] : nullptr;
  RngMap rm;   // (a sharded model takes no dilated layer: check_dilation)
  DCGP_TRY(conv_forward(ctx, L, F, rows * dd, n_mod * dd, expand ? in.S : 1, (long)in.N * dd * lat_width, z, in.seed, (uint32_t)(li + 1 + 64 * ctx->rank), m->jitter,
                        ph.sample, ph.mean, ph.var, pfx, fdone, pdone, phase, m->keep_state, &rm, li == 0 ? (int)p.first_one_launch : -1, nullptr, 0, 0));
  *out_rows_p = out_rows;
  if (!(phase & 2)) return DCGP_OK;
  DCGP_TRY(b2s_images(ctx, ctx->stream, ph.sample, 1, out_rows, g.Ho, g.Wo, L.Rout, d, o.sample));
  if (m->keep_outputs) {
    DCGP_TRY(b2s_images(ctx, ctx->stream, ph.mean, 1, out_rows, g.Ho, g.Wo, L.Rout, d, o.mean));
    DCGP_TRY(b2s_images(ctx, ctx->stream, ph.var, 1, out_rows, g.Ho, g.Wo, L.Rout, d, o.var));
  }
  return DCGP_OK;
}

// one layer of the data path on ctx->stream.  phase 1: only what needs Z alone (the layer's sweep, where it is a launch of its own), 2: the rest, 3: both.
// head_swept: whether the head's phase 1 launched anything (written by phase 1, read by phase 2).  kl: the KL pieces offered to the head (layer.h: KlOffer)
int run_layer(dcgp_model* m, const StepPlan& p, const StepIn& in, int li, const double* F, int rows, int n_mod, int phase, bool* head_swept, KlOffer* kl,
              int* out_rows_p) {
  dcgp_ctx* ctx = m->ctx;
  LayerState& L = *m->layers[li];
  const std::string pfx = model_pfx(m) + std::to_string(li) + "_";
  const double* z = in.zs ? in.zs[li] : nullptr;
  hipEvent_t fdone = (li == 0 && p.chain_beside()) ? m->ev_factor[p.bank] : nullptr;   // later layers are stream-ordered behind layer 0
  hipEvent_t pdone = p.chain_beside() ? m->ev_prep[p.bank][li] : nullptr;
  if (!L.is_head && m->dil_of(li) > 1) return run_dilated_layer(m, p, in, li, F, rows, n_mod, phase, out_rows_p);
  if (!L.is_head) {
    const int width = L.v.P * L.Rout, lat_width = L.v.P * L.R;   // channels leaving the layer / its GPs (the same unless the layer is mixed, mix.hip)
    const bool expand = in.dedup && li == 0;          // N distinct images -> S*N sampled rows
    const int out_rows = expand ? in.S * in.N : rows;
    DCGP_TRY(ensure_out(m, li, out_rows, width));
    if (L.mix_W) DCGP_TRY(L.ensure_latent((size_t)out_rows * lat_width));
    auto& o = m->outs[li];
    // device RNG: with a shard declared (dcgp_model_set_shard) every element draws at its counter in the un-sharded batch, one
    // stream per layer -- the step's value is then independent of the number of ranks; otherwise one stream per (layer, rank)
    RngMap rm;
    const bool sharded = m->shard_global > 0;
    if (sharded && (m->shard_global != in.N || m->shard_lo != 0)) { rm.W = lat_width; rm.Nl = in.N; rm.Ng = m->shard_global; rm.lo = m->shard_lo; }
    HeadUnitsArgs ride;
    if (li == p.ride_layer && (phase & 2)) {   // the head's Kzx rows ride this launch: the sweep head_forward would plan, on this layer's sample
      LayerState& Lh = *m->layers[li + 1];
      const long ldh = col_ld(out_rows);
      double* B = (double*)ws_get(ctx, model_pfx(m) + std::to_string(li + 1) + "_" + "Kzx", (size_t)Lh.Mp * ldh * sizeof(double));
      if (!B) return DCGP_ERR_ALLOC;
      ride = head_sweep_shape(ctx, Lh, o.sample, out_rows, out_rows, B, ldh);
      head_units_plan(&ride);
      if (p.ride_tail > 0) {   // the partial sums go where head_forward's conditional reads them
        ride.kd = (double*)ws_get(ctx, "kdiag_partial", (size_t)out_rows * ride.n_kd * sizeof(double));
        if (!ride.kd) return DCGP_ERR_ALLOC;
      }
    }
    DCGP_TRY(conv_forward(ctx, L, F, rows, n_mod, expand ? in.S : 1, (long)in.N * lat_width, z, in.seed, (uint32_t)(li + 1 + (sharded ? 0 : 64 * ctx->rank)),
                          m->jitter, o.sample, m->keep_outputs ? o.mean : nullptr, m->keep_outputs ? o.var : nullptr, pfx,
                          fdone, pdone, phase, m->keep_state, &rm, li == 0 ? (int)p.first_one_launch : -1,
                          (li == p.ride_layer && (phase & 2)) ? &ride : nullptr, p.ride_rows, p.ride_tail));
    *out_rows_p = out_rows;
    return DCGP_OK;
  }
  DCGP_TRY(ensure_out(m, li, rows, L.R));
  auto& o = m->outs[li];
  DCGP_TRY(ensure(ctx, &m->d_kd, &m->kd_cap, (size_t)rows));
  DCGP_TRY(head_forward(ctx, L, F, rows, n_mod, m->d_kd, o.mean, o.var, pfx, fdone, pdone,
                        phase == 1 ? 1 : (phase == 2 && *head_swept ? 2 : 0), phase == 1 ? head_swept : nullptr,
                        m->keep_state && m->grad_follows, kl, (p.ride_layer == li - 1 && p.ride_layer >= 0) ? (p.ride_tail > 0 ? rows : p.ride_rows) : 0,
                        p.ride_layer == li - 1 && p.ride_layer >= 0 && p.ride_tail > 0));
  *out_rows_p = rows;
  if (phase != 1 && m->keep_outputs) {
    // the head's sample is not needed by the ELBO; produce it only on request
    size_t n = (size_t)rows * L.R;
    if (z) {
      DCGP_TRY(reparam_async(ctx, o.mean, o.var, z, n, m->jitter, o.sample));
    } else {
      HIP_TRY(ctx, hipMemcpyAsync(o.sample, o.mean, n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
  }
  return DCGP_OK;
}

// The parameter-only chain on p.chain_s (inside a ChainScope): preparation, layer 0's early sweep where the plan has one, the factor groups, G / alpha of
// every layer.  *early0: layer 0's phase 1 is enqueued (the data path runs its phase 2).
int enqueue_chain(dcgp_model* m, const StepPlan& p, const StepIn& in, bool* early0, bool* head_swept) {
  dcgp_ctx* ctx = m->ctx;
  const int nl = (int)m->layers.size(), bank = p.bank;
  const bool beside = p.chain_beside();
  if (beside && m->done_valid[bank]) HIP_TRY(ctx, hipStreamWaitEvent(p.chain_s, m->done_ev[bank], 0));     // the bank's previous reader
  else if (beside && ctx->ev_last_valid) HIP_TRY(ctx, hipStreamWaitEvent(p.chain_s, ctx->ev_last, 0));    // first use: behind whatever ran last
  PrepArgs pa;
  pa.nl = nl;
  for (int li = 0; li < nl; ++li) pa.l[li] = m->layers[li]->prep_args(m->jitter);
  if (p.prep == PrepPlace::OnChain) {
    DCGP_TRY(prepare_all(ctx, pa));
    if (beside && !p.first_one_launch) HIP_TRY(ctx, hipEventRecord(m->ev_sweep[bank], p.chain_s));   // Z^T, |z|^2: what a sweep needs
  } else {
    if (p.prep == PrepPlace::SplitChainFirst) DCGP_TRY(prepare_all(ctx, pa, ~kPrepSweepTasks));
    ctx->stream = p.main_s;
    DCGP_TRY(prepare_all(ctx, pa, kPrepSweepTasks));
    ctx->stream = p.chain_s;
  }
  if (p.early_sweep) {
    ctx->stream = p.main_s;
    if (p.prep == PrepPlace::OnChain) HIP_TRY(ctx, hipStreamWaitEvent(p.main_s, m->ev_sweep[bank], 0));
    int out_rows = 0;
    DCGP_TRY(run_layer(m, p, in, 0, in.X, p.rows0, in.N, 1, head_swept, nullptr, &out_rows));
    *early0 = true;
    ctx->stream = p.chain_s;
  }
  if (p.prep == PrepPlace::SplitSweepFirst) DCGP_TRY(prepare_all(ctx, pa, ~kPrepSweepTasks));
  for (auto& gr : m->groups[bank]) DCGP_TRY(gr.run(ctx, p.defer, p.chain));
  if (beside) HIP_TRY(ctx, hipEventRecord(m->ev_factor[bank], p.chain_s));
  // G_r = inv(L) Lq_r and alpha = inv(L) q_mu of every layer: gate the second conditional GEMM
  bool made[8] = {}, rode[8] = {};
  for (int li = 0; li < nl; ++li) {   // layers whose right-hand sides rode the chain (build_groups): nothing left to do
    LayerState& L = *m->layers[li];
    bool live_sums = false, prior_sums = false;
    for (auto& gr : m->groups[bank]) {
      if (!gr.rode) continue;
      for (size_t i = 0; i < gr.K.size(); ++i) {
        if (gr.K[i] == L.g.K && (gr.rhs[i].Lq || gr.rhs[i].qmu)) { rode[li] = true; live_sums = gr.rhs[i].Lq != nullptr; }
        if (L.g.Kp && gr.K[i] == L.g.Kp && gr.rhs[i].Lq) prior_sums = true;
      }
    }
    if (!(made[li] = rode[li])) continue;
    L.g.klp_valid = live_sums; L.g.klpp_valid = prior_sums;
    L.g.kl_ns = chain_rhs_slots(L.Mp); L.g.kl_nsa = (L.Mp + 31) / 32;
  }
  GpMats* gs[8]; int wh[8]; bool hq[8];   // every other layer the one-launch route covers (unwhitened, M <= 256, <= 16 outputs): head_cond.hip
  for (int li = 0; li < nl; ++li) { gs[li] = &m->layers[li]->g; wh[li] = m->layers[li]->white; hq[li] = m->layers[li]->has_qsqrt; }
  DCGP_TRY(prep_solve_all(ctx, gs, wh, hq, nl, made, rode));
  for (int li = 0; li < nl; ++li) {
    if (!made[li]) DCGP_TRY(cond_prep(ctx, m->layers[li]->g, m->layers[li]->white, m->layers[li]->has_qsqrt));   // generic GEMMs
    if (beside) HIP_TRY(ctx, hipEventRecord(m->ev_prep[bank][li], p.chain_s));   // per layer: layer 0 does not wait for the others
  }
  return DCGP_OK;
}

// Where the KL pieces go (behind enqueue_chain, inside its ChainScope).  They need nothing but parameter-only state.  Where the chain left the sums of
// squares they are made of (every layer unwhitened, M <= 256, with q_sqrt), one extra workgroup per layer of the tail launch -- or of the head's one-launch
// conditional (enqueue_layers) -- adds them up with the factors' log-determinants: no KL launches, no stream of their own, no fork in front of the first
// layer and no join (tail_dev.h); m->kl_in_tail / m->kl_tail of the bank say so to the tail.  Otherwise (and with option kl_side) their own launches, on
// the KL stream: *join = the main stream must wait for ev_kl of the bank.
int place_kl(dcgp_model* m, const StepPlan& p, bool need_kl, double* scal, bool* join) {
  dcgp_ctx* ctx = m->ctx;
  const int nl = (int)m->layers.size(), bank = p.bank;
  bool in_tail = need_kl && !ctx->opt.kl_side;
  for (int li = 0; li < nl && in_tail; ++li) {   // (the sums are valid where this step's chain or prep_solve left them with G / alpha)
    const LayerState& L = *m->layers[li];
    in_tail = !L.white && L.has_qsqrt && L.g.klp_valid && (!L.g.Kp || L.g.klpp_valid);
  }
  m->kl_in_tail[bank] = in_tail;
  if (in_tail) {
    KlTail& kt = m->kl_tail[bank];
    kt.nl = nl;
    const auto it = p.defer ? ctx->ws.find("chol_Lout" + ctx->ws_tag) : ctx->ws.end();   // deferred copy: the factors are still in the chain's scratch,
    const double* lout = it != ctx->ws.end() ? (const double*)it->second.first : nullptr;      // [matrix of the group][Mp][Mp]
    for (int li = 0; li < nl; ++li) {
      const LayerState& L = *m->layers[li];
      KlTailLayer& q = kt.l[li];
      const double* prior = L.g.Kp ? L.g.Kp : L.g.K;
      q.Lfac = prior; q.ldf = L.Mp;
      if (p.defer) {
        const auto& gr = m->groups[bank][0];
        long idx = -1;
        for (size_t i = 0; i < gr.K.size(); ++i) if (gr.K[i] == prior) idx = (long)i;
        if (!lout || idx < 0) return ctx_fail(ctx, DCGP_ERR_ARG, "model: factor scratch of layer %d not found", li);
        q.Lfac = lout + idx * (long)L.Mp * L.Mp;
      }
      q.Lq = L.g.Lq; q.sums = L.g.Kp ? L.g.klpp : L.g.klp; q.M = L.M; q.Mp = L.Mp; q.R = L.R;
      q.ns = L.g.kl_ns; q.nsa = L.g.kl_nsa;
    }
  }
  if (!need_kl || in_tail) return DCGP_OK;
  if (p.kl_s != p.chain_s) {   // fork: the KL terms need the factors only, the main stream goes on with the layers
    if (!p.chain_beside()) HIP_TRY(ctx, hipEventRecord(m->ev_prep[bank][nl - 1], p.chain_s));   // (a chain beside the main stream has recorded it)
    HIP_TRY(ctx, hipStreamWaitEvent(p.kl_s, m->ev_prep[bank][nl - 1], 0));
    ctx->stream = p.kl_s;
  }
  for (auto& gr : m->groups[bank]) DCGP_TRY(gr.finish(ctx));   // the factor back over K (deferred copy): the KL terms read its diagonal
  for (int li = 0; li < nl; ++li) {
    LayerState& L = *m->layers[li];
    const double* Lp = L.g.Kp ? L.g.Kp : L.g.K;
    const double* LpinvT = L.g.Kp ? L.g.LpinvT : L.g.LinvT;
    DCGP_TRY(kl_layer(ctx, L.g, Lp, LpinvT, L.white, (model_pfx(m) + std::to_string(li)).c_str(), scal + 4 + 4 * li));
  }
  *join = p.kl_s != p.main_s;
  if (*join) HIP_TRY(ctx, hipEventRecord(m->ev_kl[bank], ctx->stream));
  return DCGP_OK;
}

// The data path over the layers on p.main_s, with the join of the KL stream.
int enqueue_layers(dcgp_model* m, const StepPlan& p, const StepIn& in, bool early0, bool head_swept, bool kl_join, double* scal, int* rows_last) {
  dcgp_ctx* ctx = m->ctx;
  const int nl = (int)m->layers.size(), bank = p.bank;
  // sweeps read Z^T / |z|^2 of this bank (a one-launch first layer waits for its G / alpha, recorded behind them on the same stream)
  if (p.chain_beside() && !p.first_one_launch && p.prep == PrepPlace::OnChain) HIP_TRY(ctx, hipStreamWaitEvent(p.main_s, m->ev_sweep[bank], 0));
  const double* F = in.X;
  int rows = p.rows0, n_mod = in.N;
  // Join the side stream where the wait is already satisfied when the main stream gets to it: in front of the last layer when
  // other layers precede it (the KL terms finish beside the first of them), behind it otherwise.  In front of the tail kernel
  // the wait packet sat between two short launches at the very end of the step (6 us).
  const bool join_early = nl > 1;
  // the KL pieces ride the head's one-launch conditional where there is one (head_cond.hip); m->kl_rode[bank] says whether they did
  KlOffer offer{&m->kl_tail[bank], scal};
  for (int li = 0; li < nl; ++li) {
    const bool last = li == nl - 1;
    int out_rows = 0;
    if (last && join_early && kl_join) HIP_TRY(ctx, hipStreamWaitEvent(p.main_s, m->ev_kl[bank], 0));
    if (li > 0 && m->pad[li] > 0) DCGP_TRY(pad_input(m, p.main_s, li, bank, F, rows, &F));   // (layer 0's: forward_all)
    if (li > 0 && m->dil_of(li) > 1) DCGP_TRY(split_input(m, p.main_s, li, bank, F, rows, &F));   // pad, then split (layer 0's: forward_all)
    DCGP_TRY(run_layer(m, p, in, li, F, rows, n_mod, (li == 0 && early0) ? 2 : 3, &head_swept,
                       (last && in.need_kl && m->kl_in_tail[bank]) ? &offer : nullptr, &out_rows));
    if (li == 0 && m->gkl_state && p.mark == ForkMark::BehindFirstLayer)
      HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, p.main_s));   // (the chain's results are ordered in front of this layer)
    if (!m->layers[li]->is_head) F = m->outs[li].sample;
    rows = n_mod = out_rows;
  }
  m->kl_rode[bank] = offer.carried;
  if (!join_early && kl_join) HIP_TRY(ctx, hipStreamWaitEvent(p.main_s, m->ev_kl[bank], 0));   // join the side stream
  *rows_last = rows;
  return DCGP_OK;
}

// layers 0..n-1 forward; leaves ctx->stream on the main stream the step runs on (the caller holds a StreamGuard).
int forward_all(dcgp_model* m, const double* X, int N, int S, const double* const* zs, uint64_t seed, int dedup,
                bool need_kl, bool pipelined, int* rows_last) {
  dcgp_ctx* ctx = m->ctx;
  if (!m->has_head) return ctx_fail(ctx, DCGP_ERR_ARG, "model has no head layer");
  const int nl = (int)m->layers.size();
  if (nl > 8) return ctx_fail(ctx, DCGP_ERR_ARG, "at most 8 layers supported");
  // a local batch that overran its declared shard would draw the noise of the NEXT sample's images (the counters are laid out by the
  // un-sharded batch): correlated samples, not an error anyone would see.  Only the ELBO / gradient paths (need_kl) are bound by the
  // declared training shard: propagate / predict_y take any batch (an AccuracyLogger's batches on rank 3 of 4), their counter layout
  // does not matter
  if (need_kl && m->shard_global > 0 && (long)m->shard_lo + N > m->shard_global)
    return ctx_fail(ctx, DCGP_ERR_ARG, "forward: %d images from image %d on overrun the declared global batch of %d (dcgp_model_set_shard)", N,
                    m->shard_lo, m->shard_global);
  DCGP_TRY(check_padding(m));
  DCGP_TRY(check_dilation(m));
  for (int li = 0; li + 1 < nl; ++li) {   // a mixed layer's maps are the next layer's channels (a dense head's single patch: all of them)
    const LayerState &A = *m->layers[li], &B = *m->layers[li + 1];
    const bool dense = B.is_head && B.v.H == 1 && B.v.W == 1;
    if (A.mix_W && B.v.C != (dense ? m->geom(li).P() : 1) * A.Rout)
      return ctx_fail(ctx, DCGP_ERR_ARG, "forward: layer %d is mixed into %d maps, layer %d takes C = %d channels", li, A.Rout, li + 1, B.v.C);
  }
  DCGP_TRY(ensure_events(m));
  const StepPlan p = plan_step(m, N, S, dedup, need_kl, pipelined);
  StepIn in{X, N, S, zs, seed, dedup, need_kl};
  if (!p.reuse) m->chain_version = 0;   // (stays 0 if this step fails on the way)
  m->bank = p.bank;
  for (auto& l : m->layers) DCGP_TRY(l->use_bank(p.bank));
  DCGP_TRY(build_groups(m, p.bank));
  if (!m->d_scal && dev_alloc(ctx, (void**)&m->d_scal, 128 * sizeof(double), "d_scal") != hipSuccess)
    return ctx_fail(ctx, DCGP_ERR_ALLOC, "model: allocation failed");
  double* scal = m->d_scal + 64 * p.bank;
  m->outs.resize(nl);
  // a step on the other main stream than the previous one starts behind it
  if (ctx->ev_last_valid && ctx->last_main != p.main_s) HIP_TRY(ctx, hipStreamWaitEvent(p.main_s, ctx->ev_last, 0));
  ctx->last_main = p.main_s;
  // a padded first layer: X is padded once, here -- the early sweep, the de-duplicated first layer and the replicas of a tiled batch then read an
  // ordinary image.  Per bank: two steps may be in flight.
  if (m->pad[0] > 0) DCGP_TRY(pad_input(m, p.main_s, 0, p.bank, X, N, &in.X));
  // a dilated first layer: the (padded) batch is split into its phase sub-images once, here, for the same readers
  if (m->dil[0] > 1) DCGP_TRY(split_input(m, p.main_s, 0, p.bank, in.X, N, &in.X));

  bool early0 = false, head_swept = false, kl_join = false;
  if (p.reuse) ++m->chain_skips;   // (never pipelined: p.main_s is ctx->stream as the caller left it)
  else {
    ChainScope scope(m, p);
    DCGP_TRY(enqueue_chain(m, p, in, &early0, &head_swept));
    DCGP_TRY(place_kl(m, p, need_kl, scal, &kl_join));
    scope.ok = true;
  }
  if (!p.reuse && !pipelined && !m->grad_follows && (!m->keep_state || m->data_grad)) { m->chain_version = m->param_version; m->chain_with_kl = need_kl; }
  // a training step: see ForkMark.  1 = the side stream itself holds the parameter-only chain (not here), 2 = it waits for ctx->ev_fork
  m->gkl_state = (m->grad_follows && !pipelined && grad_kl_early(m, false, false) == 1) ? 2 : 0;
  if (m->gkl_state && p.mark == ForkMark::BehindChain) HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, p.chain_s));
  // with the chain on a side stream a mark on the MAIN stream orders layer 0's operands only: grad_kl_early also waits for the G / alpha
  // of the other layers (cond_prep of whitened / M > 256 layers runs behind ev_prep[0] on that stream)
  m->gkl_prep_wait = (m->gkl_state && p.mark == ForkMark::BehindFirstLayer && p.chain_beside()) ? nl : 0;
  return enqueue_layers(m, p, in, early0, head_swept, kl_join, scal, rows_last);
}

// The end of a step's data path on its main stream: `ev` (already recorded there, behind the step's last command) frees the
// bank for its next writer and lets a step on the other main stream start.  ev == nullptr: the caller synchronises the stream
// itself before anything else is enqueued.
int forward_done(dcgp_model* m, hipEvent_t ev) {
  dcgp_ctx* ctx = m->ctx;
  m->done_ev[m->bank] = ev;
  m->done_valid[m->bank] = ev != nullptr;
  ctx->ev_last = ev;
  ctx->ev_last_valid = ev != nullptr;
  return DCGP_OK;
}

}  // namespace

extern "C" {

int dcgp_model_create(dcgp_ctx* ctx, int num_samples, double jitter, dcgp_model** out) {
  if (!ctx || !out || num_samples <= 0 || !(jitter >= 0.0)) return ctx ? ctx_fail(ctx, DCGP_ERR_ARG, "model_create: bad args") : DCGP_ERR_ARG;
  dcgp_model* m = new dcgp_model();
  m->ctx = ctx; m->S = num_samples; m->jitter = jitter; m->id = ++g_model_counter;
  *out = m;
  return DCGP_OK;
}

int dcgp_model_destroy(dcgp_model* model) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  hipDeviceSynchronize();   // every stream: the model's workspaces may still be in use
  ctx->ev_last = nullptr;   // (it may be one of this model's result-ring events; nothing is in flight any more)
  ctx->ev_last_valid = false;
  // the per-model workspaces of the forward / reverse pass live in the ctx under "m<id>_..." (the training step's are large:
  // R x M x columns doubles per conv layer); they go with the model
  const std::string pfx = "m" + std::to_string(model->id) + "_";
  const std::string tag = "~m" + std::to_string(model->id) + "b";   // the chain's scratch (forward_all's ws_tag)
  for (auto it = ctx->ws.begin(); it != ctx->ws.end();) {
    if (it->first.compare(0, pfx.size(), pfx) == 0 || it->first.find(tag) != std::string::npos) {
      dev_free(ctx, it->second.first);
      it = ctx->ws.erase(it);
    } else {
      ++it;
    }
  }
  if (ctx->ws_tag.find(tag) != std::string::npos) ctx->ws_tag.clear();   // operator calls behind this model must not name scratch after it
  delete model;
  return DCGP_OK;
}

int dcgp_model_set_shard(dcgp_model* model, int first_image, int global_batch) {
  if (!model) return DCGP_ERR_ARG;
  if (global_batch < 0 || first_image < 0 || (global_batch > 0 && first_image >= global_batch))
    return ctx_fail(model->ctx, DCGP_ERR_ARG, "set_shard: first image %d of a global batch of %d", first_image, global_batch);
  if (global_batch > 0 && model->any_dil)
    return ctx_fail(model->ctx, DCGP_ERR_ARG, "set_shard: the model has a dilated layer (dcgp_model_set_dilation); a sharded model takes none");
  model->shard_lo = first_image; model->shard_global = global_batch;
  return DCGP_OK;
}

int dcgp_model_set_dilation(dcgp_model* model, int layer, int d) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (layer < 0 || layer >= (int)model->layers.size() || layer >= 8) return ctx_fail(ctx, DCGP_ERR_ARG, "set_dilation: no layer %d", layer);
  if (d < 1) return ctx_fail(ctx, DCGP_ERR_ARG, "set_dilation: layer %d: the dilation must be >= 1, got %d", layer, d);
  LayerState& L = *model->layers[layer];
  if (d > 1 && L.is_head) return ctx_fail(ctx, DCGP_ERR_ARG, "set_dilation: layer %d is the head, only conv layers take a dilation", layer);
  if (d > 1 && L.v.s != 1) return ctx_fail(ctx, DCGP_ERR_ARG, "set_dilation: layer %d has stride %d, a dilated layer has stride 1", layer, L.v.s);
  if (d > 1 && model->shard_global > 0)
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_dilation: layer %d: a sharded model (dcgp_model_set_shard) takes no dilated layer", layer);
  if (model->enq_seq != model->col_seq) return ctx_fail(ctx, DCGP_ERR_ARG, "set_dilation: enqueued steps are still to be collected");
  if (d == model->dil[layer]) return DCGP_OK;
  const dcgp_model::Geom g = model->geom(layer);   // the true (padded) size: the layer was added with it
  const int span = d * (L.v.f - 1) + 1;
  if (span > g.H || span > g.W)
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_dilation: layer %d: a window of %d taps %d apart spans %d pixels, its padded input is %d x %d", layer, L.v.f, d,
                    span, g.H, g.W);
  // the patch count is part of the layout of the layer's gradient block, which is fixed by the first reverse pass or sharded step
  if (L.gZ || L.pstage || L.hyp)
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_dilation: layer %d has taken a gradient step; set its dilation before the first", layer);
  model->dil_H[layer] = g.H; model->dil_W[layer] = g.W;
  model->dil[layer] = d;
  L.v.set((g.H + d - 1) / d, (g.W + d - 1) / d, L.v.C, L.v.f, 1);   // what the kernels see from here on: the phase geometry (d == 1: the true size again)
  model->any_dil = false;
  for (int q : model->dil) model->any_dil = model->any_dil || q != 1;
  model->pad_ok = false;    // the padding chain reads the true sizes
  return DCGP_OK;
}

int dcgp_model_set_input_padding(dcgp_model* model, int layer, int pad) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (layer < 0 || layer >= (int)model->layers.size() || layer >= 8) return ctx_fail(ctx, DCGP_ERR_ARG, "set_input_padding: no layer %d", layer);
  if (pad < 0) return ctx_fail(ctx, DCGP_ERR_ARG, "set_input_padding: layer %d: the padding must be >= 0, got %d", layer, pad);
  const dcgp_model::Geom v = model->geom(layer);   // (the true size: a dilated layer's own v is its phase geometry)
  if (v.H - 2 * pad < 1 || v.W - 2 * pad < 1)
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_input_padding: layer %d was added as %d x %d, smaller than its border of %d (add the layer with the padded size)",
                    layer, v.H, v.W, pad);
  if (model->enq_seq != model->col_seq) return ctx_fail(ctx, DCGP_ERR_ARG, "set_input_padding: enqueued steps are still to be collected");
  if (layer == 0 && model->ds_X && pad != model->pad[0])
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_input_padding: a dataset is attached (its image length follows layer 0's padding); detach it first");
  model->pad[layer] = pad;
  model->any_pad = false;
  for (int p : model->pad) model->any_pad = model->any_pad || p != 0;
  model->pad_ok = false;   // checked against the neighbouring layers at the next forward
  return DCGP_OK;
}

int dcgp_model_set_keep_outputs(dcgp_model* model, int on) {
  if (!model) return DCGP_ERR_ARG;
  model->keep_outputs = on != 0;
  return DCGP_OK;
}

int dcgp_model_add_conv_layer(dcgp_model* model, int H, int W, int C, int f, int stride, int M, int R, int white,
                              int identity_mean, double variance, double lengthscale, const double* Z_host,
                              const double* Z0_host, const double* q_mu_host, const double* q_sqrt_host) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (model->has_head) return ctx_fail(ctx, DCGP_ERR_ARG, "conv layers must be added before the head");
  if (identity_mean && (f % 2 == 0)) return ctx_fail(ctx, DCGP_ERR_ARG, "Conv2dMean supports odd filter sizes only");
  std::unique_ptr<LayerState> L(new LayerState());
  DCGP_TRY(L->init(ctx, false, H, W, C, f, stride, M, R, white, identity_mean, 0, variance, lengthscale));
  DCGP_TRY(L->upload(L->Z, Z_host, (size_t)M * L->v.L));
  DCGP_TRY(L->upload(L->Z0, Z0_host ? Z0_host : Z_host, (size_t)M * L->v.L));
  DCGP_TRY(L->upload(L->q_mu, q_mu_host, (size_t)M * R));
  DCGP_TRY(L->upload(L->q_sqrt, q_sqrt_host, (size_t)R * M * M));
  model->layers.push_back(std::move(L));
  model->groups_built[0] = model->groups_built[1] = false;
  return DCGP_OK;
}

int dcgp_model_set_head(dcgp_model* model, int H, int W, int C, int f, int stride, int M, int R, int white,
                        int kernel_type, double variance, double lengthscale, const double* Z_host, const double* w_host,
                        const double* q_mu_host, const double* q_sqrt_host) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (model->has_head) return ctx_fail(ctx, DCGP_ERR_ARG, "head already set");
  if (kernel_type != 0 && kernel_type != 1) return ctx_fail(ctx, DCGP_ERR_ARG, "Invalid last layer kernel");
  std::unique_ptr<LayerState> L(new LayerState());
  DCGP_TRY(L->init(ctx, true, H, W, C, f, stride, M, R, white, 0, kernel_type, variance, lengthscale));
  DCGP_TRY(L->upload(L->Z, Z_host, (size_t)M * L->v.L));
  DCGP_TRY(L->upload(L->w, w_host, (size_t)L->v.P));
  DCGP_TRY(L->upload(L->q_mu, q_mu_host, (size_t)M * R));
  DCGP_TRY(L->upload(L->q_sqrt, q_sqrt_host, (size_t)R * M * M));
  model->layers.push_back(std::move(L));
  model->has_head = true;
  model->groups_built[0] = model->groups_built[1] = false;
  return DCGP_OK;
}

int dcgp_model_set_factor_reuse(dcgp_model* model, int mode) {
  if (!model || mode < 0 || mode > 2) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "set_factor_reuse: mode 0, 1 or 2") : DCGP_ERR_ARG;
  model->factor_reuse = mode;
  return DCGP_OK;
}
int dcgp_model_chain_skips(dcgp_model* model, uint64_t* out) {
  if (!model || !out) return DCGP_ERR_ARG;
  *out = model->chain_skips;
  return DCGP_OK;
}
int dcgp_model_factor_groups(dcgp_model* model, int cap, int* count_out, int* Mp_out, int* matrices_out, int* riding_out) {
  if (!model || !count_out || cap < 0 || (cap > 0 && (!Mp_out || !matrices_out || !riding_out))) return DCGP_ERR_ARG;
  const auto& groups = model->groups[model->bank];
  *count_out = (int)groups.size();
  for (int q = 0; q < cap && q < (int)groups.size(); ++q) {
    int riding = 0;
    for (const auto& r : groups[q].rhs) riding += (groups[q].rode && (r.Lq || r.qmu)) ? 1 : 0;
    Mp_out[q] = groups[q].Mp; matrices_out[q] = (int)groups[q].K.size(); riding_out[q] = riding;
  }
  return DCGP_OK;
}

int dcgp_model_set_param(dcgp_model* model, int layer, const char* which, const double* value_host, size_t count) {
  // (whatever becomes of the call: the parameter-only state of earlier steps is not reused -- but for the mean filter, which is no input of it)
  if (model && !(which && !strcmp(which, "mean_filter"))) ++model->param_version;
  if (!model || !which || !value_host) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (!strcmp(which, "likelihood_epsilon")) {   // model-wide, `layer` is ignored
    if (count != 1 || !(value_host[0] > 0 && value_host[0] < 1)) return ctx_fail(ctx, DCGP_ERR_ARG, "set_param(likelihood_epsilon): one value in (0, 1)");
    model->eps = value_host[0];
    return DCGP_OK;
  }
  if (!strcmp(which, "likelihood_variance")) {   // model-wide, `layer` is ignored
    if (model->lik_kind != 1) return ctx_fail(ctx, DCGP_ERR_ARG, "set_param(likelihood_variance): not a Gaussian-likelihood model");
    if (count != 1 || !(value_host[0] > 1e-6)) return ctx_fail(ctx, DCGP_ERR_ARG, "set_param(likelihood_variance): one value > 1e-6");
    HIP_TRY(ctx, hipMemcpyAsync(model->d_lik, value_host, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DCGP_OK;
  }
  if (!strcmp(which, "likelihood_scale")) {   // model-wide, `layer` is ignored
    if (model->lik_kind != 4) return ctx_fail(ctx, DCGP_ERR_ARG, "set_param(likelihood_scale): not a StudentT-likelihood model");
    if (count != 1 || !(value_host[0] > 1e-6)) return ctx_fail(ctx, DCGP_ERR_ARG, "set_param(likelihood_scale): one value > 1e-6");
    HIP_TRY(ctx, hipMemcpyAsync(model->d_lik, value_host, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DCGP_OK;
  }
  if (layer < 0 || layer >= (int)model->layers.size()) return ctx_fail(ctx, DCGP_ERR_ARG, "set_param: no layer %d", layer);
  LayerState& L = *model->layers[layer];
  auto expect = [&](size_t n) { return count == n ? DCGP_OK : ctx_fail(ctx, DCGP_ERR_ARG, "set_param(%s): expected %zu values, got %zu", which, n, count); };
  if (!strcmp(which, "Z")) { DCGP_TRY(expect((size_t)L.M * L.v.L)); return L.upload(L.Z, value_host, count); }
  if (!strcmp(which, "Z0")) {
    if (!L.Z0) return ctx_fail(ctx, DCGP_ERR_ARG, "set_param: the head has no frozen prior Z");
    DCGP_TRY(expect((size_t)L.M * L.v.L)); return L.upload(L.Z0, value_host, count);
  }
  if (!strcmp(which, "q_mu")) { DCGP_TRY(expect((size_t)L.M * L.R)); return L.upload(L.q_mu, value_host, count); }
  if (!strcmp(which, "q_sqrt")) { DCGP_TRY(expect((size_t)L.R * L.M * L.M)); return L.upload(L.q_sqrt, value_host, count); }
  if (!strcmp(which, "w")) {
    if (!L.w) return ctx_fail(ctx, DCGP_ERR_ARG, "set_param: only the head has patch weights");
    DCGP_TRY(expect((size_t)L.v.P)); return L.upload(L.w, value_host, count);
  }
  if (!strcmp(which, "mean_filter")) {
    if (!L.mean_W) return ctx_fail(ctx, DCGP_ERR_ARG, "set_param(mean_filter): layer %d has no mean filter (dcgp_model_set_mean_filter)", layer);
    DCGP_TRY(expect(L.mean_slots())); return L.upload(L.mean_W, value_host, count);
  }
  if (!strcmp(which, "mixing")) {
    if (!L.mix_W) return ctx_fail(ctx, DCGP_ERR_ARG, "set_param(mixing): layer %d is not mixed (dcgp_model_set_mixing)", layer);
    DCGP_TRY(expect(L.mix_slots())); return L.upload(L.mix_W, value_host, count);
  }
  if (!strcmp(which, "variance")) { DCGP_TRY(expect(1)); if (!(value_host[0] > 0)) return ctx_fail(ctx, DCGP_ERR_ARG, "variance must be > 0"); L.variance = value_host[0]; return DCGP_OK; }
  if (!strcmp(which, "lengthscale")) { DCGP_TRY(expect(1)); if (!(value_host[0] > 0)) return ctx_fail(ctx, DCGP_ERR_ARG, "lengthscale must be > 0"); L.ls = value_host[0]; return DCGP_OK; }
  if (!strcmp(which, "ard_lengthscales")) {
    // gpflow RBF(D, ARD=True) on the flattened features (--last-kernel rbf, conv_gp/models.py:160-168): a head whose
    // single patch is the whole input (P == 1); x / l and Z / l are formed while the operands are staged
    // A conv layer (gpflow RBF(f f C, ARD=True) as its base kernel): one lengthscale per patch element; the patch sweep scales the gathered patch
    // (rbf.hip: patch_rbf_body ARD), the preparation scales Z for both Gram matrices, Z^T and |z|^2 (prep.hip: the SC forms).
    if (L.is_head && L.v.P != 1) return ctx_fail(ctx, DCGP_ERR_ARG, "set_param(ard_lengthscales): only a single-patch head takes per-dimension lengthscales");
    if (!L.is_head && L.base_type != 0)
      return ctx_fail(ctx, DCGP_ERR_ARG, "set_param(ard_lengthscales): layer %d: only the RBF base kernel takes per-dimension lengthscales", layer);
    DCGP_TRY(expect((size_t)L.v.L));
    // the lengthscales' gradient lies inside the layer's gradient block, whose layout is fixed by the first reverse pass or sharded step
    if (!L.is_head && !L.ard && (L.gZ || L.pstage || L.hyp))
      return ctx_fail(ctx, DCGP_ERR_ARG, "set_param(ard_lengthscales): layer %d: set the lengthscales before the model's first training step", layer);
    std::vector<double> inv(count);
    for (size_t i = 0; i < count; ++i) {
      if (!(value_host[i] > 0)) return ctx_fail(ctx, DCGP_ERR_ARG, "lengthscales must be > 0");
      inv[i] = 1.0 / value_host[i];
    }
    if (!L.in_scale && !(L.in_scale = L.dalloc(count))) return ctx_fail(ctx, DCGP_ERR_ALLOC, "layer: device allocation failed");
    if (!L.ard && !(L.ard = L.dalloc(count))) return ctx_fail(ctx, DCGP_ERR_ALLOC, "layer: device allocation failed");
    L.ls = 1.0;
    DCGP_TRY(L.upload(L.ard, value_host, count));
    return L.upload(L.in_scale, inv.data(), count);
  }
  if (!strcmp(which, "base_kernel")) {   // {type, variance, p1, p2}: 0 = RBF (p1 = lengthscale), 1 = ArcCosine order 0 (p1 = weight, p2 = bias variance),
                                         // 2 = Matern32, 3 = Matern52 (p1 = lengthscale)
    DCGP_TRY(expect(4));
    const int type = (int)value_host[0];
    if (type < 0 || type > 3 || (double)type != value_host[0] || !(value_host[1] > 0) || !(value_host[2] > 0) || (type == 1 && !(value_host[3] >= 0)))
      return ctx_fail(ctx, DCGP_ERR_ARG, "set_param(base_kernel): bad kernel description");
    if (type != 0 && L.is_head) return ctx_fail(ctx, DCGP_ERR_ARG, "set_param(base_kernel): the head kernels are RBF-based (conv_gp/models.py:160-187)");
    L.base_type = type; L.variance = value_host[1];
    if (type != 1) L.ls = value_host[2]; else { L.acos_w = value_host[2]; L.acos_b = value_host[3]; }
    return DCGP_OK;
  }
  return ctx_fail(ctx, DCGP_ERR_ARG, "set_param: unknown parameter '%s'", which);
}

int dcgp_elbo_forward(dcgp_model* model, const double* X, const int32_t* y, int N, double scale,
                      const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0, double* out_host,
                      int* info_host) {
  return elbo_forward_impl(model, X, y, N, scale, z_per_layer_host, seed, dedup_layer0, out_host, info_host);   // (a Gaussian model: DCGP_ERR_ARG)
}

int dcgp_elbo_forward_enqueue(dcgp_model* model, const double* X, const int32_t* y, int N, double scale,
                              const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0, uint64_t* ticket) {
  // the caller means to keep steps in flight: data path and parameter-only chain on disjoint CUs (forward_all)
  return elbo_forward_enqueue_impl(model, X, y, N, scale, z_per_layer_host, seed, dedup_layer0, ticket, true);
}

int dcgp_elbo_forward_collect(dcgp_model* model, uint64_t ticket, double* out_host, int* info_host) {
  return elbo_forward_collect_impl(model, ticket, out_host, info_host);
}

int dcgp_elbo_forward_f64y(dcgp_model* model, const double* X, const double* y, int N, double scale,
                           const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0, double* out_host,
                           int* info_host) {
  if (model && !y) return ctx_fail(model->ctx, DCGP_ERR_ARG, "elbo_forward_f64y: y is NULL");
  return elbo_forward_impl(model, X, nullptr, N, scale, z_per_layer_host, seed, dedup_layer0, out_host, info_host, y);
}

int dcgp_elbo_forward_enqueue_f64y(dcgp_model* model, const double* X, const double* y, int N, double scale,
                                   const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0, uint64_t* ticket) {
  if (model && !y) return ctx_fail(model->ctx, DCGP_ERR_ARG, "elbo_forward_enqueue_f64y: y is NULL");
  return elbo_forward_enqueue_impl(model, X, nullptr, N, scale, z_per_layer_host, seed, dedup_layer0, ticket, true, y);
}

int dcgp_model_set_likelihood(dcgp_model* model, int kind, double variance) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (kind < 0 || kind > 3) return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood: kind 0 (RobustMax), 1 (Gaussian), 2 (Bernoulli) or 3 (Softmax), got %d", kind);
  if (kind == 1 && !(variance > 1e-6)) return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood: the Gaussian variance must be > 1e-6 (softplus + 1e-6)");
  if (!model->has_head) return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood: set the head first");
  LayerState& H = *model->layers.back();
  if (H.gZ && model->lik_kind != kind) return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood: the likelihood is fixed once a gradient was taken");
  if (model->enq_seq != model->col_seq) return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood: enqueued steps are still to be collected");
  // Softmax is chosen in place of the default RobustMax: a model already switched to float64 targets keeps them
  if (kind == 3 && model->lik().float_targets())
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood: kind 3 (Softmax) takes int32 labels, this model was set to a float64-target likelihood (kind %d)", model->lik_kind);
  if (kind == 3 && H.R < 2) return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood: the Softmax likelihood needs K >= 2 classes, the head has %d outputs", H.R);
  if (kind != 3) model->lik_Q = 0;   // (a node table belongs to the Softmax likelihood it was set on)
  ++model->param_version;
  model->lik_kind = kind;
  H.lik_slots = kind == 1 ? 1 : 0;   // (only the Gaussian variance takes a slot: a Bernoulli block is a RobustMax one)
  if (kind != 1) return DCGP_OK;
  if (!model->d_lik) {   // {variance, Adam m, Adam v}
    if (dev_alloc(ctx, (void**)&model->d_lik, 3 * sizeof(double), "d_lik") != hipSuccess) return ctx_fail(ctx, DCGP_ERR_ALLOC, "set_likelihood: device allocation failed");
    const double init[3] = {variance, 0.0, 0.0};
    HIP_TRY(ctx, hipMemcpyAsync(model->d_lik, init, sizeof init, hipMemcpyHostToDevice, ctx->stream));
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(model->d_lik, &variance, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

int dcgp_model_set_likelihood_params(dcgp_model* model, int kind, const double* params_host, int n) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (kind != 4 && kind != 5) return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood_params: kind 4 (StudentT) or 5 (Poisson), got %d (dcgp_model_set_likelihood sets the others)", kind);
  if (!params_host || n != (kind == 4 ? 2 : 1))
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood_params: kind %d takes %s", kind, kind == 4 ? "2 values {scale, deg_free}" : "1 value {binsize}");
  const double p0 = params_host[0], p1 = kind == 4 ? params_host[1] : 0.0;
  if (kind == 4 && (!(p0 > 1e-6) || !std::isfinite(p0) || !(p1 > 2.0) || !std::isfinite(p1)))
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood_params: StudentT needs scale > 1e-6 (softplus + 1e-6) and deg_free > 2, got %g, %g", p0, p1);
  if (kind == 5 && (!(p0 > 0) || !std::isfinite(p0))) return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood_params: Poisson needs binsize > 0, got %g", p0);
  if (!model->has_head) return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood_params: set the head first");
  LayerState& H = *model->layers.back();
  if (H.gZ && model->lik_kind != kind) return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood_params: the likelihood is fixed once a gradient was taken");
  if (model->enq_seq != model->col_seq) return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood_params: enqueued steps are still to be collected");
  // a model that has taken steps with int32 labels keeps them (as Softmax is refused on a float64-target model)
  if (!model->lik().float_targets() && model->enq_seq > 0)
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_likelihood_params: kind %d takes float64 targets, this model has taken steps with int32 labels (kind %d)", kind, model->lik_kind);
  const bool fresh = model->lik_kind != kind;
  ++model->param_version;
  model->lik_Q = 0;   // (a node table belongs to the Softmax likelihood it was set on)
  model->lik_kind = kind;
  H.lik_slots = kind == 4 ? 1 : 0;   // (the StudentT scale takes the Gaussian variance's slot: a Poisson block is a RobustMax one)
  if (kind == 5) { model->lik_binsize = p0; return DCGP_OK; }
  model->lik_nu = p1; model->lik_cnu = student_t_const(p1);
  if (!model->d_lik && dev_alloc(ctx, (void**)&model->d_lik, 3 * sizeof(double), "d_lik") != hipSuccess)   // {scale, Adam m, Adam v}
    return ctx_fail(ctx, DCGP_ERR_ALLOC, "set_likelihood_params: device allocation failed");
  const double init[3] = {p0, 0.0, 0.0};
  HIP_TRY(ctx, hipMemcpyAsync(model->d_lik, init, fresh ? sizeof init : sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

}  // extern "C"

// the status words of the factorisations the model's current bank holds (with factor reuse: the chain of an earlier call)
int fill_status(dcgp_model* model, FactorStatus* st) {
  auto& groups = model->groups[model->bank];
  if (groups.size() > 16) return ctx_fail(model->ctx, DCGP_ERR_ARG, "model: too many factor groups");
  st->ngroups = (int)groups.size();
  for (int q = 0; q < st->ngroups; ++q) { st->info[q] = groups[q].d_info; st->ninfo[q] = (int)groups[q].K.size(); }
  return DCGP_OK;
}

int forward_data_impl(dcgp_model* model, const double* X, int N, int S, const double* const* z_per_layer_host, uint64_t seed,
                      int dedup_layer0, int* rows_last) {
  StreamGuard guard(model->ctx);
  DCGP_TRY(forward_all(model, X, N, S, z_per_layer_host, seed, dedup_layer0, false, false, rows_last));
  return forward_done(model, nullptr);   // the caller synchronises the stream before it returns
}

int elbo_forward_enqueue_impl(dcgp_model* model, const double* X, const int32_t* y, int N, double scale,
                              const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0, uint64_t* ticket,
                              bool pipelined, const double* yf) {
  if (!model || !X || !(y || yf) || N <= 0 || !ticket) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "elbo_forward: bad args") : DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (!model->has_head) return ctx_fail(ctx, DCGP_ERR_ARG, "model has no head layer");
  const Likelihood lik = model->lik();
  const Targets targets = Targets::of(y, yf, model->layers.back()->R);
  DCGP_TRY(lik_check_targets(ctx, lik, targets, "elbo_forward"));
  if (model->enq_seq - model->col_seq >= (uint64_t)dcgp_model::RING)
    return ctx_fail(ctx, DCGP_ERR_ARG, "elbo_forward_enqueue: %d steps in flight, collect the oldest first", dcgp_model::RING);
  if (!model->h_ring) {
    if (hipHostMalloc((void**)&model->h_ring, dcgp_model::RING * 8 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void**)&model->h_ring_dev, model->h_ring, 0) != hipSuccess)
      return ctx_fail(ctx, DCGP_ERR_ALLOC, "elbo_forward: pinned result slots");
    memset(model->h_ring, 0, dcgp_model::RING * 8 * sizeof(double));
    for (auto& e : model->ring_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  int rows = 0;
  const int S = model->S;
  const auto host_t0 = std::chrono::steady_clock::now();
  StreamGuard guard(ctx);   // forward_all leaves ctx->stream on the step's main stream
  const int nl = (int)model->layers.size();
  LayerState& H = *model->layers[nl - 1];
  const int slot = (int)(model->enq_seq % dcgp_model::RING);
  DCGP_TRY(forward_all(model, X, N, S, z_per_layer_host, seed, dedup_layer0, true, pipelined, &rows));
  auto& o = model->outs[nl - 1];
  double* scal = model->d_scal + 64 * model->bank;
  DCGP_TRY(ensure(ctx, &model->d_ve, &model->ve_cap, (size_t)rows));
  // rows == S*N normally; a head-only model under dedup has rows == N with S identical copies
  const double inv_s = (rows == S * N) ? 1.0 / S : 1.0;
  ElboFinish fin;
  DCGP_TRY(fill_finish(model, scale, slot, &fin));
  const KlTail* klt = (model->kl_in_tail[model->bank] && !model->kl_rode[model->bank]) ? &model->kl_tail[model->bank] : nullptr;
  // From here on a kernel that writes this slot's completion word (ticket + 1) may be in flight.  If anything below fails the ticket is
  // NOT handed out and the next enqueue reuses slot and ticket: the word is cleared, behind a device sync, so that the stale kernel's
  // write cannot satisfy the retried step's wait early.
  struct SlotGuard {
    dcgp_model* m; int slot; bool armed = true;
    ~SlotGuard() {
      if (!armed) return;
      hipDeviceSynchronize();
      m->h_ring[8 * slot + 4] = 0.0;
    }
  } slot_guard{model, slot};
  if (!ctx->comm) {
    // (Measured and dropped, round 6: this launch's work at the end of the head's one-launch conditional -- the last of the R workgroups of a 16-row
    // strip to arrive runs the rows' expectations, the last workgroup of the launch the sum and the assembly.  cfg2 head-only 0.2210 -> 0.2234 ms, cfg1
    // 0.1416 -> 0.1462, conv + head +2 us (profiles/r06_tail_ride_and_prep_ab.txt): two levels of agent-scope release/acquire at the end of 200
    // workgroups cost more than the 13 us launch they replace.)
    // expectations, their sum, the KL pieces where the chain left their ingredients, and the ELBO assembly in one launch
    DCGP_TRY(lik_elbo_tail(ctx, lik, o.mean, o.var, targets, rows, N, H.R, model->d_ve, inv_s, scal, fin, klt));
  } else {
    // multi-GPU: the data term is summed over the ranks between the reduction and the assembly
    DCGP_TRY(lik_elbo_tail(ctx, lik, o.mean, o.var, targets, rows, N, H.R, model->d_ve, inv_s, scal, ElboFinish(), klt));
    // A step kept in flight: collective and assembly go to the comm stream behind one event, and the main stream is free for the next step's
    // data path at once -- in stream, a 1-double ncclAllReduce (~20 us of latency over xGMI, more when a rank is late) sat in front of the next
    // step's layer kernel.  What it reads (scal of this bank, the chain's status words) stays untouched until the bank's next writer, which
    // waits for this step's ring event (forward_all: done_ev).  (Not for a training step: its gradient collectives follow on the main stream,
    // and one communicator's collectives stay on one stream.)
    const bool side_comm = pipelined && !model->grad_follows && !ctx->no_side && !ctx->opt.comm_inline;
    if (side_comm) {
      if (!ctx->stream_comm) {
        if (hipStreamCreateWithFlags(&ctx->stream_comm, hipStreamNonBlocking) != hipSuccess) return ctx_fail(ctx, DCGP_ERR_HIP, "comm stream");
        for (auto& e : ctx->ev_comm) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
      }
      HIP_TRY(ctx, hipEventRecord(ctx->ev_comm[slot], ctx->stream));
      HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream_comm, ctx->ev_comm[slot], 0));
      ctx->stream = ctx->stream_comm;   // (the StreamGuard above restores the caller's stream)
      if (ctx->comm_gate) DCGP_TRY(comm_gate_wait(ctx));
    }
    DCGP_TRY(allreduce_sum_f64_async(ctx, scal, 1));
    hipLaunchKernelGGL(combine_kernel, dim3(1), dim3(64), 0, ctx->stream, scal, fin);
    LAUNCH_CHECK(ctx);
  }
  HIP_TRY(ctx, hipEventRecord(model->ring_ev[slot], ctx->stream));
  DCGP_TRY(forward_done(model, model->ring_ev[slot]));
  if (ctx->timing) {   // host time to enqueue one step (everything before the wait), reported beside the kernel timers
    auto& acc = ctx->tim["host_enqueue"];
    acc.launches += 1;
    acc.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count();
  }
  slot_guard.armed = false;
  *ticket = model->enq_seq++;
  return DCGP_OK;
}

int elbo_forward_collect_impl(dcgp_model* model, uint64_t ticket, double* out_host, int* info_host) {
  if (!model || !out_host) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "elbo_forward_collect: bad args") : DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (info_host) *info_host = 0;
  if (ticket != model->col_seq || ticket >= model->enq_seq)
    return ctx_fail(ctx, DCGP_ERR_ARG, "elbo_forward_collect: tickets are collected in the order they were handed out");
  const int slot = (int)(ticket % dcgp_model::RING);
  // The step's last kernel writes its four result words and then (system-scope release) ticket + 1 into the pinned slot: the host polls
  // that word instead of waiting for the event behind the kernel -- the event's signal is another packet for the command processor and a
  // wake-up through the runtime, several microseconds on a step of 150-800.  The event is still consulted now and then: a failed launch
  // or a lost device must end the wait.
  const volatile double* hv = model->h_ring + 8 * slot;
  const double want = (double)(ticket + 1);
  // bounded spin: a step of this path is 0.15-0.8 ms; one that has not answered after ~65 000 polls (a millisecond or two: the
  // large configurations, a rank waiting for a slower peer's all-reduce) hands the core back and blocks on the event instead --
  // eight ranks of a node must not hold eight cores against RCCL's proxy threads
  for (unsigned spins = 1; hv[4] != want; ++spins) {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield");
#endif
    if ((spins & 0xfff) == 0) {
      const hipError_t q = hipEventQuery(model->ring_ev[slot]);
      if (q == hipSuccess) break;                       // complete: coherent host memory already holds the words
      if (q != hipErrorNotReady) { HIP_TRY(ctx, q); }
      if (spins >= (1u << 16)) {
        HIP_TRY(ctx, hipEventSynchronize(model->ring_ev[slot]));
        break;
      }
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  ++model->col_seq;
  const double* h = model->h_ring + 8 * slot;
  out_host[0] = h[0]; out_host[1] = h[1]; out_host[2] = h[2];
  // the timers resolve their events lazily, once nothing is in flight any more
  if (ctx->timing && ctx->pending.size() > 512 && model->col_seq == model->enq_seq) timing_flush(ctx);   // synchronises every stream of the ctx
  const int bad = (int)h[3];
  if (info_host) *info_host = bad;
  if (bad) return ctx_fail(ctx, DCGP_ERR_NOT_PD, "Cholesky: matrix not positive definite at column %d", bad);
  return DCGP_OK;
}

int elbo_forward_impl(dcgp_model* model, const double* X, const int32_t* y, int N, double scale,
                      const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0, double* out_host,
                      int* info_host, const double* yf) {
  if (!model || !out_host) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "elbo_forward: bad args") : DCGP_ERR_ARG;
  if (model->enq_seq != model->col_seq) return ctx_fail(model->ctx, DCGP_ERR_ARG, "elbo_forward: enqueued steps are still to be collected");
  if (info_host) *info_host = 0;
  uint64_t ticket = 0;
  DCGP_TRY(elbo_forward_enqueue_impl(model, X, y, N, scale, z_per_layer_host, seed, dedup_layer0, &ticket, false, yf));
  return elbo_forward_collect_impl(model, ticket, out_host, info_host);
}

extern "C" {

int dcgp_model_propagate(dcgp_model* model, const double* X, int N, int S, const double* const* z_per_layer_host,
                         uint64_t seed, double* out_fmean, double* out_fvar, int* info_host) {
  if (!model || !X || N <= 0 || S <= 0) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "propagate: bad args") : DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (info_host) *info_host = 0;
  int rows = 0;
  DCGP_TRY(forward_data_impl(model, X, N, S, z_per_layer_host, seed, 0, &rows));
  const int nl = (int)model->layers.size();
  auto& o = model->outs[nl - 1];
  size_t n = (size_t)rows * o.width;
  if (out_fmean) HIP_TRY(ctx, hipMemcpyAsync(out_fmean, o.mean, n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  if (out_fvar) HIP_TRY(ctx, hipMemcpyAsync(out_fvar, o.var, n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  return finish_inference(model, info_host);
}

namespace {
// mean over the S samples of the class probabilities: p_bar[n][k] = 1/S sum_s p[s*N + n][k]
__global__ void sample_mean_kernel(const double* __restrict__ p, int S, long NK, double* __restrict__ out) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= NK) return;
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc += p[(long)s * NK + i];
  out[i] = acc / (double)S;
}
}  // namespace

int dcgp_model_predict_y(dcgp_model* model, const double* X, int N, int S, const double* const* z_per_layer_host,
                         uint64_t seed, double* out_p, double* out_p_mean, int* info_host) {
  if (!model || !X || N <= 0 || S <= 0 || (!out_p && !out_p_mean))
    return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "predict_y: bad args") : DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  const Likelihood lik = model->lik();
  if (lik.float_targets()) return ctx_fail(ctx, DCGP_ERR_ARG, "predict_y: a Gaussian- or Bernoulli-likelihood model predicts with dcgp_model_predict_mean_var");
  if (model->has_head) DCGP_TRY(lik_check_targets(ctx, lik, Targets{nullptr, nullptr, model->layers.back()->R, false}, "predict_y"));
  if (info_host) *info_host = 0;
  int rows = 0;
  DCGP_TRY(forward_data_impl(model, X, N, S, z_per_layer_host, seed, 0, &rows));
  const int nl = (int)model->layers.size();
  auto& o = model->outs[nl - 1];
  const int K = o.width;
  double* p = out_p;
  if (!p) {
    p = (double*)ws_get(ctx, "predict_p", (size_t)rows * K * sizeof(double));
    if (!p) return DCGP_ERR_ALLOC;
  }
  DCGP_TRY(lik_class_probs(ctx, lik, o.mean, o.var, rows, K, p));
  if (out_p_mean) {
    long NK = (long)N * K;
    hipLaunchKernelGGL(sample_mean_kernel, dim3((unsigned)((NK + 255) / 256)), dim3(256), 0, ctx->stream, p, S, NK, out_p_mean);
    LAUNCH_CHECK(ctx);
  }
  return finish_inference(model, info_host);
}

int dcgp_model_predict_mean_var(dcgp_model* model, const double* X, int N, int S, const double* const* z_per_layer_host,
                                uint64_t seed, double* out_mean, double* out_var, int* info_host) {
  if (!model || !X || N <= 0 || S <= 0 || (!out_mean && !out_var))
    return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "predict_mean_var: bad args") : DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (!model->lik().float_targets()) return ctx_fail(ctx, DCGP_ERR_ARG, "predict_mean_var: not a Gaussian- or Bernoulli-likelihood model (dcgp_model_predict_y)");
  if (info_host) *info_host = 0;
  int rows = 0;
  DCGP_TRY(forward_data_impl(model, X, N, S, z_per_layer_host, seed, 0, &rows));
  auto& o = model->outs.back();
  DCGP_TRY(lik_predict(ctx, model->lik(), o.mean, o.var, (long)rows * o.width, out_mean, out_var));
  return finish_inference(model, info_host);
}

int dcgp_model_patch_evidence(dcgp_model* model, const double* X, int N, int S, const double* const* z_per_layer_host, uint64_t seed,
                              double* out_c, double* out_fmean, int* info_host) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (info_host) *info_host = 0;
  if (N < 0 || S <= 0) return ctx_fail(ctx, DCGP_ERR_ARG, "patch_evidence: bad args (N %d, S %d)", N, S);
  if (!model->has_head) return ctx_fail(ctx, DCGP_ERR_ARG, "model has no head layer");
  const int nl = (int)model->layers.size();
  LayerState& H = *model->layers[nl - 1];
  if (H.in_scale || (H.v.H == 1 && H.v.W == 1))
    return ctx_fail(ctx, DCGP_ERR_ARG, "patch_evidence: a dense RBF head has no patches to split its mean over");
  if (H.base_type != 0) return ctx_fail(ctx, DCGP_ERR_ARG, "patch_evidence: the head's base kernel must be RBF");
  if (N == 0) return DCGP_OK;
  if (!X || !out_c) return ctx_fail(ctx, DCGP_ERR_ARG, "patch_evidence: NULL pointer");
  int rows = 0;
  DCGP_TRY(forward_data_impl(model, X, N, S, z_per_layer_host, seed, 0, &rows));
  // the head's input: the last hidden layer's sample, or the S copies of X (row n shows image n % N) -- what head_forward swept
  const double* F = model->pad[nl - 1] > 0 ? model->pad_in[nl - 1] : (nl > 1 ? model->outs[nl - 2].sample : X);
  const int n_mod = nl > 1 ? rows : N;
  // beta = inv(L)^T alpha from the chain's own factors: L^-T q_mu when whitened (alpha is q_mu), Kuu^-1 q_mu otherwise
  DCGP_TRY(patch_map(ctx, F, rows, n_mod, H.v, H.Z, H.ZS, H.M, H.variance, H.ls, H.w, nullptr, H.g.LinvT, H.g.alpha, H.g.Rp, H.R, out_c,
                     "m" + std::to_string(model->id) + "_"));
  if (out_fmean)
    HIP_TRY(ctx, hipMemcpyAsync(out_fmean, model->outs[nl - 1].mean, (size_t)rows * H.R * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  return finish_inference(model, info_host);
}

}  // extern "C"

namespace {
// A test set in batches of `batch` images, enqueued back to back on the main stream: per batch forward_all (the parameter-only chain
// only where factor_reuse does not let it stand) and ONE tail launch; behind the last batch one sum launch and one
// read-back -- the call's only stream synchronisation.
//   Buffer reuse between batches: the head's mean / var (model->outs), the sweeps' scratch and d_kd are written by batch b + 1 on the
//   main stream, behind batch b's tail; the Kdiag excursion to the auxiliary stream forks from the main stream at that point
//   (layer_impl.h: ev_aux).  The chain of a batch (factor_reuse 0, or the first batch) writes the parameter-only state of its bank
//   on its own stream: done_ev[bank] -- recorded on the main stream behind the tail of the last batch on that bank -- orders it.
//   Workspaces: batch 0 is the largest, every later request is served by what it grew.
// With views set (dcgp_model_set_eval_views; not the single identity view) a batch of n images becomes its V n view images, view-major in a per-model
// workspace (augment.hip: view v of image i at row v n + i), forward_all runs on those, and its head rows [S][V n][K] -- row s V n + v n + i =
// (s V + v) n + i -- are S V samples of n images to the tail: the predictive distribution of an image is the mixture over samples and views.
// tail(lo, n, SV, o): the tail launch of the batch of n images from image lo on, on the head's rows o = SV samples of them; sum(st): the launch behind the last batch, which
// leaves `nres` words in res -- [2] the first non-positive pivot of st, [3] the labels outside [0, K) -- read back into h.
template <class Tail, class Sum>
int eval_batches(dcgp_model* model, const double* X, int N_total, int batch, int S, const double* const* zs, uint64_t seed, const char* who,
                 Tail tail, Sum sum, const double* res, double* h, int nres, int* info_host) {
  dcgp_ctx* ctx = model->ctx;
  const int nl = (int)model->layers.size();
  const int K = model->layers[nl - 1]->R;
  const long in_len = model->image_len();   // one image of X (unpadded: a padded first layer pads its batch on the device)
  const bool views = model->eval_views_active();
  const int V = views ? model->eval_V : 1;
  double* vw = nullptr;
  if (views) {
    if ((long)model->ev_H * model->ev_W * model->ev_C != in_len)
      return ctx_fail(ctx, DCGP_ERR_ARG, "%s: the views' %d x %d x %d images are not the model's of %ld values", who, model->ev_H, model->ev_W, model->ev_C, in_len);
    const long nmax = N_total < batch ? N_total : batch;
    if ((long)S * V * nmax > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: S * V * batch = %d * %d * %ld head rows exceed 2^31 - 1", who, S, V, nmax);
    vw = (double*)ws_get(ctx, "m" + std::to_string(model->id) + "_eval_views", (size_t)V * nmax * in_len * sizeof(double));
    if (!vw) return DCGP_ERR_ALLOC;
  }
  DCGP_TRY(ensure_events(model));
  StreamGuard guard(ctx);
  std::vector<const double*> zb(nl, nullptr);
  const int nb = (N_total + batch - 1) / batch;
  for (int b = 0; b < nb; ++b) {
    const long lo = (long)b * batch;
    const int n = (int)(N_total - lo < batch ? N_total - lo : batch);
    // noise: per layer the batches' [S][V n_b][D_l] tables back to back, batch b's from S * V * lo * D_l on (V = 1 without views)
    for (int l = 0; l < nl && zs; ++l) {
      const LayerState& L = *model->layers[l];
      const long D = L.is_head ? L.R : model->geom(l).P() * L.R;   // (image layout: a dilated layer's true patch count)
      zb[l] = zs[l] ? zs[l] + (long)S * V * lo * D : nullptr;
    }
    // the batch forward_all sees: the caller's images, or their views (the workspace is rewritten behind the previous batch's tail, on its stream)
    const double* Xb = X + lo * in_len;
    if (views) {
      DCGP_TRY(gather_eval_views(model, Xb, n, vw));
      Xb = vw;
    }
    int rows = 0;
    DCGP_TRY(forward_all(model, Xb, V * n, S, zs ? zb.data() : nullptr, seed + (uint64_t)b, 0, false, false, &rows));
    const auto& o = model->outs[nl - 1];
    if (rows != S * V * n || o.width != K)
      return ctx_fail(ctx, DCGP_ERR_ARG, "%s: head rows %d x %d, expected %d x %d", who, rows, o.width, S * V * n, K);
    DCGP_TRY(tail(lo, n, S * V, o));
    HIP_TRY(ctx, hipEventRecord(model->ev_eval[model->bank], ctx->stream));
    DCGP_TRY(forward_done(model, model->ev_eval[model->bank]));
  }
  FactorStatus st;   // the status words of the factorisations the batches used
  DCGP_TRY(fill_status(model, &st));
  DCGP_TRY(sum(st));
  HIP_TRY(ctx, hipMemcpyAsync(h, res, nres * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (h[3] > 0) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: %d labels outside [0, %d)", who, (int)h[3], K);
  const int bad = (int)h[2];
  if (info_host) *info_host = bad;
  if (bad) return ctx_fail(ctx, DCGP_ERR_NOT_PD, "Cholesky: matrix not positive definite at column %d", bad);
  return DCGP_OK;
}

// The evaluation tails (lik_eval_tail) and sum over eval_batches.
// yf (Gaussian or Bernoulli model, y == nullptr): targets [N_total][K]; out_p_mean is then the sample-mean prediction (Bernoulli: the
// sample-mean p) [N_total][K], out_ld_nd (may be nullptr) the log density per (image, output), and out_host[0] the sum of the squared
// errors of the sample-mean prediction (Bernoulli: the number of correct (image, output) entries; per image in sqerr, summed alike).
int evaluate_impl(dcgp_model* model, const double* X, const int32_t* y, int N_total, int batch, int S, const double* const* zs,
                  uint64_t seed, double* out_logdens, double* out_p_mean, double* out_host, int* info_host, const char* who,
                  const double* yf = nullptr, double* out_ld_nd = nullptr) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (info_host) *info_host = 0;
  if (!X || !(y || yf) || N_total <= 0 || batch <= 0 || S <= 0 || !out_host)
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: bad args (N %d, batch %d, S %d)", who, N_total, batch, S);
  if (!model->has_head) return ctx_fail(ctx, DCGP_ERR_ARG, "model has no head layer");
  const int K = model->layers.back()->R;
  const Likelihood lik = model->lik();
  const Targets targets = Targets::of(y, yf, K);
  DCGP_TRY(lik_check_targets(ctx, lik, targets, who));
  if (!yf && K < 2) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: the last layer has %d outputs, a multi-class likelihood needs >= 2", who, K);
  const int V = model->eval_views_active() ? model->eval_V : 1;   // (eval_batches: S * V samples per image)
  if (!yf && (long)S * V * K + K > kEvalMaxSlots)
    return V > 1 ? ctx_fail(ctx, DCGP_ERR_ARG, "%s: S = %d samples of V = %d views of %d classes exceed the tail's LDS (S * V * K + K <= %d)", who, S, V, K, kEvalMaxSlots)
                 : ctx_fail(ctx, DCGP_ERR_ARG, "%s: S = %d samples of %d classes exceed the tail's LDS", who, S, K);
  // the per-image results of the whole set: requested once, before batch 0
  const std::string mp = "m" + std::to_string(model->id) + "_";
  EvalOut eo;
  eo.logdens = out_logdens ? out_logdens : (double*)ws_get(ctx, mp + "eval_logdens", (size_t)N_total * sizeof(double));
  eo.ld_nd = out_ld_nd; eo.p_mean = out_p_mean;
  eo.ok = yf ? nullptr : (int*)ws_get(ctx, mp + "eval_ok", (size_t)N_total * sizeof(int));
  eo.score = yf ? (double*)ws_get(ctx, mp + "eval_sqerr", (size_t)N_total * sizeof(double)) : nullptr;
  double* res = (double*)ws_get(ctx, mp + "eval_res", 4 * sizeof(double));
  if (!eo.logdens || !(eo.ok || eo.score) || !res) return DCGP_ERR_ALLOC;
  double h[4];
  DCGP_TRY(eval_batches(
      model, X, N_total, batch, S, zs, seed, who,
      [&](long lo, int n, int SV, const dcgp_model::Out& o) { return lik_eval_tail(ctx, lik, o.mean, o.var, targets, n, SV, K, lo, eo); },
      [&](const FactorStatus& st) { return lik_eval_sum(ctx, lik, eo, N_total, st, res); }, res, h, 4, info_host));
  out_host[0] = h[0];
  out_host[1] = h[1];
  return DCGP_OK;
}

// eval_batches with the uncertainty tails (uncertainty.hip) in place of the evaluation tails and unc_sum in place of the sum kernel.  f64y: the
// Bernoulli entry (targets yf [N_total][K], entries = (image, output) pairs); otherwise RobustMax (labels y [N_total], entries = images).  Labels may
// be nullptr.  u holds the caller's outputs (any may be nullptr: the per-entry values the dataset kernel reads then live in workspaces).
int uncertainty_impl(dcgp_model* model, const double* X, const int32_t* y, const double* yf, bool f64y, int N_total, int batch, int S,
                     const double* const* zs, uint64_t seed, int bins, UncOut u, double* out_table, double* out_host, int* info_host,
                     const char* who) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (info_host) *info_host = 0;
  if (!X || N_total <= 0 || batch <= 0 || S <= 0 || bins < 1 || !out_host)
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: bad args (N %d, batch %d, S %d, bins %d)", who, N_total, batch, S, bins);
  if (model->lik_kind == 1) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: class probabilities need a classification likelihood, this model is Gaussian", who);
  if (model->lik_kind == 4 || model->lik_kind == 5)
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: class probabilities need a classification likelihood, this model is %s", who, model->lik_kind == 4 ? "StudentT" : "Poisson");
  if (!model->has_head) return ctx_fail(ctx, DCGP_ERR_ARG, "model has no head layer");
  const int K = model->layers.back()->R;
  const Likelihood lik = model->lik();
  const Targets targets{y, yf, K, f64y};
  DCGP_TRY(lik_check_targets(ctx, lik, targets, who));
  if (!f64y && K < 2) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: the last layer has %d outputs, a multi-class likelihood needs >= 2", who, K);
  const int V = model->eval_views_active() ? model->eval_V : 1;   // (eval_batches: S * V samples per image)
  if (!f64y && V > 1 && (long)S * V * K + K + kUncExtraSlots > kEvalMaxSlots)
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: S = %d samples of V = %d views of %d classes exceed the tail's LDS (S * V * K + K + %d <= %d)", who, S, V, K, kUncExtraSlots, kEvalMaxSlots);
  if (!f64y && (long)S * K + K + kUncExtraSlots > kEvalMaxSlots)
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: S = %d samples of %d classes exceed the tail's LDS (S * K + K + %d <= %d)", who, S, K, kUncExtraSlots, kEvalMaxSlots);
  const bool labels = f64y ? yf != nullptr : y != nullptr;
  const long n_ent = f64y ? (long)N_total * K : N_total;
  const std::string mp = "m" + std::to_string(model->id) + "_";
  auto dbl = [&](double* given, const char* name, long n) { return given ? given : (double*)ws_get(ctx, mp + name, (size_t)n * sizeof(double)); };
  if (labels) {
    u.logdens = dbl(u.logdens, "unc_logdens", N_total);
    u.ok = (int*)ws_get(ctx, mp + "unc_ok", (size_t)n_ent * sizeof(int));
    u.brier = dbl(nullptr, "unc_brier", n_ent);
    if (!u.logdens || !u.ok || !u.brier) return DCGP_ERR_ALLOC;
  } else {
    u.logdens = nullptr;
  }
  u.pred_ent = dbl(u.pred_ent, "unc_pred_ent", n_ent);
  u.mi = dbl(u.mi, "unc_mi", n_ent);
  u.conf = dbl(u.conf, "unc_conf", n_ent);
  if (!u.pred) u.pred = (int*)ws_get(ctx, mp + "unc_pred", (size_t)n_ent * sizeof(int));
  double* table = dbl(out_table, "unc_table", 3L * bins);
  double* res = (double*)ws_get(ctx, mp + "unc_res", 9 * sizeof(double));
  if (!u.pred_ent || !u.mi || !u.conf || !u.pred || !table || !res) return DCGP_ERR_ALLOC;
  UncSumArgs sa;
  sa.logdens = u.logdens; sa.n_img = N_total; sa.ok = labels ? u.ok : nullptr; sa.brier = u.brier; sa.pred_ent = u.pred_ent; sa.mi = u.mi;
  sa.conf = u.conf; sa.n_ent = n_ent; sa.bins = bins; sa.table = table;
  double h[9];
  DCGP_TRY(eval_batches(
      model, X, N_total, batch, S, zs, seed, who,
      [&](long lo, int n, int SV, const dcgp_model::Out& o) { return lik_unc_tail(ctx, lik, o.mean, o.var, targets, n, SV, K, lo, u); },
      [&](const FactorStatus& st) { return unc_sum(ctx, sa, st, res); }, res, h, 9, info_host));
  out_host[0] = h[0];
  out_host[1] = h[1];
  for (int q = 2; q < 7; ++q) out_host[q] = h[q + 2];
  return DCGP_OK;
}
}  // namespace

extern "C" {

int dcgp_model_predict_density_f64y(dcgp_model* model, const double* X, const double* y, int N, int S,
                                    const double* const* z_per_layer, uint64_t seed, double* out_logdens, int* info_host) {
  if (model && (!out_logdens || !y)) return ctx_fail(model->ctx, DCGP_ERR_ARG, "predict_density_f64y: out_logdens or y is NULL");
  double sums[2];
  return evaluate_impl(model, X, nullptr, N, N, S, z_per_layer, seed, nullptr, nullptr, sums, info_host, "predict_density", y, out_logdens);
}

int dcgp_model_evaluate_f64y(dcgp_model* model, const double* X, const double* y, int N_total, int batch, int S,
                             const double* const* z_per_layer, uint64_t seed, double* out_logdens, double* out_y_mean,
                             double* out_host, int* info_host) {
  if (model && !y) return ctx_fail(model->ctx, DCGP_ERR_ARG, "evaluate_f64y: y is NULL");
  return evaluate_impl(model, X, nullptr, N_total, batch, S, z_per_layer, seed, out_logdens, out_y_mean, out_host, info_host, "evaluate", y);
}

int dcgp_model_predict_density(dcgp_model* model, const double* X, const int32_t* y, int N, int S,
                               const double* const* z_per_layer, uint64_t seed, double* out_logdens, int* info_host) {
  if (model && !out_logdens) return ctx_fail(model->ctx, DCGP_ERR_ARG, "predict_density: out_logdens is NULL");
  double sums[2];
  return evaluate_impl(model, X, y, N, N, S, z_per_layer, seed, out_logdens, nullptr, sums, info_host, "predict_density");
}

int dcgp_model_evaluate(dcgp_model* model, const double* X, const int32_t* y, int N_total, int batch, int S,
                        const double* const* z_per_layer, uint64_t seed, double* out_logdens, double* out_p_mean,
                        double* out_host, int* info_host) {
  return evaluate_impl(model, X, y, N_total, batch, S, z_per_layer, seed, out_logdens, out_p_mean, out_host, info_host, "evaluate");
}

int dcgp_model_evaluate_uncertainty(dcgp_model* model, const double* X, const int32_t* y, int N_total, int batch, int S,
                                    const double* const* z_per_layer, uint64_t seed, int bins, double* out_logdens, double* out_p_mean,
                                    double* out_pred_entropy, double* out_exp_entropy, double* out_mutual_info, double* out_confidence,
                                    int32_t* out_prediction, double* out_table, double* out_host, int* info_host) {
  UncOut u;
  u.logdens = out_logdens; u.p_mean = out_p_mean; u.pred_ent = out_pred_entropy; u.exp_ent = out_exp_entropy; u.mi = out_mutual_info;
  u.conf = out_confidence; u.pred = out_prediction;
  return uncertainty_impl(model, X, y, nullptr, false, N_total, batch, S, z_per_layer, seed, bins, u, out_table, out_host, info_host,
                          "evaluate_uncertainty");
}

int dcgp_model_evaluate_uncertainty_f64y(dcgp_model* model, const double* X, const double* y, int N_total, int batch, int S,
                                         const double* const* z_per_layer, uint64_t seed, int bins, double* out_logdens, double* out_p_mean,
                                         double* out_pred_entropy, double* out_exp_entropy, double* out_mutual_info,
                                         double* out_confidence, int32_t* out_prediction, double* out_table, double* out_host,
                                         int* info_host) {
  UncOut u;
  u.logdens = out_logdens; u.p_mean = out_p_mean; u.pred_ent = out_pred_entropy; u.exp_ent = out_exp_entropy; u.mi = out_mutual_info;
  u.conf = out_confidence; u.pred = out_prediction;
  return uncertainty_impl(model, X, nullptr, y, true, N_total, batch, S, z_per_layer, seed, bins, u, out_table, out_host, info_host,
                          "evaluate_uncertainty");
}

int dcgp_model_layer_output(dcgp_model* model, int layer, double* out_sample, double* out_mean, double* out_var,
                            int* rows, int* width) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (layer < 0 || layer >= (int)model->outs.size()) return ctx_fail(ctx, DCGP_ERR_ARG, "layer_output: no output for layer %d", layer);
  auto& o = model->outs[layer];
  if (rows) *rows = o.rows;
  if (width) *width = o.width;
  size_t n = (size_t)o.rows * o.width * sizeof(double);
  if ((out_mean || out_var || (out_sample && model->layers[layer]->is_head)) && !model->keep_outputs)
    return ctx_fail(ctx, DCGP_ERR_ARG, "layer_output: enable dcgp_model_set_keep_outputs before the forward pass");
  if (out_sample) HIP_TRY(ctx, hipMemcpyAsync(out_sample, o.sample, n, hipMemcpyDeviceToDevice, ctx->stream));
  if (out_mean) HIP_TRY(ctx, hipMemcpyAsync(out_mean, o.mean, n, hipMemcpyDeviceToDevice, ctx->stream));
  if (out_var) HIP_TRY(ctx, hipMemcpyAsync(out_var, o.var, n, hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

}  // extern "C"

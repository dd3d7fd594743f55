// optim.hip -- the optimiser steps on the gradients the reverse pass (grad.hip) leaves in every layer's gradient block, and the C API that reads
// parameters and gradients back or freezes them.  opt_enqueue / opt_readback are also what a training step (grad.hip: elbo_grad_run) ends on.
#include "model_state.h"

namespace {

inline unsigned blocks_for(long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

// tf.train.AdamOptimizer / GradientDescentOptimizer on gpflow's unconstrained variables, ascending the ELBO.  transform 0: identity;
// 1: gpflow transforms.positive (x = softplus(u) + 1e-6): the parameter is held constrained, moved through u.
// ONE launch for every parameter group of every layer (a launch per group: ten 5 us launches and 2 x layers small copies on a 1.5 ms
// step): block b works on group g with first_block[g] <= b < first_block[g + 1].  A layer's kernel hyper-parameters live on the host
// (they are launch arguments of the forward pass): their current values arrive as arguments, the updated ones go to the device copy
// and straight into a pinned host slot.
struct OptGroup {
  double* p; const double* g; double* m; double* v;   // parameter, gradient, Adam moments (unused by SGD)
  double* recip;                                      // != null: 1 / p is kept here as well (the dense head's staging scale)
  long n;
  int transform, hyp_layer;                           // hyp_layer >= 0: p is that layer's {variance, p1, p2} triple
  // sharded step (OptArgs::sharded): the group's offset in its layer's gradient block, the layer, and whether it only passes through
  long off; int layer, frozen;
  int hold;                                           // hyp_layer >= 0: bit i set = element i of the triple is held (set_trainable on one ArcCosine parameter)
};
constexpr int kNormSlot = 32;        // ctx->h_scratch[32]: a clipped step's norm (the hyper-parameter triples take [0, 24))
constexpr int OPT_GROUPS_MAX = 56;   // 7 conv layers of up to 6 groups (Z, q_mu, q_sqrt, hyper, mean filter, mixing) below a head of up to 7
struct OptArgs {
  OptGroup grp[OPT_GROUPS_MAX];
  int first_block[OPT_GROUPS_MAX + 1];
  int ng, sgd;
  double lr, b1, b2, eps;            // lr: Adam's bias-corrected step size, or the plain SGD rate
  double hyp_in[8][3];
  double* host_out;                  // [8][3] pinned
  const double* status;              // != null: a non-zero word there (the step's factorisation failed) leaves every parameter untouched
  // Sharded step (dcgp_model_set_grad_exchange 1): only the elements whose position in the layer's block lies in [sh_lo, sh_hi) are updated --
  // the gradient there is this rank's reduce-scattered sum -- and every value of the range, updated or frozen, also goes to stage[layer]
  // (the block's layout), which the all-gather then completes.  stage_only: the parameter arrays are left alone (the debug entry's other ranks).
  int sharded, stage_only;
  long sh_lo[8], sh_hi[8];
  double* stage[8];
  // Clipping by global norm (dcgp_model_set_grad_clip; the CLIP instance of the update and the two norm kernels only): clip[0] the step's scale c,
  // clip[1 + b] block b's partial sum of g_u^2; norm_out: the pinned slot the norm itself goes to
  double* clip;
  double max_norm;
  double* norm_out;
};
// The gradient the update moves element i of group G by, in the unconstrained space, as the two factors the update multiplies: g_u = g * f, g the
// gradient with respect to the constrained value x and f = dx/du (1, or sigmoid(u) = 1 - exp(-y) under transform 1).  false: the update leaves the
// element where it is (a frozen group, a held element of a hyper-parameter triple) -- it is no part of the norm either.  The clipped update and the
// norm both take g_u from here.
__device__ __forceinline__ bool opt_grad_u(const OptGroup& G, long i, double x, double* g, double* f) {
  if (G.frozen || (G.hyp_layer >= 0 && ((G.hold >> (int)i) & 1))) return false;
  *g = G.g[i];
  *f = G.transform == 1 ? -expm1(-(x - 1e-6)) : 1.0;
  return true;
}
// the sum of v over a block of 256 threads (four waves of 64), the same tree every time: lanes by halving within a wave, then the four waves' sums
// through LDS.  Every thread of the block calls it; every thread gets the sum.
__device__ __forceinline__ double block_sum_256(double v, double* red /* 4 doubles of LDS */) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
// Norm, first stage: the update's grid over the update's group table; block b leaves the sum of g_u^2 over its 256 elements in clip[1 + b].  (The
// parameter is read where the transform needs it only: the large groups are identity-transform.)
__global__ __launch_bounds__(256) void opt_norm_partial_kernel(OptArgs a) {
  if (a.status && *a.status != 0.0) return;
  __shared__ double red[4];
  int gi = 0;
  while (gi + 1 < a.ng && (int)blockIdx.x >= a.first_block[gi + 1]) ++gi;
  const OptGroup& G = a.grp[gi];
  const long i = (long)((int)blockIdx.x - a.first_block[gi]) * 256 + threadIdx.x;
  double sq = 0.0;
  if (i < G.n) {
    const double x = G.transform != 1 ? 0.0 : (G.hyp_layer >= 0 ? a.hyp_in[G.hyp_layer][i] : G.p[i]);
    double g, f;
    if (opt_grad_u(G, i, x, &g, &f)) { const double gu = g * f; sq = gu * gu; }
  }
  const double sum = block_sum_256(sq, red);
  if (threadIdx.x == 0) a.clip[1 + blockIdx.x] = sum;
}
// Norm, second stage (one block): thread t adds the partial sums t, t + 256, ... in index order, the 256 results go through the same tree -- the
// value depends on the partial sums alone, not on which block wrote when.  Leaves the scale in clip[0] and the norm in the pinned slot.
__global__ __launch_bounds__(256) void opt_norm_final_kernel(OptArgs a, int nb) {
  if (a.status && *a.status != 0.0) return;
  __shared__ double red[4];
  double s = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) s += a.clip[1 + b];
  const double sum = block_sum_256(s, red);
  if (threadIdx.x == 0) {
    const double norm = sqrt(sum);
    a.clip[0] = norm <= a.max_norm ? 1.0 : a.max_norm / norm;   // max_norm / max(norm, max_norm), and 1.0 for max_norm = +inf
    *a.norm_out = norm;
  }
}
// CLIP: the step on c * g_u, c from clip[0] (the norm kernels in front of it); the other instance is the step as it always was and reads nothing of it
template <bool CLIP>
__global__ __launch_bounds__(256) void opt_step_kernel(OptArgs a) {
  if (a.status && *a.status != 0.0) return;
  int gi = 0;
  while (gi + 1 < a.ng && (int)blockIdx.x >= a.first_block[gi + 1]) ++gi;
  const OptGroup& G = a.grp[gi];
  const long i = (long)((int)blockIdx.x - a.first_block[gi]) * 256 + threadIdx.x;
  if (i >= G.n) return;
  if (a.sharded && (G.off + i < a.sh_lo[G.layer] || G.off + i >= a.sh_hi[G.layer])) return;
  const double x = G.hyp_layer >= 0 ? a.hyp_in[G.hyp_layer][i] : G.p[i];
  double out;
  if constexpr (CLIP) {
    const double c = a.clip[0];
    double g, f;
    if (!opt_grad_u(G, i, x, &g, &f)) {
      out = x;
    } else if (a.sgd) {   // (the products in the unclipped step's order: c == 1.0 is that step to the bit)
      const double gr = c * g;
      if (G.transform == 1) {
        const double y = x - 1e-6;
        double u = y > 35.0 ? y : log(expm1(y));
        u += a.lr * gr * f;
        out = (u > 35.0 ? u : log1p(exp(u))) + 1e-6;
      } else {
        out = x + a.lr * gr;
      }
    } else {
      double gr = -g;
      double u = x;
      if (G.transform == 1) {
        const double y = x - 1e-6;
        u = y > 35.0 ? y : log(expm1(y));
        gr *= f;
      }
      gr *= c;
      const double mi = a.b1 * G.m[i] + (1.0 - a.b1) * gr;
      const double vi = a.b2 * G.v[i] + (1.0 - a.b2) * gr * gr;
      G.m[i] = mi;
      G.v[i] = vi;
      u -= a.lr * mi / (sqrt(vi) + a.eps);
      out = G.transform == 1 ? (u > 35.0 ? u : log1p(exp(u))) + 1e-6 : u;
    }
  } else if (G.frozen || (G.hyp_layer >= 0 && ((G.hold >> (int)i) & 1))) {
    out = x;
  } else if (a.sgd) {   // plain gradient ascent on the ELBO in the unconstrained space
    const double gr = G.g[i];
    if (G.transform == 1) {
      const double y = x - 1e-6;
      double u = y > 35.0 ? y : log(expm1(y));
      u += a.lr * gr * -expm1(-y);
      out = (u > 35.0 ? u : log1p(exp(u))) + 1e-6;
    } else {
      out = x + a.lr * gr;
    }
  } else {
    double gr = -G.g[i];                               // minimise -ELBO
    double u = x;
    if (G.transform == 1) {
      const double y = x - 1e-6;
      u = y > 35.0 ? y : log(expm1(y));               // softplus^-1
      gr *= -expm1(-y);                                // dx/du = sigmoid(u) = 1 - exp(-y)
    }
    const double mi = a.b1 * G.m[i] + (1.0 - a.b1) * gr;
    const double vi = a.b2 * G.v[i] + (1.0 - a.b2) * gr * gr;
    G.m[i] = mi;
    G.v[i] = vi;
    u -= a.lr * mi / (sqrt(vi) + a.eps);
    out = G.transform == 1 ? (u > 35.0 ? u : log1p(exp(u))) + 1e-6 : u;
  }
  if (a.sharded) a.stage[G.layer][G.off + i] = out;
  if (G.frozen || a.stage_only) return;
  G.p[i] = out;
  if (G.recip) G.recip[i] = 1.0 / out;
  if (G.hyp_layer >= 0) a.host_out[3 * G.hyp_layer + i] = out;
}
// behind the all-gather: the other ranks' shards of the staged block into this rank's parameter arrays
__global__ __launch_bounds__(256) void opt_unstage_kernel(OptArgs a) {
  if (a.status && *a.status != 0.0) return;
  int gi = 0;
  while (gi + 1 < a.ng && (int)blockIdx.x >= a.first_block[gi + 1]) ++gi;
  const OptGroup& G = a.grp[gi];
  const long i = (long)((int)blockIdx.x - a.first_block[gi]) * 256 + threadIdx.x;
  if (i >= G.n || G.frozen) return;
  if (G.off + i >= a.sh_lo[G.layer] && G.off + i < a.sh_hi[G.layer]) return;   // this rank's own shard: already in place
  const double out = a.stage[G.layer][G.off + i];
  G.p[i] = out;
  if (G.recip) G.recip[i] = 1.0 / out;
  if (G.hyp_layer >= 0) a.host_out[3 * G.hyp_layer + i] = out;
}

}  // namespace

// the launch alone, behind whatever the stream holds (status: see OptArgs).
// vranks > 0 (debugging aid, dcgp_model_debug_sharded_adam): the sharded step of `vranks` ranks played on this one GPU from rank 0's point of
// view -- its own shard for real, the others' into the staging block only, then the unstage pass.
int opt_enqueue(dcgp_model* model, const char* who, bool sgd, double lr, double beta1, double beta2, double eps, const double* status, int vranks) {
  dcgp_ctx* ctx = model->ctx;
  const int nl = (int)model->layers.size();
  if (nl > 8) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: at most 8 layers", who);
  const bool comm_sharded = ctx->comm && ctx->nranks > 1 && model->grad_exchange == 1 && model->grad_scattered;
  const bool sharded = comm_sharded || vranks > 0;
  const bool clip = model->grad_clip > 0.0;
  model->norm_pending = false;
  // a rank of a sharded update holds its shard of the gradient only: the norm would need an exchange of its own
  if (clip && sharded)
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: gradient clipping is on (dcgp_model_set_grad_clip) and the update is sharded (exchange mode 1): a rank sees "
                    "only its shard of the gradient, the global norm is not formed across ranks", who);
  ++model->param_version;   // the parameters change: parameter-only state of earlier steps is not reused (model_state.h)
  // Moments are rank-local in exchange mode 1: a rank holds m / v of its own shard only.  A full update on top of them (exchange mode 0, or an
  // optimiser step behind dcgp_elbo_grad) would move every element outside the shard with stale or zero moments -- differently on every rank.
  if (!sgd && !comm_sharded && vranks == 0 && model->sharded_steps > 0)
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: %llu sharded Adam steps were taken on this model (exchange mode 1): its moments cover this rank's shard only, "
                    "a full update would let the replicas diverge", who, (unsigned long long)model->sharded_steps);
  if (comm_sharded && !sgd) ++model->sharded_steps;
  const int nranks = vranks > 0 ? vranks : ctx->nranks, rank = vranks > 0 ? 0 : ctx->rank;
  OptArgs a{};
  a.sgd = sgd ? 1 : 0; a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.status = status;
  a.sharded = sharded ? 1 : 0;
  double* h = ctx->h_scratch;   // 64 pinned doubles: {variance, p1, p2} per layer
  if (hipHostGetDevicePointer((void**)&a.host_out, h, 0) != hipSuccess) return ctx_fail(ctx, DCGP_ERR_HIP, "%s: pinned slot not mapped", who);
  int nb = 0, cur_layer = 0;
  const double* blk0 = nullptr;
  auto add = [&](double* p, const double* g, double* const* mv, long n, int transform, int hyp_layer, double* recip, bool frozen) -> int {
    if (n <= 0 || (frozen && !sharded)) return DCGP_OK;
    if (a.ng >= OPT_GROUPS_MAX) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: too many parameter groups", who);
    OptGroup& G = a.grp[a.ng];
    G.p = p; G.g = g; G.m = mv[0]; G.v = mv[1]; G.recip = recip; G.n = n; G.transform = transform; G.hyp_layer = hyp_layer;
    G.off = (long)(g - blk0); G.layer = cur_layer; G.frozen = frozen ? 1 : 0;
    a.first_block[a.ng++] = nb;
    nb += (int)blocks_for(n);
    return DCGP_OK;
  };
  long shard[8] = {};
  for (int li = 0; li < nl; ++li) {
    LayerState& L = *model->layers[li];
    if (!L.gZ) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: call dcgp_elbo_grad first", who);
    DCGP_TRY(L.ensure_adam());   // (SGD: for the device copy of the hyper-parameters)
    cur_layer = li; blk0 = L.gZ;
    if (sharded) {
      DCGP_TRY(L.ensure_stage());
      if (nranks - 1 > (int)LayerState::kGradBlockPad) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: more ranks than the gradient block is padded for", who);
      DCGP_TRY(dcgp_shard_range((long)L.grad_block_count(), nranks, rank, &a.sh_lo[li], &a.sh_hi[li], &shard[li]));
      a.stage[li] = L.pstage;
    }
    a.hyp_in[li][0] = L.variance; a.hyp_in[li][1] = L.base_type == 1 ? L.acos_w : L.ls; a.hyp_in[li][2] = L.base_type == 1 ? L.acos_b : 1.0;
    DCGP_TRY(add(L.Z, L.gZ, L.aZ, (long)L.M * L.v.L, 0, -1, nullptr, (L.frozen & 1u) != 0));
    DCGP_TRY(add(L.q_mu, L.gq_mu, L.aq_mu, (long)L.M * L.R, 0, -1, nullptr, (L.frozen & 2u) != 0));
    if (L.has_qsqrt) DCGP_TRY(add(L.q_sqrt, L.gq_sqrt, L.aq_sqrt, (long)L.R * L.M * L.M, 0, -1, nullptr, (L.frozen & 4u) != 0));   // upper triangle: zero gradient, zero step
    if (L.is_head && L.w) DCGP_TRY(add(L.w, L.gw, L.aw, (long)L.v.P, 0, -1, nullptr, (L.frozen & 8u) != 0));
    const int ng_hyp = a.ng;
    DCGP_TRY(add(L.hyp, L.gscal, L.ahyp, 3, 1, li, nullptr, (L.frozen & 16u) != 0));
    if (a.ng > ng_hyp) a.grp[ng_hyp].hold = (int)((L.frozen >> 5) & 3u) << 1;   // bits 32 / 64: elements 1 / 2 of the triple stay where they are
    if (a.ng > ng_hyp && L.ard && !L.is_head) a.grp[ng_hyp].hold |= 2;          // an ARD conv layer: the scalar lengthscale is the unit the vector is measured in, held at 1
    if (L.ard) DCGP_TRY(add(L.ard, L.gard, L.aard, (long)L.v.L, 1, -1, L.in_scale, (L.frozen & (16u | 128u)) != 0));   // dense head, ARD conv layer: per-dimension lengthscales and the scale 1 / l
    if (L.mean_W) DCGP_TRY(add(L.mean_W, L.gmean_W, L.amean_W, (long)L.mean_slots(), 0, -1, nullptr, !L.mean_trainable));   // the mean filter (conv_mean.hip)
    if (L.mix_W) DCGP_TRY(add(L.mix_W, L.gmix_W, L.amix_W, (long)L.mix_slots(), 0, -1, nullptr, !L.mix_trainable));   // the mixing matrix (mix.hip), unconstrained
    if (L.glik) {   // Gaussian likelihood variance / StudentT scale: the last slot of the head's block, moments beside it on the device
      if (!model->d_lik) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: the head's block has a likelihood slot but the model no Gaussian likelihood", who);
      double* lik_mv[2] = {model->d_lik + 1, model->d_lik + 2};
      DCGP_TRY(add(model->d_lik, L.glik, lik_mv, 1, 1, -1, nullptr, model->lik_frozen));
    }
  }
  a.first_block[a.ng] = nb;
  if (nb <= 0) return DCGP_OK;
  if (clip) {   // norm and scale behind the gradient, in front of the update, on the step's stream
    if (model->clip_cap < (size_t)nb + 1) {
      HIP_TRY(ctx, hipDeviceSynchronize());   // (nothing may still read the smaller buffer)
      dev_free(ctx, model->d_clip); model->d_clip = nullptr; model->clip_cap = 0;
      if (dev_alloc(ctx, (void**)&model->d_clip, ((size_t)nb + 1) * sizeof(double), "d_clip") != hipSuccess)
        return ctx_fail(ctx, DCGP_ERR_ALLOC, "%s: allocation of the norm's %d partial sums failed", who, nb);
      model->clip_cap = (size_t)nb + 1;
    }
    a.clip = model->d_clip; a.max_norm = model->grad_clip; a.norm_out = a.host_out + kNormSlot;
    {
      ScopedTimer tm(ctx, "opt_norm");
      hipLaunchKernelGGL(opt_norm_partial_kernel, dim3(nb), dim3(256), 0, ctx->stream, a);
      LAUNCH_CHECK(ctx);
      hipLaunchKernelGGL(opt_norm_final_kernel, dim3(1), dim3(256), 0, ctx->stream, a, nb);
      LAUNCH_CHECK(ctx);
    }
    ScopedTimer tm(ctx, "opt_step_clip");
    hipLaunchKernelGGL(opt_step_kernel<true>, dim3(nb), dim3(256), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    model->norm_pending = true;
    return DCGP_OK;
  }
  {
    ScopedTimer tm(ctx, "opt_step");
    hipLaunchKernelGGL(opt_step_kernel<false>, dim3(nb), dim3(256), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
  }
  if (!sharded) return DCGP_OK;
  if (vranks > 0) {   // the other ranks' shards: into the staging block only
    for (int r = 1; r < vranks; ++r) {
      OptArgs b = a;
      b.stage_only = 1;
      for (int li = 0; li < nl; ++li) DCGP_TRY(dcgp_shard_range((long)model->layers[li]->grad_block_count(), vranks, r, &b.sh_lo[li], &b.sh_hi[li], nullptr));
      hipLaunchKernelGGL(opt_step_kernel<false>, dim3(nb), dim3(256), 0, ctx->stream, b);
      LAUNCH_CHECK(ctx);
    }
  } else {
    for (int li = 0; li < nl; ++li) DCGP_TRY(all_gather_f64_async(ctx, model->layers[li]->pstage, (size_t)shard[li]));
  }
  hipLaunchKernelGGL(opt_unstage_kernel, dim3(nb), dim3(256), 0, ctx->stream, a);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}
// the updated kernel hyper-parameters back into the host-side layer state (the stream must have been synchronised)
int opt_readback(dcgp_model* model) {
  const double* h = model->ctx->h_scratch;
  const int nl = (int)model->layers.size();
  if (model->norm_pending) {   // a clipped step: its pre-clip norm, beside the triples
    model->grad_norms.push_back(h[kNormSlot]);
    model->norm_pending = false;
  }
  for (int li = 0; li < nl; ++li) {
    LayerState& L = *model->layers[li];
    if (L.frozen & 16u) continue;
    L.variance = h[3 * li];
    if (L.base_type == 1) { L.acos_w = h[3 * li + 1]; L.acos_b = h[3 * li + 2]; } else L.ls = h[3 * li + 1];
  }
  return DCGP_OK;
}

// one optimiser step over every trainable group of the model (sgd: plain ascent, otherwise Adam with the bias-corrected rate lr)
static int opt_step(dcgp_model* model, const char* who, bool sgd, double lr, double beta1, double beta2, double eps, int vranks = 0) {
  DCGP_TRY(opt_enqueue(model, who, sgd, lr, beta1, beta2, eps, nullptr, vranks));
  HIP_TRY(model->ctx, hipStreamSynchronize(model->ctx->stream));
  return opt_readback(model);
}

extern "C" {

int dcgp_model_adam_step(dcgp_model* model, double lr, double beta1, double beta2, double eps, int t) {
  if (!model || t < 0 || !(lr > 0) || !(beta1 >= 0 && beta1 < 1) || !(beta2 >= 0 && beta2 < 1) || !(eps > 0))
    return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "adam_step: bad arguments") : DCGP_ERR_ARG;
  // t == 0: the model's own count of Adam steps since its moment buffers were created (they start at zero with it) --
  // what tf.train.AdamOptimizer's beta powers do for a freshly built optimiser, whatever global_step a checkpoint carried
  if (t == 0) t = ++model->adam_t; else model->adam_t = t;
  const double lr_t = lr * sqrt(1.0 - pow(beta2, (double)t)) / (1.0 - pow(beta1, (double)t));
  model->grad_norms.clear();
  return opt_step(model, "adam_step", false, lr_t, beta1, beta2, eps);
}

// Multi-rank training step: how the ranks exchange a step's gradient (0: all-reduce, every rank updates everything; 1: reduce-scatter, each rank
// updates its shard of every layer's parameter block, all-gather of the parameters -- SURVEY section 5).  Applies to dcgp_model_train_step_adam;
// dcgp_elbo_grad alone always all-reduces (its caller wants the whole gradient).
int dcgp_model_set_grad_exchange(dcgp_model* model, int mode) {
  if (!model || (mode != 0 && mode != 1)) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "set_grad_exchange: mode 0 or 1") : DCGP_ERR_ARG;
  if (mode == 0 && model->grad_exchange == 1 && model->sharded_steps > 0)
    return ctx_fail(model->ctx, DCGP_ERR_ARG, "set_grad_exchange: %llu sharded Adam steps were taken: the moments are rank-local (each rank holds its own shard's), "
                    "the all-reduce route cannot continue from them", (unsigned long long)model->sharded_steps);
  model->grad_exchange = mode;
  return DCGP_OK;
}
// Debugging aid: one Adam step (dcgp_model_adam_step's arguments) taken the way `ranks` ranks would take it in exchange mode 1, played on this one
// GPU from rank 0's point of view -- shard 0 updated in place, the other shards through the staging block and the unstage pass.  The gradient must be
// the complete one (dcgp_elbo_grad).  Parameters and moments come out bit-identical to dcgp_model_adam_step's (tests/test_gpu_model.py).
int dcgp_model_debug_sharded_adam(dcgp_model* model, int ranks, double lr, double beta1, double beta2, double eps, int t) {
  if (!model || ranks < 1 || t < 0 || !(lr > 0) || !(beta1 >= 0 && beta1 < 1) || !(beta2 >= 0 && beta2 < 1) || !(eps > 0))
    return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "debug_sharded_adam: bad arguments") : DCGP_ERR_ARG;
  if (model->grad_clip > 0.0)   // (refused in front of the step count: opt_enqueue's own check is the multi-rank step's)
    return ctx_fail(model->ctx, DCGP_ERR_ARG, "debug_sharded_adam: gradient clipping is on (dcgp_model_set_grad_clip) and the update is sharded: a rank sees "
                    "only its shard of the gradient, the global norm is not formed across ranks");
  if (t == 0) t = ++model->adam_t; else model->adam_t = t;
  const double lr_t = lr * sqrt(1.0 - pow(beta2, (double)t)) / (1.0 - pow(beta1, (double)t));
  model->grad_norms.clear();
  return opt_step(model, "debug_sharded_adam", false, lr_t, beta1, beta2, eps, ranks);
}

int dcgp_model_sgd_step(dcgp_model* model, double lr) {
  if (!model || !(lr > 0)) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "sgd_step: bad arguments") : DCGP_ERR_ARG;
  model->grad_norms.clear();
  return opt_step(model, "sgd_step", true, lr, 0.0, 0.0, 0.0);
}

int dcgp_model_set_trainable(dcgp_model* model, int layer, const char* which, int on) {
  if (!model || !which) return DCGP_ERR_ARG;
  if (!strcmp(which, "likelihood_variance")) {   // model-wide, `layer` is ignored
    if (model->lik_kind != 1) return ctx_fail(model->ctx, DCGP_ERR_ARG, "set_trainable(likelihood_variance): not a Gaussian-likelihood model");
    model->lik_frozen = !on;
    return DCGP_OK;
  }
  if (!strcmp(which, "likelihood_scale")) {   // model-wide, `layer` is ignored
    if (model->lik_kind != 4) return ctx_fail(model->ctx, DCGP_ERR_ARG, "set_trainable(likelihood_scale): not a StudentT-likelihood model");
    model->lik_frozen = !on;
    return DCGP_OK;
  }
  if (layer < 0 || layer >= (int)model->layers.size()) return ctx_fail(model->ctx, DCGP_ERR_ARG, "set_trainable: no layer %d", layer);
  LayerState& L = *model->layers[layer];
  if (!strcmp(which, "mean_filter")) {
    if (!L.mean_W) return ctx_fail(model->ctx, DCGP_ERR_ARG, "set_trainable(mean_filter): layer %d has no mean filter (dcgp_model_set_mean_filter)", layer);
    L.mean_trainable = on != 0;
    return DCGP_OK;
  }
  if (!strcmp(which, "mixing")) {
    if (!L.mix_W) return ctx_fail(model->ctx, DCGP_ERR_ARG, "set_trainable(mixing): layer %d is not mixed (dcgp_model_set_mixing)", layer);
    L.mix_trainable = on != 0;
    return DCGP_OK;
  }
  unsigned bit = 0;
  if (!strcmp(which, "Z")) bit = 1u;
  else if (!strcmp(which, "q_mu")) bit = 2u;
  else if (!strcmp(which, "q_sqrt")) bit = 4u;
  else if (!strcmp(which, "w")) bit = 8u;
  else if (!strcmp(which, "variance") || !strcmp(which, "lengthscale") || !strcmp(which, "hyper")) bit = 16u;
  else if (L.base_type == 1 && !strcmp(which, "weight_variances")) bit = 32u;   // one ArcCosine parameter alone (the other and the variance go on moving)
  else if (L.base_type == 1 && !strcmp(which, "bias_variance")) bit = 64u;
  else if (!strcmp(which, "ard_lengthscales")) {   // the per-dimension lengthscales alone (the variance goes on moving; "hyper" holds both)
    if (!L.ard) return ctx_fail(model->ctx, DCGP_ERR_ARG, "set_trainable(ard_lengthscales): layer %d has no ARD lengthscales", layer);
    bit = 128u;
  }
  else return ctx_fail(model->ctx, DCGP_ERR_ARG, "set_trainable: unknown parameter '%s'", which);
  if (on) L.frozen &= ~bit; else L.frozen |= bit;
  return DCGP_OK;
}

int dcgp_model_get_param(dcgp_model* model, int layer, const char* which, double* out_host, size_t count) {
  if (!model || !which || !out_host) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (!strcmp(which, "likelihood_variance")) {   // model-wide, `layer` is ignored
    if (model->lik_kind != 1) return ctx_fail(ctx, DCGP_ERR_ARG, "get_param(likelihood_variance): not a Gaussian-likelihood model");
    if (count != 1) return ctx_fail(ctx, DCGP_ERR_ARG, "get_param(likelihood_variance): expected 1 value");
    HIP_TRY(ctx, hipMemcpyAsync(out_host, model->d_lik, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DCGP_OK;
  }
  if (!strcmp(which, "likelihood_scale")) {   // model-wide, `layer` is ignored
    if (model->lik_kind != 4) return ctx_fail(ctx, DCGP_ERR_ARG, "get_param(likelihood_scale): not a StudentT-likelihood model");
    if (count != 1) return ctx_fail(ctx, DCGP_ERR_ARG, "get_param(likelihood_scale): expected 1 value");
    HIP_TRY(ctx, hipMemcpyAsync(out_host, model->d_lik, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DCGP_OK;
  }
  if (layer < 0 || layer >= (int)model->layers.size()) return ctx_fail(ctx, DCGP_ERR_ARG, "get_param: no layer %d", layer);
  LayerState& L = *model->layers[layer];
  const double* src = nullptr;
  size_t n = 0;
  if (!strcmp(which, "variance") || !strcmp(which, "lengthscale") || !strcmp(which, "weight_variances") || !strcmp(which, "bias_variance")) {
    if (count != 1) return ctx_fail(ctx, DCGP_ERR_ARG, "get_param(%s): expected 1 value", which);
    out_host[0] = which[0] == 'v' ? L.variance : (which[0] == 'l' ? L.ls : (which[0] == 'w' ? L.acos_w : L.acos_b));
    return DCGP_OK;
  }
  if (!strcmp(which, "Z")) { src = L.Z; n = (size_t)L.M * L.v.L; }
  else if (!strcmp(which, "q_mu")) { src = L.q_mu; n = (size_t)L.M * L.R; }
  else if (!strcmp(which, "q_sqrt")) { src = L.q_sqrt; n = (size_t)L.R * L.M * L.M; }
  else if (!strcmp(which, "w")) {
    if (!L.w) return ctx_fail(ctx, DCGP_ERR_ARG, "get_param: only the head has patch weights");
    src = L.w; n = (size_t)L.v.P;
  } else if (!strcmp(which, "ard_lengthscales")) {
    if (!L.ard) return ctx_fail(ctx, DCGP_ERR_ARG, "get_param: this layer has no ARD lengthscales");
    src = L.ard; n = (size_t)L.v.L;
  } else if (!strcmp(which, "mean_filter")) {
    if (!L.mean_W) return ctx_fail(ctx, DCGP_ERR_ARG, "get_param: this layer has no mean filter");
    src = L.mean_W; n = L.mean_slots();
  } else if (!strcmp(which, "mixing")) {
    if (!L.mix_W) return ctx_fail(ctx, DCGP_ERR_ARG, "get_param: this layer is not mixed");
    src = L.mix_W; n = L.mix_slots();
  } else return ctx_fail(ctx, DCGP_ERR_ARG, "get_param: unknown parameter '%s'", which);
  if (count != n) return ctx_fail(ctx, DCGP_ERR_ARG, "get_param(%s): expected %zu values, got %zu", which, n, count);
  HIP_TRY(ctx, hipMemcpyAsync(out_host, src, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

int dcgp_model_get_grad(dcgp_model* model, int layer, const char* which, double* out_host, size_t count) {
  if (!model || !which || !out_host) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (!strcmp(which, "likelihood_variance")) {   // model-wide, `layer` is ignored: the last slot of the head's gradient block
    const LayerState* H = model->has_head ? model->layers.back().get() : nullptr;
    if (model->lik_kind != 1 || !H || !H->glik) return ctx_fail(ctx, DCGP_ERR_ARG, "get_grad(likelihood_variance): no Gaussian-likelihood gradient (dcgp_elbo_grad_f64y first)");
    if (count != 1) return ctx_fail(ctx, DCGP_ERR_ARG, "get_grad(likelihood_variance): expected 1 value");
    HIP_TRY(ctx, hipMemcpyAsync(out_host, H->glik, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DCGP_OK;
  }
  if (!strcmp(which, "likelihood_scale")) {   // model-wide, `layer` is ignored: the last slot of the head's gradient block
    const LayerState* H = model->has_head ? model->layers.back().get() : nullptr;
    if (model->lik_kind != 4 || !H || !H->glik) return ctx_fail(ctx, DCGP_ERR_ARG, "get_grad(likelihood_scale): no StudentT-likelihood gradient (dcgp_elbo_grad_f64y first)");
    if (count != 1) return ctx_fail(ctx, DCGP_ERR_ARG, "get_grad(likelihood_scale): expected 1 value");
    HIP_TRY(ctx, hipMemcpyAsync(out_host, H->glik, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DCGP_OK;
  }
  if (layer < 0 || layer >= (int)model->layers.size()) return ctx_fail(ctx, DCGP_ERR_ARG, "get_grad: no layer %d", layer);
  LayerState& L = *model->layers[layer];
  if (!L.gZ) return ctx_fail(ctx, DCGP_ERR_ARG, "get_grad: call dcgp_elbo_grad first");
  const double* src = nullptr;
  size_t n = 0;
  if (!strcmp(which, "Z")) { src = L.gZ; n = (size_t)L.M * L.v.L; }
  else if (!strcmp(which, "q_mu")) { src = L.gq_mu; n = (size_t)L.M * L.R; }
  else if (!strcmp(which, "q_sqrt")) { src = L.gq_sqrt; n = (size_t)L.R * L.M * L.M; }
  else if (!strcmp(which, "variance")) { src = L.gscal; n = 1; }
  else if (!strcmp(which, "lengthscale") || !strcmp(which, "weight_variances")) { src = L.gscal + 1; n = 1; }
  else if (!strcmp(which, "bias_variance")) { src = L.gscal + 2; n = 1; }
  else if (!strcmp(which, "w")) {
    if (!L.is_head) return ctx_fail(ctx, DCGP_ERR_ARG, "get_grad: only the head has patch weights");
    src = L.gw; n = (size_t)L.v.P;
  } else if (!strcmp(which, "ard_lengthscales")) {
    if (!L.ard || !L.gard) return ctx_fail(ctx, DCGP_ERR_ARG, "get_grad: this layer has no ARD lengthscales");
    src = L.gard; n = (size_t)L.v.L;
  } else if (!strcmp(which, "mean_filter")) {
    if (!L.mean_W || !L.gmean_W) return ctx_fail(ctx, DCGP_ERR_ARG, "get_grad: this layer has no mean filter");
    src = L.gmean_W; n = L.mean_slots();
  } else if (!strcmp(which, "mixing")) {
    if (!L.mix_W || !L.gmix_W) return ctx_fail(ctx, DCGP_ERR_ARG, "get_grad: this layer is not mixed");
    src = L.gmix_W; n = L.mix_slots();
  } else return ctx_fail(ctx, DCGP_ERR_ARG, "get_grad: unknown parameter '%s'", which);
  if (count != n) return ctx_fail(ctx, DCGP_ERR_ARG, "get_grad(%s): expected %zu values, got %zu", which, n, count);
  HIP_TRY(ctx, hipMemcpyAsync(out_host, src, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

// Adam's moments of one parameter group (names as dcgp_model_get_param's groups; "hyper": the triple, "likelihood": the model's one slot)
static int adam_group(dcgp_model* model, int layer, const char* which, const char* who, size_t count, double** m, double** v) {
  dcgp_ctx* ctx = model->ctx;
  if (model->sharded_steps > 0)
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: %llu sharded Adam steps were taken on this model (exchange mode 1): its moments cover this rank's shard only",
                    who, (unsigned long long)model->sharded_steps);
  size_t n = 0;
  if (!strcmp(which, "likelihood")) {   // model-wide, `layer` is ignored
    if (!model->d_lik || (model->lik_kind != 1 && model->lik_kind != 4))
      return ctx_fail(ctx, DCGP_ERR_ARG, "%s(likelihood): this model's likelihood has no trainable parameter", who);
    *m = model->d_lik + 1; *v = model->d_lik + 2; n = 1;
  } else {
    if (layer < 0 || layer >= (int)model->layers.size()) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: no layer %d", who, layer);
    LayerState& L = *model->layers[layer];
    DCGP_TRY(L.ensure_adam());
    double* const* mv = nullptr;
    if (!strcmp(which, "Z")) { mv = L.aZ; n = (size_t)L.M * L.v.L; }
    else if (!strcmp(which, "q_mu")) { mv = L.aq_mu; n = (size_t)L.M * L.R; }
    else if (!strcmp(which, "q_sqrt")) { mv = L.aq_sqrt; n = (size_t)L.R * L.M * L.M; }
    else if (!strcmp(which, "hyper")) { mv = L.ahyp; n = 3; }
    else if (!strcmp(which, "w")) {
      if (!L.is_head || !L.w) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: only the head has patch weights", who);
      mv = L.aw; n = (size_t)L.v.P;
    } else if (!strcmp(which, "ard_lengthscales")) {
      if (!L.ard) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: this layer has no ARD lengthscales", who);
      mv = L.aard; n = (size_t)L.v.L;
    } else if (!strcmp(which, "mean_filter")) {
      if (!L.mean_W) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: this layer has no mean filter", who);
      mv = L.amean_W; n = L.mean_slots();
    } else if (!strcmp(which, "mixing")) {
      if (!L.mix_W) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: this layer is not mixed", who);
      mv = L.amix_W; n = L.mix_slots();
    } else return ctx_fail(ctx, DCGP_ERR_ARG, "%s: unknown parameter group '%s'", who, which);
    if (!mv[0] || !mv[1]) return ctx_fail(ctx, DCGP_ERR_ARG, "%s(%s): the group has no moment buffers", who, which);
    *m = mv[0]; *v = mv[1];
  }
  if (count != n) return ctx_fail(ctx, DCGP_ERR_ARG, "%s(%s): expected %zu values, got %zu", who, which, n, count);
  return DCGP_OK;
}

int dcgp_model_get_adam_state(dcgp_model* model, int layer, const char* which, double* m_host, double* v_host, size_t count) {
  if (!model || !which || !m_host || !v_host) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "get_adam_state: NULL pointer") : DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  double *m = nullptr, *v = nullptr;
  DCGP_TRY(adam_group(model, layer, which, "get_adam_state", count, &m, &v));
  HIP_TRY(ctx, hipMemcpyAsync(m_host, m, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(v_host, v, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

int dcgp_model_set_adam_state(dcgp_model* model, int layer, const char* which, const double* m_host, const double* v_host, size_t count) {
  if (!model || !which || !m_host || !v_host) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "set_adam_state: NULL pointer") : DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (model->enq_seq != model->col_seq) return ctx_fail(ctx, DCGP_ERR_ARG, "set_adam_state: enqueued steps are still to be collected");
  double *m = nullptr, *v = nullptr;
  DCGP_TRY(adam_group(model, layer, which, "set_adam_state", count, &m, &v));
  HIP_TRY(ctx, hipMemcpyAsync(m, m_host, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(v, v_host, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

int dcgp_model_get_adam_t(dcgp_model* model, int* t) {
  if (!model || !t) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "get_adam_t: NULL pointer") : DCGP_ERR_ARG;
  *t = model->adam_t;
  return DCGP_OK;
}

int dcgp_model_set_adam_t(dcgp_model* model, int t) {
  if (!model) return DCGP_ERR_ARG;
  if (t < 0) return ctx_fail(model->ctx, DCGP_ERR_ARG, "set_adam_t: t must be >= 0, got %d", t);
  if (model->enq_seq != model->col_seq) return ctx_fail(model->ctx, DCGP_ERR_ARG, "set_adam_t: enqueued steps are still to be collected");
  model->adam_t = t;
  return DCGP_OK;
}

int dcgp_model_set_grad_clip(dcgp_model* model, double max_norm) {
  if (!model) return DCGP_ERR_ARG;
  if (!(max_norm >= 0.0)) return ctx_fail(model->ctx, DCGP_ERR_ARG, "set_grad_clip: max_norm must be >= 0 (0: off, +inf: measure only), got %g", max_norm);
  if (model->enq_seq != model->col_seq) return ctx_fail(model->ctx, DCGP_ERR_ARG, "set_grad_clip: enqueued steps are still to be collected");
  model->grad_clip = max_norm;
  model->grad_norms.clear();
  return DCGP_OK;
}

int dcgp_model_grad_norms(dcgp_model* model, double* out_host, int cap, int* count_out) {
  if (!model || !count_out || cap < 0 || (cap > 0 && !out_host)) return model ? ctx_fail(model->ctx, DCGP_ERR_ARG, "grad_norms: bad arguments") : DCGP_ERR_ARG;
  const int n = (int)model->grad_norms.size();
  *count_out = n;
  for (int i = 0; i < n && i < cap; ++i) out_host[i] = model->grad_norms[i];
  return DCGP_OK;
}

int dcgp_model_set_grad_shards(dcgp_model* model, int shards) {
  if (!model || shards < 0) return DCGP_ERR_ARG;
  model->grad_shards = shards;
  return DCGP_OK;
}

int dcgp_model_grad_block(dcgp_model* model, int layer, double** block_dev, size_t* count) {
  if (!model || !block_dev || !count) return DCGP_ERR_ARG;
  if (layer < 0 || layer >= (int)model->layers.size()) return ctx_fail(model->ctx, DCGP_ERR_ARG, "grad_block: no layer %d", layer);
  LayerState& L = *model->layers[layer];
  DCGP_TRY(L.ensure_grads());
  *block_dev = L.gZ;
  *count = L.grad_block_count();
  return DCGP_OK;
}

}  // extern "C"

// A training run on the device: the training set is uploaded once (dcgp_model_set_dataset) and K Adam steps, each on its own rows of it and at its
// own learning rate, go through one call (dcgp_model_train_run_adam) -- gpflow.actions.Loop(self.loop, stop=test_every) of the reference's
// Experiment._optimize with the optimiser it set up (conv_gp/experiment.py:38-49,84-108).  A step of the run is dcgp_model_train_step_adam on a
// batch that a gather kernel writes from the resident set: no image crosses the bus per step, and the results are that call's bit for bit.
// With an augmentation set (dcgp_model_set_augmentation) the gather is augment.hip's, which also shifts and flips each image by a draw made on the
// device; without one it is gather_batch_kernel below, as it always was.
//
// Stream order.  Every step of the run ends in the wait dcgp_model_train_step_adam ends in, and the host enqueues step i + 1 behind it.  It has to:
// the kernels of a step take the base kernels' hyper-parameters (variance, lengthscale) by value from the host-side layer state, which the update of
// step i writes (opt_readback) -- step i + 1 cannot be enqueued before step i's update has been read back.  What follows from the wait:
//   - step i + 1's parameter-only chain starts behind step i's update on whichever stream it runs (the update is the last command of the main
//     stream, which the host has waited for);
//   - ONE set of batch buffers is enough: the gather of step i + 1 is enqueued on the ctx stream, the main stream of a step that is not pipelined.
//     The readers of step i's batch on the side streams (the reverse pass) are joined into the main stream in front of step i's update
//     (model_backward joins once, at the end), so they are over when the host's wait returns; the readers of step i + 1's batch are the first
//     layer's launches on the same stream behind the gather, and everything else of the step is ordered behind those by the step's own events;
//   - a step that fails is the last one enqueued: the run returns there, and no later update exists that a run-level status word would have to stop
//     (the failed step's own update reads the step's status word on the device, as in dcgp_model_train_step_adam).
#include <vector>

#include "model_state.h"

namespace {

// rows idx[0 .. batch) of the resident set into the step's batch: one workgroup per row, consecutive lanes on consecutive doubles (rows of any
// length: 189 = 9 x 7 x 3, 338, 784, 3072).  Targets: int32 labels (D == 0) or D doubles per row.  The host has checked 0 <= idx < n.
__global__ __launch_bounds__(256) void gather_batch_kernel(const double* __restrict__ X, long len, const int32_t* __restrict__ idx, int batch, long n,
                                                           double* __restrict__ Xb, const int32_t* __restrict__ y32, const double* __restrict__ yf,
                                                           int D, int32_t* __restrict__ yb32, double* __restrict__ ybf) {
  const int b = blockIdx.x;
  if (b >= batch) return;
  const long r = idx[b];
  if (r < 0 || r >= n) return;
  const double* src = X + r * len;
  double* dst = Xb + (long)b * len;
  for (long j = threadIdx.x; j < len; j += 256) dst[j] = src[j];
  if (D == 0) {
    if (threadIdx.x == 0) yb32[b] = y32[r];
  } else {
    for (int j = threadIdx.x; j < D; j += 256) ybf[(long)b * D + j] = yf[r * D + j];
  }
}

template <class T>
int grow(dcgp_ctx* ctx, T** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes && *p) return DCGP_OK;
  if (*p) { HIP_TRY(ctx, hipDeviceSynchronize()); dev_free(ctx, *p); *p = nullptr; *cap = 0; }
  if (dev_alloc(ctx, (void**)p, bytes, "train_run") != hipSuccess) return ctx_fail(ctx, DCGP_ERR_ALLOC, "train_run: allocation of %zu bytes failed", bytes);
  *cap = bytes;
  return DCGP_OK;
}

bool float_targets(const dcgp_model* m) { return m->lik_kind == 1 || m->lik_kind == 2 || m->lik_kind == 4 || m->lik_kind == 5; }

}  // namespace

extern "C" {

int dcgp_model_set_dataset(dcgp_model* model, const double* X_host, const void* Y_host, long n, int y_is_f64) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (n < 0 || (n > 0 && (!X_host || !Y_host))) return ctx_fail(ctx, DCGP_ERR_ARG, "set_dataset: bad args");
  if (model->enq_seq != model->col_seq) return ctx_fail(ctx, DCGP_ERR_ARG, "set_dataset: enqueued steps are still to be collected");
  if (model->ds_X || model->ds_Y) {   // nothing may still read the earlier set
    HIP_TRY(ctx, hipDeviceSynchronize());
    dev_free(ctx, model->ds_X); dev_free(ctx, model->ds_Y);
    model->ds_X = nullptr; model->ds_Y = nullptr; model->ds_n = 0; model->ds_len = 0; model->ds_D = 0;
  }
  if (n == 0) return DCGP_OK;
  if (!model->has_head || model->layers.empty()) return ctx_fail(ctx, DCGP_ERR_ARG, "set_dataset: the model has no head layer yet");
  if ((y_is_f64 != 0) != float_targets(model))
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_dataset: this model's likelihood takes %s targets", float_targets(model) ? "float64 [n][D]" : "int32 labels");
  const long len = model->image_len();   // the caller's images: a padded first layer pads them on the device
  const int D = y_is_f64 ? model->layers.back()->R : 0;
  const size_t xb = (size_t)n * len * sizeof(double), yb = y_is_f64 ? (size_t)n * D * sizeof(double) : (size_t)n * sizeof(int32_t);
  if (dev_alloc(ctx, (void**)&model->ds_X, xb, "dataset_X") != hipSuccess || dev_alloc(ctx, &model->ds_Y, yb, "dataset_Y") != hipSuccess) {
    dev_free(ctx, model->ds_X); dev_free(ctx, model->ds_Y);
    model->ds_X = nullptr; model->ds_Y = nullptr;
    return ctx_fail(ctx, DCGP_ERR_ALLOC, "set_dataset: allocation of %zu + %zu bytes failed", xb, yb);
  }
  HIP_TRY(ctx, hipMemcpy(model->ds_X, X_host, xb, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(model->ds_Y, Y_host, yb, hipMemcpyHostToDevice));
  model->ds_n = n; model->ds_len = len; model->ds_D = D;
  return DCGP_OK;
}

int dcgp_model_set_augmentation(dcgp_model* model, int H, int W, int C, int max_shift, int hflip) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (model->enq_seq != model->col_seq) return ctx_fail(ctx, DCGP_ERR_ARG, "set_augmentation: enqueued steps are still to be collected");
  if (max_shift == 0 && hflip == 0) {   // off: the geometry plays no part
    model->aug_H = model->aug_W = model->aug_C = model->aug_shift = model->aug_hflip = 0;
    return DCGP_OK;
  }
  if (!model->has_head || model->layers.empty()) return ctx_fail(ctx, DCGP_ERR_ARG, "set_augmentation: the model has no head layer yet");
  if (const char* why = augment_geometry_error(H, W, C, max_shift))
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_augmentation: %s (H %d W %d C %d max_shift %d)", why, H, W, C, max_shift);
  if ((long)H * W * C != model->image_len())
    return ctx_fail(ctx, DCGP_ERR_ARG, "set_augmentation: %d x %d x %d is not the model's image of %ld values", H, W, C, model->image_len());
  model->aug_H = H; model->aug_W = W; model->aug_C = C; model->aug_shift = max_shift; model->aug_hflip = hflip != 0;
  return DCGP_OK;
}

int dcgp_model_train_run_adam(dcgp_model* model, const int32_t* idx_host, int steps, int batch, double scale, const double* lr_host, uint64_t seed0,
                              int dedup_layer0, double beta1, double beta2, double eps, double* elbo_host, int* steps_done, int* info_host) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (steps_done) *steps_done = 0;
  if (info_host) *info_host = 0;
  // everything is checked before anything is enqueued: a bad index never reaches a kernel
  if (!idx_host || !lr_host || !elbo_host || !steps_done) return ctx_fail(ctx, DCGP_ERR_ARG, "train_run_adam: NULL pointer");
  if (steps < 1 || batch < 1) return ctx_fail(ctx, DCGP_ERR_ARG, "train_run_adam: steps and batch must be >= 1");
  if (ctx->comm && ctx->nranks > 1) return ctx_fail(ctx, DCGP_ERR_ARG, "train_run_adam: a run drives one GPU (this ctx holds %d ranks)", ctx->nranks);
  if (!model->ds_X || model->ds_n <= 0) return ctx_fail(ctx, DCGP_ERR_ARG, "train_run_adam: no dataset attached (dcgp_model_set_dataset)");
  if (model->enq_seq != model->col_seq) return ctx_fail(ctx, DCGP_ERR_ARG, "train_run_adam: enqueued steps are still to be collected");
  if (!(beta1 >= 0 && beta1 < 1) || !(beta2 >= 0 && beta2 < 1) || !(eps > 0)) return ctx_fail(ctx, DCGP_ERR_ARG, "train_run_adam: bad optimiser arguments");
  if (model->augmenting() && (long)model->aug_H * model->aug_W * model->aug_C != model->ds_len)
    return ctx_fail(ctx, DCGP_ERR_ARG, "train_run_adam: the augmentation's %d x %d x %d images are not the attached set's rows of %ld", model->aug_H,
                    model->aug_W, model->aug_C, model->ds_len);
  for (int i = 0; i < steps; ++i)
    if (!(lr_host[i] > 0)) return ctx_fail(ctx, DCGP_ERR_ARG, "train_run_adam: learning rate of step %d is not > 0", i);
  const size_t count = (size_t)steps * batch;
  for (size_t k = 0; k < count; ++k)
    if (idx_host[k] < 0 || idx_host[k] >= model->ds_n)
      return ctx_fail(ctx, DCGP_ERR_ARG, "train_run_adam: index %d (step %zu, position %zu) is outside the dataset's %ld rows", idx_host[k], k / batch,
                      k % batch, model->ds_n);
  const long len = model->ds_len;
  const int D = model->ds_D;
  DCGP_TRY(grow(ctx, &model->run_idx, &model->run_idx_cap, count * sizeof(int32_t)));
  DCGP_TRY(grow(ctx, &model->run_X, &model->run_X_cap, (size_t)batch * len * sizeof(double)));
  DCGP_TRY(grow(ctx, &model->run_Y, &model->run_Y_cap, D ? (size_t)batch * D * sizeof(double) : (size_t)batch * sizeof(int32_t)));
  HIP_TRY(ctx, hipMemcpy(model->run_idx, idx_host, count * sizeof(int32_t), hipMemcpyHostToDevice));   // the whole table, once per run
  const int32_t* y32 = D ? nullptr : (const int32_t*)model->ds_Y;
  const double* yf = D ? (const double*)model->ds_Y : nullptr;
  int32_t* yb32 = D ? nullptr : (int32_t*)model->run_Y;
  double* ybf = D ? (double*)model->run_Y : nullptr;
  const bool augment = model->augmenting();
  model->grad_norms.clear();   // clipping on: every step's wait leaves its pre-clip norm here (opt_readback)
  for (int i = 0; i < steps; ++i) {
    if (augment) {   // the same rows, each shifted and flipped by the draw of (this step's seed, its batch position)
      DCGP_TRY(gather_augment_batch(model, model->run_idx + (size_t)i * batch, batch, seed0 + (uint64_t)i, y32, yf, D, yb32, ybf));
    } else {
      hipLaunchKernelGGL(gather_batch_kernel, dim3(batch), dim3(256), 0, ctx->stream, model->ds_X, len, model->run_idx + (size_t)i * batch, batch,
                         model->ds_n, model->run_X, y32, yf, D, yb32, ybf);
      LAUNCH_CHECK(ctx);
    }
    double out[3] = {0.0, 0.0, 0.0};
    const int rc = train_step_adam_run(model, model->run_X, yb32, batch, scale, nullptr, seed0 + (uint64_t)i, dedup_layer0, lr_host[i], beta1, beta2, eps,
                                       0, out, info_host, ybf);
    if (rc != DCGP_OK) return rc;   // the per-step loop's failure: parameters, moments and step count as that step left them
    elbo_host[i] = out[0];
    *steps_done = i + 1;
  }
  return DCGP_OK;
}

}  // extern "C"

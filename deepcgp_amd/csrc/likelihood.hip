// likelihood.hip -- the one place that knows which likelihood a model has (host code only: no kernels).  Every function takes the
// Likelihood and the Targets (layer.h) and dispatches once on the kind to the launchers of cond.hip / evaluate.hip / uncertainty.hip /
// grad.hip / input_grad.hip (RobustMax), softmax.hip and pointwise.hip (Gaussian, Bernoulli, StudentT, Poisson); what differs between
// their argument lists ends here.
#include "layer_impl.h"

int lik_check_targets(dcgp_ctx* ctx, const Likelihood& lik, const Targets& t, const char* who) {
  if (lik.float_targets() != t.f64 && (lik.kind == 4 || lik.kind == 5))
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: a StudentT- or Poisson-likelihood model takes float64 targets (the _f64y entry points)", who);
  if (lik.float_targets() != t.f64)
    return ctx_fail(ctx, DCGP_ERR_ARG, t.f64 ? "%s: a RobustMax or Softmax model takes int32 labels, not float64 targets"
                                             : "%s: a Gaussian- or Bernoulli-likelihood model takes float64 targets (the _f64y entry points)", who);
  if (lik.kind == 3 && !lik.nodes) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: the Softmax likelihood has no node table yet (dcgp_model_set_likelihood_nodes)", who);
  return DCGP_OK;
}

int lik_elbo_tail(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, const Targets& t, int n_rows, int n_labels, int K,
                  double* ve_rows, double inv_s, double* scal, const ElboFinish& fin, const KlTail* kl) {
  switch (lik.kind) {
    case 3: return softmax_elbo_tail(ctx, mu, var, t.labels, n_rows, n_labels, K, lik.nodes, lik.Q, ve_rows, inv_s, scal, fin, kl);
    case 1:
    case 2:
    case 4:
    case 5: return quad_elbo_tail(ctx, lik.quad(), mu, var, t.values, n_rows, n_labels, K, ve_rows, inv_s, scal, fin, kl);
    default: return elbo_tail(ctx, mu, var, t.labels, n_rows, n_labels, K, lik.eps, ve_rows, inv_s, scal, fin, kl);
  }
}

int lik_grad_seeds(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, const Targets& t, int rows, int n_labels, int K,
                   double weight, double* gm, double* gv, double* gs2) {
  if (lik.kind == 1 && (!lik.s2 || !gs2)) return ctx_fail(ctx, DCGP_ERR_ARG, "grad: the Gaussian likelihood has no variance on the device");
  if (lik.kind == 4 && (!lik.s2 || !gs2)) return ctx_fail(ctx, DCGP_ERR_ARG, "grad: the StudentT likelihood has no scale on the device");
  switch (lik.kind) {
    case 3: return softmax_grad(ctx, mu, var, t.labels, rows, n_labels, K, lik.nodes, lik.Q, weight, gm, gv);
    case 1:
    case 2:
    case 4:
    case 5: return quad_grad(ctx, lik.quad(), mu, var, t.values, rows, K, n_labels, weight, gm, gv, lik.n_params() ? gs2 : nullptr);
    default: return robustmax_grad(ctx, mu, var, t.labels, rows, n_labels, K, lik.eps, weight, gm, gv);
  }
}

int lik_predict(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, long n, double* out_mean, double* out_var) {
  switch (lik.kind) {
    case 1:
    case 2:
    case 4:
    case 5: return quad_elementwise(ctx, lik.quad(), 1, mu, var, nullptr, n, out_mean, out_var);
    default: return ctx_fail(ctx, DCGP_ERR_ARG, "predict_mean_var: not a Gaussian- or Bernoulli-likelihood model (dcgp_model_predict_y)");
  }
}

int lik_class_probs(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, int rows, int K, double* out_p) {
  switch (lik.kind) {
    case 1:
    case 2: return ctx_fail(ctx, DCGP_ERR_ARG, "predict_y: a Gaussian- or Bernoulli-likelihood model predicts with dcgp_model_predict_mean_var");
    case 4:
    case 5: return ctx_fail(ctx, DCGP_ERR_ARG, "predict_y: a StudentT- or Poisson-likelihood model predicts with dcgp_model_predict_mean_var");
    case 3:
      if (!lik.nodes) return ctx_fail(ctx, DCGP_ERR_ARG, "predict_y: the Softmax likelihood has no node table yet (dcgp_model_set_likelihood_nodes)");
      return softmax_predict(ctx, mu, var, rows, K, lik.nodes, lik.Q, out_p, nullptr);
    default:
      if (K < 2) return ctx_fail(ctx, DCGP_ERR_ARG, "predict_y: the last layer has %d outputs, RobustMax needs >= 2", K);
      return varexp_rows(ctx, mu, var, nullptr, rows, 1, K, lik.eps, out_p, 1);
  }
}

int lik_eval_tail(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, const Targets& all, int n, int S, int K, long lo,
                  const EvalOut& o) {
  const Targets t = all.from(lo);
  switch (lik.kind) {
    case 1:
    case 2:
    case 4:
    case 5: return quad_eval_tail(ctx, lik.quad(), mu, var, t.values, n, S, K, lo, o.logdens, o.ld_nd, o.p_mean, o.score);
    case 3: return softmax_eval_tail(ctx, mu, var, t.labels, n, S, K, lik.nodes, lik.Q, lo, o.logdens, o.p_mean, o.ok);
    default: return eval_tail(ctx, mu, var, t.labels, n, S, K, lik.eps, lo, o.logdens, o.p_mean, o.ok);
  }
}

int lik_eval_sum(dcgp_ctx* ctx, const Likelihood& lik, const EvalOut& o, long n, const FactorStatus& st, double* res) {
  if (lik.float_targets()) return quad_eval_sum(ctx, o.logdens, o.score, n, st, res);   // (the scores: squared errors; Bernoulli: correct counts)
  return eval_sum(ctx, o.logdens, o.ok, n, st, res);                                      // (Softmax: eval_tail's outputs, the same sum)
}

int lik_unc_tail(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, const Targets& all, int n, int S, int K, long lo,
                 const UncOut& o) {
  const Targets t = all.from(lo);
  switch (lik.kind) {
    case 1: return ctx_fail(ctx, DCGP_ERR_ARG, "evaluate_uncertainty: class probabilities need a classification likelihood, this model is Gaussian");
    case 2: return bern_unc_tail(ctx, mu, var, t.values, n, S, K, lo, o);
    case 4: return ctx_fail(ctx, DCGP_ERR_ARG, "evaluate_uncertainty: class probabilities need a classification likelihood, this model is StudentT");
    case 5: return ctx_fail(ctx, DCGP_ERR_ARG, "evaluate_uncertainty: class probabilities need a classification likelihood, this model is Poisson");
    case 3: return softmax_unc_tail(ctx, mu, var, t.labels, n, S, K, lik.nodes, lik.Q, lo, o);
    default: return unc_tail(ctx, mu, var, t.labels, n, S, K, lik.eps, lo, o);
  }
}

int lik_density_max_k(const Likelihood& lik) { return lik.kind == 3 ? 4096 : kRmDensityMaxK; }

int lik_density_grad(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, const int32_t* y, int n_img, int S, int K, double* J,
                     double* gm, double* gv) {
  switch (lik.kind) {
    case 1:
    case 2:
    case 4:
    case 5: return ctx_fail(ctx, DCGP_ERR_ARG, "input_grad: the density objective exists for the RobustMax and Softmax likelihoods only");
    case 3: return softmax_density_grad(ctx, mu, var, y, n_img, S, K, lik.nodes, lik.Q, J, gm, gv);
    default: return rm_density_grad(ctx, mu, var, y, n_img, S, K, lik.eps, J, gm, gv);
  }
}

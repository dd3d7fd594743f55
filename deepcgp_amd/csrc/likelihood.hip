// likelihood.hip -- the one place that knows which likelihood a model has (host code only: no kernels).  Every function takes the
// Likelihood and the Targets (layer.h) and dispatches once on the kind to the launchers of cond.hip / evaluate.hip / uncertainty.hip /
// grad.hip (RobustMax), gaussian.hip and bernoulli.hip; what differs between their argument lists ends here.
#include "layer_impl.h"

int lik_check_targets(dcgp_ctx* ctx, const Likelihood& lik, const Targets& t, const char* who) {
  if (lik.float_targets() == t.f64) return DCGP_OK;
  return ctx_fail(ctx, DCGP_ERR_ARG, t.f64 ? "%s: a RobustMax model takes int32 labels, not float64 targets"
                                           : "%s: a Gaussian- or Bernoulli-likelihood model takes float64 targets (the _f64y entry points)", who);
}

int lik_elbo_tail(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, const Targets& t, int n_rows, int n_labels, int K,
                  double* ve_rows, double inv_s, double* scal, const ElboFinish& fin, const KlTail* kl) {
  switch (lik.kind) {
    case 1: return gauss_elbo_tail(ctx, mu, var, t.values, n_rows, n_labels, K, lik.s2, ve_rows, inv_s, scal, fin, kl);
    case 2: return bern_elbo_tail(ctx, mu, var, t.values, n_rows, n_labels, K, ve_rows, inv_s, scal, fin, kl);
    default: return elbo_tail(ctx, mu, var, t.labels, n_rows, n_labels, K, lik.eps, ve_rows, inv_s, scal, fin, kl);
  }
}

int lik_grad_seeds(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, const Targets& t, int rows, int n_labels, int K,
                   double weight, double* gm, double* gv, double* gs2) {
  switch (lik.kind) {
    case 1:
      if (!lik.s2 || !gs2) return ctx_fail(ctx, DCGP_ERR_ARG, "grad: the Gaussian likelihood has no variance on the device");
      return gauss_grad(ctx, mu, var, t.values, rows, K, n_labels, lik.s2, weight, gm, gv, gs2);
    case 2: return bern_grad(ctx, mu, var, t.values, rows, K, n_labels, weight, gm, gv);
    default: return robustmax_grad(ctx, mu, var, t.labels, rows, n_labels, K, lik.eps, weight, gm, gv);
  }
}

int lik_predict(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, long n, double* out_mean, double* out_var) {
  switch (lik.kind) {
    case 1: return gauss_predict(ctx, mu, var, n, lik.s2, out_mean, out_var);
    case 2: return bern_predict(ctx, mu, var, n, out_mean, out_var);
    default: return ctx_fail(ctx, DCGP_ERR_ARG, "predict_mean_var: not a Gaussian- or Bernoulli-likelihood model (dcgp_model_predict_y)");
  }
}

int lik_eval_tail(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, const Targets& all, int n, int S, int K, long lo,
                  const EvalOut& o) {
  const Targets t = all.from(lo);
  switch (lik.kind) {
    case 1: return gauss_eval_tail(ctx, mu, var, t.values, n, S, K, lik.s2, lo, o.logdens, o.ld_nd, o.p_mean, o.score);
    case 2: return bern_eval_tail(ctx, mu, var, t.values, n, S, K, lo, o.logdens, o.ld_nd, o.p_mean, o.score);
    default: return eval_tail(ctx, mu, var, t.labels, n, S, K, lik.eps, lo, o.logdens, o.p_mean, o.ok);
  }
}

int lik_eval_sum(dcgp_ctx* ctx, const Likelihood& lik, const EvalOut& o, long n, const FactorStatus& st, double* res) {
  if (lik.float_targets()) return gauss_eval_sum(ctx, o.logdens, o.score, n, st, res);   // (Bernoulli: the same sum over its correct counts)
  return eval_sum(ctx, o.logdens, o.ok, n, st, res);
}

int lik_unc_tail(dcgp_ctx* ctx, const Likelihood& lik, const double* mu, const double* var, const Targets& all, int n, int S, int K, long lo,
                 const UncOut& o) {
  const Targets t = all.from(lo);
  switch (lik.kind) {
    case 1: return ctx_fail(ctx, DCGP_ERR_ARG, "evaluate_uncertainty: class probabilities need a classification likelihood, this model is Gaussian");
    case 2: return bern_unc_tail(ctx, mu, var, t.values, n, S, K, lo, o);
    default: return unc_tail(ctx, mu, var, t.labels, n, S, K, lik.eps, lo, o);
  }
}

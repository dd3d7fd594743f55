// pointwise_dev.h -- the per-output likelihoods as log-density functors (device code): every head output an independent scalar with a
// float64 target y.  pointwise.hip's kernels are templated on one of these; uncertainty.hip shares the probit.
//
//   Gaussian(s2)                    logp(f, y) = -0.5 (log 2 pi + log s2) - 0.5 (y - f)^2 / s2                     (gpflow likelihoods.Gaussian)
//   Bernoulli(probit)               logp(f, y) = log p(f) if y == 1 else log(1 - p(f)),  p(f) = Phi(f) (1 - 2e-3) + 1e-3   (likelihoods.Bernoulli)
//   StudentT(scale s, deg_free nu)  logp(f, y) = c_nu - log s - (nu + 1) / 2 log1p(r^2 / nu),  r = (y - f) / s     (likelihoods.StudentT)
//   Poisson(exp link, binsize b)    logp(f, y) = y (f + log b) - b e^f - lgamma(y + 1)                             (likelihoods.Poisson)
//
// A functor says with its flags which members it has; a kernel asks for the others nowhere (if constexpr):
//   param()                          the one trainable parameter p (kHasParam: its gradient is reduced), read from its device word where set
//   base(y, p), tail(f, y, p)        logp = base + tail with base free of f (kHasBase; else logp = tail), under the 20-node rule
//   dtail, dparam                    d logp / d f and / d p at a node                                    (!kClosedVe; dparam: kHasParam)
//   ve, ve_grad                      kClosedVe: the variational expectation in closed form; weight * its (d / d m, d / d v) and the
//                                    unweighted d / d p term
//   predict                          kClosedPredict: (E_y, V_y) in closed form; else cm / cv, the conditional mean / variance of y given f
//   logdens                          kClosedLogdens: log of the predictive density of one sample (m, v) in closed form
//   score(mean, y)                   what the evaluation tail adds up per output from the sample-mean prediction: the squared error, or 1 / 0
// Each expression keeps the operations and the association of the kernel it came from: the results are those kernels' bits.
#pragma once

constexpr double kInvSqrt2 = 0.70710678118654752440, kInvSqrtPi = 0.56418958354775628695, kInvSqrt2Pi = 0.39894228040143267794;
constexpr double kLog2Pi = 1.83787706640934548356;

// gpflow's jittered probit (every log finite) and the Bernoulli log density at p
__device__ __forceinline__ double probit(double x) { return 0.5 * (1.0 + erf(x * kInvSqrt2)) * (1.0 - 2e-3) + 1e-3; }
__device__ __forceinline__ double bern_logp(double p, bool pos) { return pos ? log(p) : log(1.0 - p); }

__device__ __forceinline__ double squared_error(double mean, double y) { const double e = mean - y; return e * e; }

struct GaussianDensity {
  static constexpr bool kHasParam = true, kHasBase = false, kClosedVe = true, kClosedPredict = true, kClosedLogdens = true;
  const double* s2_dev; double s2_val;
  __device__ double param() const { return s2_dev ? *s2_dev : s2_val; }
  __device__ double ve(double m, double v, double y, double s2) const {
    const double inv = 1.0 / s2, c = -0.5 * (kLog2Pi + log(s2)), e = y - m;
    return c - 0.5 * (e * e + v) * inv;
  }
  __device__ void ve_grad(double m, double v, double y, double s2, double weight, double* gm, double* gv, double* dp) const {
    const double inv = 1.0 / s2, e = y - m;
    *gm = weight * e * inv;
    *gv = -0.5 * weight * inv;
    *dp = -0.5 * inv + 0.5 * (e * e + v) * inv * inv;
  }
  __device__ void predict(double m, double v, double s2, double* e, double* vy) const { *e = m; *vy = v + s2; }
  __device__ double logdens(double m, double v, double y, double s2) const {
    const double vv = v + s2, e = y - m;
    return -0.5 * (kLog2Pi + log(vv)) - 0.5 * e * e / vv;
  }
  __device__ double score(double mean, double y) const { return squared_error(mean, y); }
};

struct BernoulliDensity {
  static constexpr bool kHasParam = false, kHasBase = false, kClosedVe = false, kClosedPredict = true, kClosedLogdens = true;
  __device__ double param() const { return 0.0; }
  __device__ double tail(double f, double y, double) const { return bern_logp(probit(f), y == 1.0); }
  __device__ double dtail(double f, double y, double) const {
    const double p = probit(f), dp = exp(-0.5 * f * f) * kInvSqrt2Pi * (1.0 - 2e-3);
    return y == 1.0 ? dp / p : -dp / (1.0 - p);
  }
  __device__ void predict(double m, double v, double, double* e, double* vy) const {
    const double p = probit(m / sqrt(1.0 + v));
    *e = p; *vy = p - p * p;
  }
  __device__ double logdens(double m, double v, double y, double) const { return bern_logp(probit(m / sqrt(1.0 + v)), y == 1.0); }
  __device__ double score(double mean, double y) const { return (mean > 0.5) == (y == 1.0) ? 1.0 : 0.0; }   // a correct output
};

struct StudentTDensity {
  static constexpr bool kHasParam = true, kHasBase = true, kClosedVe = false, kClosedPredict = true, kClosedLogdens = false;
  const double* scale_dev; double scale_val, nu, c_nu;
  __device__ double param() const { return scale_dev ? *scale_dev : scale_val; }
  __device__ double base(double, double s) const { return c_nu - log(s); }
  __device__ double tail(double f, double y, double s) const { const double r = (y - f) / s; return -0.5 * (nu + 1.0) * log1p(r * r / nu); }
  __device__ double dtail(double f, double y, double s) const { const double r = (y - f) / s; return (nu + 1.0) * r / (s * (nu + r * r)); }
  __device__ double dparam(double f, double y, double s) const { const double r = (y - f) / s; return -1.0 / s + (nu + 1.0) * r * r / (s * (nu + r * r)); }
  // (the rule integrates f and f^2 exactly: v is its s^2 / 2 = max(v, 5e-11), what the sum gives under the clamp)
  __device__ void predict(double m, double v, double s, double* e, double* vy) const { *e = m; *vy = 0.5 * fmax(2.0 * v, 1e-10) + s * s * nu / (nu - 2.0); }
  __device__ double score(double mean, double y) const { return squared_error(mean, y); }
};

struct PoissonDensity {
  static constexpr bool kHasParam = false, kHasBase = true, kClosedVe = true, kClosedPredict = false, kClosedLogdens = false;
  double b, log_b;
  __device__ double param() const { return 0.0; }
  __device__ double base(double y, double) const { return y * log_b - lgamma(y + 1.0); }
  __device__ double tail(double f, double y, double) const { return y * f - b * exp(f); }
  __device__ double cm(double f, double) const { return b * exp(f); }
  __device__ double cv(double f, double) const { return b * exp(f); }
  __device__ double ve(double m, double v, double y, double) const { return y * m - b * exp(m + 0.5 * v) - lgamma(y + 1.0) + y * log_b; }
  __device__ void ve_grad(double m, double v, double y, double, double weight, double* gm, double* gv, double*) const {
    const double e = b * exp(m + 0.5 * v);
    *gm = weight * (y - e); *gv = weight * (-0.5 * e);
  }
  __device__ double score(double mean, double y) const { return squared_error(mean, y); }
};

/*
 * dcgp.h -- C-ABI of libdcgp.so: the MI355X (gfx950) conv-GP forward / ELBO hot path of DeepCGP.
 *
 * The reference (kekeblom/DeepCGP) has no FFI seam: the path is Python methods that build
 * TensorFlow graph nodes.  Every entry point below therefore names the reference *method* it
 * replaces (file:line under the reference tree); the Python classes in deepcgp_amd/ keep the
 * reference's names and call these through ctypes (see INTEGRATION.md for the binding).
 *
 * Conventions
 *   - every array is float64 ("double"), C-contiguous row-major, resident in DEVICE memory unless
 *     the parameter name ends in _host; labels are int32;
 *   - every function returns a status (DCGP_OK == 0); dcgp_last_error(ctx) gives the message;
 *   - one ctx <-> one device <-> one HIP stream; a ctx is not thread-safe; calls are stream-ordered
 *     and have completed (stream synchronised) on return unless stated otherwise;
 *   - the caller owns every buffer it allocates with dcgp_malloc; the library owns only internal
 *     workspaces hanging off the ctx / model;
 *   - "not positive definite" (the reference's tf.errors.InvalidArgumentError from tf.cholesky,
 *     conv_gp/experiment.py:45) is DCGP_ERR_NOT_PD with the 1-based failing column in *info.
 */
#ifndef DCGP_H
#define DCGP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCGP_OK 0
#define DCGP_ERR_ARG (-1)      /* bad argument (NULL, non-positive size, unsupported shape)      */
#define DCGP_ERR_HIP (-2)      /* a HIP runtime call failed                                       */
#define DCGP_ERR_NOT_PD (-3)   /* Cholesky hit a non-positive pivot                               */
#define DCGP_ERR_RCCL (-4)     /* an RCCL call failed / communicator missing                      */
#define DCGP_ERR_ALLOC (-5)    /* device allocation failed                                        */

typedef struct dcgp_ctx dcgp_ctx;
typedef struct dcgp_model dcgp_model;

/* ---- context, memory, errors ------------------------------------------------------------- */
int dcgp_ctx_create(int device, dcgp_ctx** out);
int dcgp_ctx_destroy(dcgp_ctx* ctx);
const char* dcgp_last_error(dcgp_ctx* ctx);
int dcgp_device_count(int* count);
int dcgp_malloc(dcgp_ctx* ctx, size_t bytes, void** dptr);
int dcgp_free(dcgp_ctx* ctx, void* dptr);
int dcgp_h2d(dcgp_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int dcgp_d2h(dcgp_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int dcgp_memset(dcgp_ctx* ctx, void* dptr, int value, size_t bytes);
int dcgp_sync(dcgp_ctx* ctx);
/* Device memory the library itself holds for this ctx (the named, grow-only workspaces: factor scratch, K_uf / A1 slabs of the
 * sweep + GEMM route, partial sums) and the number of such workspaces.  SURVEY.md 8(b) planned a dcgp_workspace_query that SIZES
 * caller-provided workspaces; the library grows its own lazily instead (nothing on the reference side owns scratch memory either:
 * TensorFlow allocates graph temporaries itself), so the query reports what has been taken so far.                               */
int dcgp_workspace_query(dcgp_ctx* ctx, size_t* bytes_out, int* count_out);
/* Debugging aids of the library's device allocator (csrc/ctx.hip, csrc/dev_guard.h), both process-wide and read once.  DCGP_POISON_WS: every
 * fresh device allocation of the library (workspaces, layer and model buffers, dcgp_malloc) is filled with 0xFF bytes (NaNs).  DCGP_GUARD_WS=<bytes>
 * (not a number: 4096; rounded up to a multiple of 256): every allocation is followed by that many guard bytes of 0xFF, starting at the REQUESTED
 * size, and checked when it is freed.  tests/test_gpu_memcheck.py runs every feature family under both.
 * dcgp_debug_guard_bytes: *out = the guard size in bytes, 0 when the mode is off. */
int dcgp_debug_guard_bytes(dcgp_ctx* ctx, long* out);
/* Synchronises the device and reads back the guard of every live allocation; *n_bad_out = guards with a byte that is no longer 0xFF, plus the
 * broken guards that frees have found since the last call.  report (may be NULL; report_len bytes, always terminated): label, requested bytes
 * and offset of the first bad byte past the requested end, for the first eight of them.  A violation is reported once: a live allocation's
 * guard is made whole again and the remembered ones are cleared.  Mode off: *n_bad_out = 0. */
int dcgp_debug_check_guards(dcgp_ctx* ctx, long* n_bad_out, char* report, int report_len);
/* Copies one zero byte to dptr + requested bytes + offset_past_end, i.e. into the guard of an allocation of this ctx: the way to show that the
 * checker sees a byte.  DCGP_ERR_ARG unless guard mode is on, dptr is a registered allocation and 0 <= offset_past_end < the guard size. */
int dcgp_debug_touch_guard(dcgp_ctx* ctx, void* dptr, long offset_past_end);
/* A/B and debugging switches (csrc/common.h: DcgpOptions).  A ctx reads the environment variable DCGP_<NAME> once, in
 * dcgp_ctx_create, as the switch's initial value; afterwards only these calls change it -- no getenv on the step path.  Names are
 * lower case ("no_fused_layer", "kl_side", ...); an unknown name is DCGP_ERR_ARG.  dcgp_ctx_get_option also answers "n_cus": the
 * compute units of the ctx's device, which is no switch and cannot be set.                                                          */
int dcgp_ctx_set_option(dcgp_ctx* ctx, const char* name, long value);
int dcgp_ctx_get_option(dcgp_ctx* ctx, const char* name, long* value_out);

/* ---- per-kernel HIP-event timing (bench.py's roofline leg) -------------------------------- */
/* When enabled, the launches of the named kernel families ("kuf", "gemm_cond", "potrf", "trtri",
 * "head_kzx", "head_kdiag", ...) are bracketed by hipEvents on the ctx stream.                 */
int dcgp_timing_enable(dcgp_ctx* ctx, int on);   /* 0 off, 1 every family, 2 only the roofline kernels ("conv_fused", "gemm_cond_s3", "kuf"), every 7th launch of them */
int dcgp_timing_reset(dcgp_ctx* ctx);
int dcgp_timing_query(dcgp_ctx* ctx, const char* name, int* launches, double* total_ms);
int dcgp_timing_names(dcgp_ctx* ctx, char* buf, size_t buflen);   /* ';'-separated list */

/* ---- patch view: FullView.extract_patches / extract_patches_PNL (conv_gp/views.py:32-54) --- */
/* X [N,H,W,C] -> out [N,P,L] (pnl == 0) or [P,N,L] (pnl != 0); VALID window, dilation 1 (a dilated view splits the images into phase sub-images around this call);
 * p = oh*W' + ow, l = (kh*f + kw)*C + c.                                                         */
int dcgp_extract_patches(dcgp_ctx* ctx, const double* X, int N, int H, int W, int C, int f, int stride,
                         double* out, int pnl);

/* ---- inducing-patch kernel matrices ------------------------------------------------------- */
/* MultiOutputConvKernel.Kuu (conv_gp/layers.py:18-21) == RBF.K(Z) + jitter*I; also the dispatch
 * Kuu(feature, kern, jitter) of conv_gp/kernels.py:172-174.  Z [M,L] -> out [M,M].               */
int dcgp_kuu_rbf(dcgp_ctx* ctx, const double* Z, int M, int L, double variance, double lengthscale,
                 double jitter, double* out_MM);
/* FullView.extract_patches_PNL + MultiOutputConvKernel.Kuf (conv_gp/views.py:40-44,
 * conv_gp/layers.py:23-32) fused: the patches are gathered from an LDS-staged image and never
 * materialised.  X [N,H,W,C], Z [M,L] -> out.  layout 0: [P,M,N] (the reference's Kuf layout);
 * layout 1: [M, N*P] with column n*P + p (the layout the fused conditional consumes).            */
int dcgp_kuf_patches_rbf(dcgp_ctx* ctx, const double* X, int N, int H, int W, int C, int f, int stride,
                         const double* Z, int M, double variance, double lengthscale,
                         double* out, int layout);
/* MultiOutputConvKernel.Kuf (conv_gp/layers.py:23-32) with gpflow.kernels.RBF(f*f*C, ARD=True) as the base kernel:
 * k(x, z) = variance * exp(-1/2 sum_l (x_l - z_l)^2 / lengthscales[l]^2), one lengthscale per patch element
 * l = (kh*f + kw)*C + c.  The arguments of dcgp_kuf_patches_rbf with a DEVICE array of L = f*f*C lengthscales (all > 0)
 * in place of the scalar; same layouts.  The patch is divided by the lengthscales where it is gathered (a pixel sits at
 * different l in overlapping patches), Z while its transpose is formed.  K_uu of such a kernel: dcgp_kuu_rbf on the
 * rows Z / lengthscales with lengthscale 1.                                                                          */
int dcgp_kuf_patches_rbf_ard(dcgp_ctx* ctx, const double* X, int N, int H, int W, int C, int f, int stride,
                             const double* Z, int M, double variance, const double* lengthscales,
                             double* out, int layout);
/* The same two matrices for the ArcCosine(order = 0) base kernel that `--base-kernel acos` selects for the conv
 * layers (conv_gp/models.py:118-119; gpflow.kernels.ArcCosine: k = variance * (pi - theta) / pi,
 * theta = acos(1e-15 + (1 - 2e-15) cos), cos from <x,z> = weight_variance * x.z + bias_variance; Kdiag = variance). */
int dcgp_kuu_acos(dcgp_ctx* ctx, const double* Z, int M, int L, double variance, double weight_variance,
                  double bias_variance, double jitter, double* out_MM);
int dcgp_kuf_patches_acos(dcgp_ctx* ctx, const double* X, int N, int H, int W, int C, int f, int stride,
                          const double* Z, int M, double variance, double weight_variance,
                          double bias_variance, double* out, int layout);
/* The same two matrices for gpflow.kernels.Matern32 (nu2 = 3) and gpflow.kernels.Matern52 (nu2 = 5), ARD = False:
 * k = variance (1 + a) exp(-a), a = sqrt(3) r, and k = variance (1 + a + a^2 / 3) exp(-a), a = sqrt(5) r, with
 * r = sqrt(max(|x - z|^2, 0) / lengthscale^2 + 1e-12) (gpflow's scaled_euclid_dist); Kdiag = variance.  The conv layers'
 * base kernel under --base-kernel matern32 | matern52.                                                        */
int dcgp_kuu_matern(dcgp_ctx* ctx, const double* Z, int M, int L, int nu2, double variance, double lengthscale,
                    double jitter, double* out_MM);
int dcgp_kuf_patches_matern(dcgp_ctx* ctx, const double* X, int N, int H, int W, int C, int f, int stride,
                            const double* Z, int M, int nu2, double variance, double lengthscale,
                            double* out, int layout);

/* ---- dense M x M factorisations ------------------------------------------------------------ */
/* tf.cholesky (conv_gp/conditionals.py:29, layers.py:151,156): in place, lower factor, strict
 * upper triangle zeroed.  *info_host = 0, or the 1-based column of the first non-positive pivot
 * (return value DCGP_ERR_NOT_PD).                                                                */
int dcgp_potrf_lower(dcgp_ctx* ctx, double* A_MM, int M, int* info_host);
/* inverse of a lower-triangular factor (the form in which the triangular solves of
 * conv_gp/conditionals.py:31-33,44-47 are applied on the matrix cores).                          */
int dcgp_trtri_lower(dcgp_ctx* ctx, const double* L_MM, int M, double* Linv_MM);

/* ---- the conditional ---------------------------------------------------------------------- */
/* conditional(Kmn, Kmm, Knn, f, full_cov=False, q_sqrt, white) of conv_gp/conditionals.py:6-67.
 * Kmn [P,M,N], Kmm [M,M] (not overwritten), Knn [P,N], f [M,R], q_sqrt [R,M,M] lower-triangular
 * (its strict upper triangle is ignored, matrix_band_part at :55) or NULL.
 * out_mean [N,P,R], out_var [R,P,N].                                                            */
int dcgp_conditional(dcgp_ctx* ctx, const double* Kmn, const double* Kmm, const double* Knn,
                     const double* f, const double* q_sqrt, int white, int P, int M, int N, int R,
                     double* out_mean, double* out_var, int* info_host);

/* ConvLayer.conditional_ND (conv_gp/layers.py:96-135) for the Zero mean function, fused end to
 * end (patch gather -> Kuf -> Cholesky -> conditional), plus Layer.sample_from_conditional's
 * reparameterisation when z != NULL.  X [N, H*W*C]; out_* [N, P*R] (column p*R + r); any of the
 * three outputs may be NULL.  z [N, P*R].  identity_mean != 0 adds Conv2dMean
 * (conv_gp/mean_functions.py:28-41; odd filter sizes only).                                      */
int dcgp_conv_layer_forward(dcgp_ctx* ctx, const double* X, int N, int H, int W, int C, int f, int stride,
                            const double* Z, int M, int R, double variance, double lengthscale,
                            const double* q_mu, const double* q_sqrt, int white, int identity_mean,
                            const double* z, double jitter,
                            double* out_sample, double* out_mean, double* out_var, int* info_host);

/* ---- classification-head kernels ----------------------------------------------------------- */
/* ConvKernel.Kzx (conv_gp/kernels.py:117-133) / AdditivePatchKernel.Kzx (:63-74; identical
 * arithmetic): out[m,n] = (1/P) sum_p w[p] k(Z[m], x[n,p]).  X [N,H,W,C], Z [M,L], w [P] -> [M,N] */
int dcgp_convkernel_kzx(dcgp_ctx* ctx, const double* X, int N, int H, int W, int C, int f, int stride,
                        const double* Z, int M, double variance, double lengthscale, const double* w,
                        double* out_MN);
/* ConvKernel.Kdiag (conv_gp/kernels.py:106-115): out[n] = (1/P^2) sum_{p,p'} w[p] w[p'] k(x[n,p], x[n,p']). */
int dcgp_convkernel_kdiag(dcgp_ctx* ctx, const double* X, int N, int H, int W, int C, int f, int stride,
                          double variance, double lengthscale, const double* w, double* out_N);
/* The head's mean split over the patches, out[n,p,r] = (w[p]/P) sum_m k(Z[m], x[n,p]) beta[m,r], so that sum_p out[n,p,:] =
 * (Kzx^T beta)[n,:]: one launch that never stores K_uf.  Replaces dcgp_kuf_patches_rbf into a [P,M,N] buffer followed by
 * dcgp_gemm_strided -- the per-patch maps the reference reads off its patch-weight and inducing-patch plots
 * (conv_gp/utils/tensorboard.py:164-195, Inspect.ipynb).  X [N,H,W,C], Z [M,L], w [P], beta [M,R] -> out [N,P,R] (device).
 * N == 0: DCGP_OK, nothing written. */
int dcgp_convkernel_patch_mean(dcgp_ctx* ctx, const double* X, int N, int H, int W, int C, int f, int stride,
                               const double* Z, int M, double variance, double lengthscale, const double* w,
                               const double* beta, int R, double* out_NPR);
/* AdditivePatchKernel.Kdiag (conv_gp/kernels.py:53-61): out[n] = variance * mean_p w[p].        */
int dcgp_additive_kdiag(dcgp_ctx* ctx, int N, int P, double variance, const double* w, double* out_N);

/* doubly_stochastic_dgp SVGP_Layer.conditional_ND (call site conv_gp/models.py:192-198) given
 * Kuf [M,N], Ku [M,M] (jitter already added), Kdiag [N]; out_mean, out_var [N,R].               */
int dcgp_svgp_conditional(dcgp_ctx* ctx, const double* Kuf, const double* Ku, const double* Kdiag,
                          const double* q_mu, const double* q_sqrt, int white, int M, int N, int R,
                          double* out_mean, double* out_var, int* info_host);

/* ---- full covariances of the head (prediction only) ----------------------------------------- */
/* ConvKernel.K (conv_gp/kernels.py:81-104), additive == 0:
 *     out[b,n,n'] = (1/P^2) sum_{p,p'} w[p] w[p'] k(x[b,n,p], x2[b,n',p'])
 * AdditivePatchKernel.K (conv_gp/kernels.py:34-51), additive != 0:
 *     out[b,n,n'] = (1/P) sum_p w[p] k(x[b,n,p], x2[b,n',p])
 * RBF base kernel.  X [B,N,H,W,C], X2 [B,N2,H,W,C] or NULL (X2 = X, N2 = N: only n <= n' is computed and mirrored, so each
 * out[b] is symmetric bit for bit), w [P] -> out [B,N,N2].  Deterministic: no floating-point atomics.                      */
int dcgp_convkernel_k(dcgp_ctx* ctx, const double* X, const double* X2, int B, int N, int N2, int H, int W, int C, int f,
                      int stride, double variance, double lengthscale, const double* w, int additive, double* out);
/* doubly_stochastic_dgp SVGP_Layer.conditional_ND(X, full_cov=True) for B input sets against one q(u):
 * Kuf [B,M,N], Ku [M,M] (jitter already added), Kff [B,N,N], q_mu [M,R], q_sqrt [R,M,M] (lower triangle used) or NULL.
 * out_mean [B,N,R]; out_var [B,N,N,R] = Kff - A1^T A1 + (Lq_r^T A)^T (Lq_r^T A), A1 = inv(Lu) Kuf, A = A1 (white) or
 * inv(Lu)^T A1.  A Ku that is not positive definite: DCGP_ERR_NOT_PD with the 1-based column in *info_host.                */
int dcgp_svgp_conditional_full_cov(dcgp_ctx* ctx, const double* Kuf, const double* Ku, const double* Kff, const double* q_mu,
                                   const double* q_sqrt, int white, int B, int M, int N, int R, double* out_mean,
                                   double* out_var, int* info_host);
/* doubly_stochastic_dgp.utils.reparameterize(mean, var, z, full_cov=True) (the full_cov branch of DGP_Base.propagate):
 * out[s,:,d] = mean[s,:,d] + chol(var[s,:,:,d] + jitter I) z[s,:,d] for all S x D matrices in one launch.
 * mean, z, out [S,N,D]; var [S,N,N,D] (lower triangle used).  N <= 128 (DCGP_ERR_ARG beyond).  A matrix that is not
 * positive definite: DCGP_ERR_NOT_PD, *info_host = its 1-based failing column.                                          */
int dcgp_reparam_full_cov(dcgp_ctx* ctx, const double* mean, const double* var, const double* z, int S, int N, int D,
                          double jitter, double* out, int* info_host);

/* ---- KL, likelihood, sampling --------------------------------------------------------------- */
/* gpflow.kullback_leiblers.gauss_kl(q_mu, q_sqrt, K) (call sites conv_gp/layers.py:145,147);
 * K == NULL is the whitened prior.  q_mu [M,R], q_sqrt [R,M,M], K [M,M].                         */
int dcgp_gauss_kl(dcgp_ctx* ctx, const double* q_mu, const double* q_sqrt, const double* K, int M, int R,
                  double* out_host, int* info_host);
/* gpflow MultiClass(K) + RobustMax(eps).variational_expectations, 20 Gauss-Hermite points (call
 * site conv_gp/models.py:67).  mu, var [n,K]; y [n] int32 -> out [n].                            */
int dcgp_robustmax_varexp(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n,
                          int K, double eps, double* out_n);
/* MultiClass.predict_mean_and_var: per-class probabilities [n,K].                                */
int dcgp_robustmax_predict(dcgp_ctx* ctx, const double* mu, const double* var, int n, int K, double eps,
                           double* out_p);
/* gpflow likelihoods.SoftMax(K) variational_expectations / predict_mean_and_var (MonteCarloLikelihood) with the per-call draw replaced by
 * a fixed table of nodes [Q, K] (standard-normal draws, the same for every row; device): with s = sqrt(max(var, 1e-10)), f_q = mu + s * e_q,
 * out_n [n] = 1/Q sum_q (f_q[y] - logsumexp_k f_q[k]) and out_p [n, K] = 1/Q sum_q softmax(f_q), summed in a fixed order (two calls give the
 * same bits).  mu, var [n, K]; y [n] int32.  DCGP_ERR_ARG unless 2 <= K, 1 <= Q, Q * K <= 4096 (the table's 32 KB of LDS) and every
 * label is in [0, K).                                                                            */
int dcgp_softmax_varexp(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n,
                        int K, const double* nodes, int Q, double* out_n);
int dcgp_softmax_predict(dcgp_ctx* ctx, const double* mu, const double* var, int n, int K,
                         const double* nodes, int Q, double* out_p);
/* gpflow likelihoods.StudentT(scale, deg_free) (kind 4, params_host = {scale > 1e-6, deg_free > 2}) and likelihoods.Poisson(invlink=exp,
 * binsize) (kind 5, params_host = {binsize > 0}) on arrays mu, var, y, out [n, K] (device; y float64), per element with the 20 Gauss-Hermite
 * nodes x_i, c_i = w_i / sqrt(pi), f_i = mu + sqrt(max(2 var, 1e-10)) x_i:
 *   dcgp_quad_varexp      Likelihood.variational_expectations: sum_i c_i logp(f_i, y); Poisson: gpflow's closed form
 *                         y mu - b exp(mu + var / 2) - lgamma(y + 1) + y log b,
 *   dcgp_quad_predict     Likelihood.predict_mean_and_var: E_y = sum_i c_i cm(f_i), V_y = sum_i c_i (cv(f_i) + cm(f_i)^2) - E_y^2 (StudentT: the
 *                         closed forms mu and var + scale^2 nu / (nu - 2); Poisson: cm = cv = b e^f); either output may be NULL,
 *   dcgp_quad_logdensity  Likelihood.predict_density: logsumexp_i (logp(f_i, y) + log c_i),
 * with logp = c_nu - log scale - (nu + 1) / 2 log1p(((y - f) / scale)^2 / nu) or y (f + log b) - b e^f - lgamma(y + 1).  Another kind, a
 * bad parameter or n, K <= 0: DCGP_ERR_ARG.                                                       */
int dcgp_quad_varexp(dcgp_ctx* ctx, int kind, const double* params_host, const double* mu, const double* var, const double* y,
                     int n, int K, double* out);
int dcgp_quad_predict(dcgp_ctx* ctx, int kind, const double* params_host, const double* mu, const double* var, int n, int K,
                      double* out_mean, double* out_var);
int dcgp_quad_logdensity(dcgp_ctx* ctx, int kind, const double* params_host, const double* mu, const double* var, const double* y,
                         int n, int K, double* out);
/* The reverse tail of dcgp_quad_varexp on the same arrays (what TensorFlow autodiff of Likelihood.variational_expectations gives):
 * out_gm, out_gv [n, K] = weight * d varexp / d(mu, var) per element (d / d var = 0 where 2 var <= 1e-10) and, kind 4, out_gparam [1] (device) =
 * weight * the sum over the elements of d varexp / d scale, summed in a fixed order; kind 5 leaves out_gparam alone (it may be NULL). */
int dcgp_quad_grad_seeds(dcgp_ctx* ctx, int kind, const double* params_host, const double* mu, const double* var, const double* y,
                         int n, int K, double weight, double* out_gm, double* out_gv, double* out_gparam);
/* doubly_stochastic_dgp.utils.reparameterize: out = mean + z*sqrt(var + jitter), n elements.     */
int dcgp_reparam(dcgp_ctx* ctx, const double* mean, const double* var, const double* z, size_t n,
                 double jitter, double* out);

/* ---- model-level path: DGP_Base.propagate / _build_likelihood (doubly_stochastic_dgp, call sites
 *      conv_gp/models.py:65-70, conv_gp/utils/tensorboard.py:32) ------------------------------- */
int dcgp_model_create(dcgp_ctx* ctx, int num_samples, double jitter, dcgp_model** out);
int dcgp_model_destroy(dcgp_model* model);
/* ConvLayer (conv_gp/layers.py:52-94).  Parameter arrays are HOST pointers, copied to the device.
 * Z0 is the frozen initial Z of the KL prior (conv_gp/layers.py:149-152); NULL -> Z.             */
int dcgp_model_add_conv_layer(dcgp_model* model, int H, int W, int C, int f, int stride, int M, int R,
                              int white, int identity_mean, double variance, double lengthscale,
                              const double* Z_host, const double* Z0_host,
                              const double* q_mu_host, const double* q_sqrt_host);
/* SVGP_Layer(kern=ConvKernel|AdditivePatchKernel) (conv_gp/models.py:169-198).
 * kernel_type 0 = ConvKernel, 1 = AdditivePatchKernel.                                           */
int dcgp_model_set_head(dcgp_model* model, int H, int W, int C, int f, int stride, int M, int R,
                        int white, int kernel_type, double variance, double lengthscale,
                        const double* Z_host, const double* w_host,
                        const double* q_mu_host, const double* q_sqrt_host);
/* Symmetric zero padding of `pad` >= 0 pixels on all four sides of layer `layer`'s input image, across all channels: the output is
 * ((H + 2 pad - f) / stride + 1) x ((W + 2 pad - f) / stride + 1).  The layer (a conv layer or a patch head) is added with the PADDED
 * H, W; this call records that its input is its predecessor's output (X for layer 0, which stays [N][H W C] in the unpadded geometry
 * in every call: forward, gradient, input gradient, evaluation, dataset) with the border added on the device.  The first forward
 * checks, before anything is launched, that predecessor output + 2 pad is the layer's H, W, that the channels agree, and refuses a
 * dense head (per-dimension lengthscales); this call itself refuses a layer that does not exist, pad < 0 and a border that leaves
 * no image inside the layer's H x W.  pad = 0 (the default) is the unpadded layer, on exactly the unpadded code path.
 * Padding is no parameter: checkpoints do not hold it.                                                                        */
int dcgp_model_set_input_padding(dcgp_model* model, int layer, int pad);
/* Dilation (atrous rate) d >= 1 of conv layer `layer`: the window's taps sit d pixels apart, so its f x f filter spans d (f - 1) + 1
 * pixels of the (padded) input Hp x Wp and the output is (Hp - d (f - 1)) x (Wp - d (f - 1)), with the same patch length, Z and M.
 * Generalises the reference's FullView.dilation = 1, passed as `rates` to tf.extract_image_patches (conv_gp/views.py:24,37).
 * The layer-adding contract: a dilated layer is added like any other, with its true (padded) input size Hp x Wp and stride 1, and the
 * layer above with the true output size; this call keeps Hp x Wp in the model and switches the layer's own geometry to the PHASE
 * geometry ceil(Hp / d) x ceil(Wp / d): the layer runs as an ordinary VALID layer on the d^2 phase sub-images of its input
 * (space-to-batch on the device, csrc/dilate.hip) and its outputs are put back into image layout behind it.  X, dX, datasets, explicit
 * noise and dcgp_model_layer_output stay in the caller's image geometry in every call.  The patch count is part of the layout of the
 * layer's gradient block, so the dilation is set before the model's first gradient step.  This call refuses a layer that does not
 * exist, d < 1, the head, a layer whose stride is not 1, a window whose span d (f - 1) + 1 exceeds the padded input, a layer that has
 * taken a gradient step, a sharded model (dcgp_model_set_shard refuses a dilated model in turn) and enqueued steps still to be
 * collected.  EVERY forward of a model with a dilated layer checks, before anything is launched, that the layers below and above take
 * and give the dilated layer's true sizes and channels (nothing is remembered between calls: changing a neighbour's padding later is
 * caught).  d = 1 (the default) is the undilated layer on exactly the undilated code path.  Dilation is no parameter: checkpoints
 * do not hold it.
 * Not provided: dilation with stride > 1, a dilated head, per-axis dilation, full covariances through a dilated layer, multi-rank.  */
int dcgp_model_set_dilation(dcgp_model* model, int layer, int d);
/* A linear convolutional mean function on conv layer `layer` (conv_gp/mean_functions.py:6-41 with any filter; added to the conditional's
 * mean at conv_gp/layers.py:133-134): m(x)[n, p, r] = sum_l patch_p(x_n)[l] W[l][r] on the layer's own window -- its f, stride and, through
 * the padded copy the layer reads, its padding.  filter_host [f*f*C][R] in FullView's (kh, kw, c) element order: the reference's
 * conv_filter [f, f, C, R] flattened.  Every entry point that goes through the model evaluates it (one launch behind the layer's own,
 * added to mean and sample; such a layer carries no head rows), differentiates it (dX for the layers below and dcgp_model_input_grad) and,
 * with trainable != 0, forms its gradient (L R slots at the very end of the layer's gradient block, zero while frozen) and moves it in the
 * optimiser steps.  Allowed before the layer's first gradient step; calling it again replaces values and flag.  DCGP_ERR_ARG on the
 * head, on a layer added with identity_mean (the in-launch Conv2dMean), once the layer's gradient block exists, or while enqueued steps
 * are still to be collected.  The filter is "mean_filter" in dcgp_model_set_param / _get_param / _get_grad / _set_trainable
 * (conv_gp/mean_functions.py:6-41, conv_gp/layers.py:133-134).  It is no input of the factorisation chain: writing it starts no new
 * parameter version, so dcgp_model_set_factor_reuse keeps its chain.  No atomics: two runs give the same bits. */
int dcgp_model_set_mean_filter(dcgp_model* model, int layer, const double* filter_host /* [f*f*C][R] */, int trainable);
/* A mixed conv layer (csrc/mix.hip; gpflow's SharedMixed... / LinearCoregionalization on the patches): the layer's G = gp_count latent GPs leave it as R
 * feature maps, sample[j, r] = sum_g u[j, g] W[g, r] of the latent sample u (sample, then mix: P * G noise values a row, the counters of an unmixed
 * layer of gp_count G), mean[j, r] = sum_g gm[j, g] W[g, r], var[j, r] = sum_g gv[j, g] W[g, r]^2; a mean filter then has R columns and adds into the
 * maps.  The KL term is the G latent GPs'.  W_host [G][R], unconstrained, trainable until dcgp_model_set_trainable(.., "mixing", 0); NULL switches the
 * mixing off again.  W is "mixing" in dcgp_model_set_param / _get_param / _get_grad / _set_trainable and the moment accessors; its gradient sits at
 * the very end of the layer's gradient block.  Starts a new parameter version.  DCGP_ERR_ARG, naming the number: G other than the layer's gp_count, R
 * outside 1 .. 64 or other than the channels C the next layer takes, the head, a layer added with identity_mean (give it the centre-pixel filter
 * through dcgp_model_set_mean_filter), a layer that has its mean filter already or has taken a gradient step, enqueued steps still to be collected.
 * A mixed layer cannot carry the head's rows in its launch, and it is not the model's last layer.  No atomics: two runs give the same bits. */
int dcgp_model_set_mixing(dcgp_model* model, int layer, const double* W_host /* [G][R] or NULL */, int G, int R);
/* The mixing's kernels as operators (device pointers, synchronous).  Forward: columns col0 .. col0 + Kc - 1, replica s < rep of column j at
 * s * lat_stride + j * G of u / gm / gv and at s * out_stride + j * R of sample / mean / var (each output and its input may be NULL). */
int dcgp_mix_forward(dcgp_ctx* ctx, const double* W_dev, int G, int R, const double* u_dev, const double* gm_dev, const double* gv_dev, long col0, long Kc,
                     int rep, long lat_stride, long out_stride, double* sample_dev, double* mean_dev, double* var_dev);
/* Backward on Kc columns: gu [Kc][G] = gF W^T and gW [G][R] = u^T gF (either may be NULL); gW's partial sums have a fixed order. */
int dcgp_mix_backward(dcgp_ctx* ctx, const double* W_dev, int G, int R, const double* u_dev, const double* gF_dev, long Kc, double* gu_dev, double* gW_dev);
/* keep every layer's (sample, mean, var) of the next forward passes for dcgp_model_layer_output   */
int dcgp_model_set_keep_outputs(dcgp_model* model, int on);
/* Push a changed parameter: which = "Z", "Z0", "q_mu", "q_sqrt", "w", "variance", "lengthscale", or
 * "base_kernel" = {type, variance, p1, p2}: type 0 RBF (p1 = lengthscale), type 1 ArcCosine order 0 (p1 = weight
 * variance, p2 = bias variance; conv layers only, conv_gp/models.py:113-121), type 2 Matern32 and type 3 Matern52
 * (p1 = lengthscale; conv layers only), or "ard_lengthscales" = one lengthscale
 * per input dimension for a single-patch head (H = W = f = 1, C = D): gpflow RBF(D, ARD=True) on the flattened
 * features, the dense head of --last-kernel rbf (conv_gp/models.py:160-168).  "likelihood_epsilon" (one value in
 * (0, 1), `layer` ignored) is the RobustMax epsilon of the ELBO / predict_y entry points (default 1e-3).
 * "mean_filter" [f*f*C, R]: the filter of a conv layer given one by dcgp_model_set_mean_filter (conv_gp/mean_functions.py:6-41,
 * conv_gp/layers.py:133-134); it alone starts no new parameter version.  */
int dcgp_model_set_param(dcgp_model* model, int layer, const char* which, const double* value_host,
                         size_t count);

/* One forward ELBO evaluation of a minibatch (compute_log_likelihood semantics):
 *   X [N, H*W*C], y [N] int32 (device).  z_per_layer_host: array of num_layers DEVICE pointers,
 *   each [S, N, D_l] standard-normal noise (entries may be NULL -> counter-based device RNG with
 *   `seed`); NULL -> RNG for all layers.  scale = num_data / global_batch.  dedup_layer0 != 0
 *   evaluates the first layer on the N distinct images only (propagate() tiles X S times, so the
 *   S copies are identical; results are bit-identical either way).
 *   If the ctx holds a communicator (dcgp_comm_init_rank) the data term is all-reduced (sum) over
 *   the ranks before scaling.  out_host[0] = ELBO, [1] = sum_n E_q log p(y_n) (global), [2] = sum KL. */
int dcgp_elbo_forward(dcgp_model* model, const double* X, const int32_t* y, int N, double scale,
                      const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0,
                      double* out_host, int* info_host);
/* Throughput mode of dcgp_elbo_forward for loops that do not need step i's value before step i + 1 is queued (an
 * optimisation loop: session.run(train_op) at conv_gp/experiment.py:84-108 returns nothing; the logger reads the
 * objective every test_every steps only).  _enqueue queues the same launches and returns a ticket without waiting;
 * _collect waits for that step and hands back what dcgp_elbo_forward would have (same values, same error codes).
 * Tickets are collected in the order they were handed out, at most 4 may be outstanding; X, y and the noise buffers of
 * an enqueued step must stay untouched until it is collected.  The host then runs ahead of the device, which hides
 * the launch latency at the head of a step and the wake-up after it. */
int dcgp_elbo_forward_enqueue(dcgp_model* model, const double* X, const int32_t* y, int N, double scale,
                              const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0,
                              uint64_t* ticket);
int dcgp_elbo_forward_collect(dcgp_model* model, uint64_t ticket, double* out_host, int* info_host);
/* The ELBO of dcgp_elbo_forward AND its gradient with respect to every trainable value (what TensorFlow autodiff
 * hands the optimiser at conv_gp/experiment.py:84-108): Z, q_mu, q_sqrt (lower triangle), the base-kernel
 * hyper-parameters of every layer (variance + lengthscale, ArcCosine: variance + weight / bias variances, dense head:
 * variance + one lengthscale per input dimension), patch_weights of the head -- constrained values, not gpflow's
 * unconstrained ones.  dedup_layer0 as in dcgp_elbo_forward: the first layer's conditional and its reverse pass run on
 * the N distinct images (the S gradients per image are added first) -- same values.
 * The gradients stay on the device; read them with dcgp_model_get_grad. */
int dcgp_elbo_grad(dcgp_model* model, const double* X, const int32_t* y, int N, double scale,
                   const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0, double* out_host,
                   int* info_host);
/* which = "Z" [M, L], "q_mu" [M, R], "q_sqrt" [R, M, M], "variance" [1], "lengthscale" [1] (RBF) or "weight_variances" [1] and
 * "bias_variance" [1] (ArcCosine conv layers), "w" [P] (head),
 * "ard_lengthscales" [D] (dense RBF(ARD) head; its scalar "lengthscale" gradient is 0),
 * "mean_filter" [f*f*C, R] (a conv layer with a filter mean, conv_gp/mean_functions.py:6-41, conv_gp/layers.py:133-134; zero while the filter is frozen). */
int dcgp_model_get_grad(dcgp_model* model, int layer, const char* which, double* out_host, size_t count);
/* Data parallelism of the gradient: every rank holds a shard of the batch and the full parameters.  The data part of
 * the gradient is a sum over shards, the KL part is replicated, so each rank computes scale * data_grad(shard) -
 * KL_grad / shards and the sum over ranks is the full gradient.  With a communicator on the ctx
 * (dcgp_comm_init_rank) dcgp_elbo_grad does that sum itself: one in-stream ncclAllReduce per layer over the layer's
 * contiguous gradient block.  Without one (host-side reduction, tests) set the shard count explicitly and reduce
 * the blocks yourself: block = [Z | q_mu | q_sqrt | w | variance, p1, p2 | ARD lengthscales (head)], device pointer
 * (p1 = lengthscale or ArcCosine weight variance, p2 = ArcCosine bias variance).  shards = 0
 * restores the default (ranks of the communicator, else 1). */
int dcgp_model_set_grad_shards(dcgp_model* model, int shards);
/* Multi-GPU: this rank holds images [first_image, first_image + N) of a minibatch of global_batch images.  With it
 * declared the device RNG of Layer.sample_from_conditional draws every element at its counter in the UN-sharded batch, so the ELBO
 * of a step does not depend on the number of ranks (global_batch = 0: not sharded, one RNG stream per rank). */
int dcgp_model_set_shard(dcgp_model* model, int first_image, int global_batch);
int dcgp_model_grad_block(dcgp_model* model, int layer, double** block_dev, size_t* count);
/* One optimiser step on the gradients dcgp_elbo_grad left on the device: tf.train.AdamOptimizer semantics
 * (lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t); theta -= lr_t m / (sqrt(v) + eps); t = 1, 2, ...) ascending the
 * ELBO in gpflow's unconstrained space -- variance / lengthscale through transforms.positive (softplus + 1e-6),
 * q_sqrt on its lower triangle, Z / q_mu / patch_weights as they are (gpflow.train.AdamOptimizer at
 * conv_gp/experiment.py:104-107; the learning-rate schedule :71-73 stays with the caller).  t = 0: use the model's
 * own count of steps taken since its (zero-initialised) moment buffers were created -- a freshly built optimiser
 * restarts its beta powers whatever global_step a loaded checkpoint carries (experiment.py:84-89). */
int dcgp_model_adam_step(dcgp_model* model, double lr, double beta1, double beta2, double eps, int t);
/* One training step in one call -- dcgp_elbo_grad and dcgp_model_adam_step enqueued back to back with a single wait at the end: what
 * session.run(minimise_op) is to the reference (conv_gp/experiment.py:84-108).  Arguments: those of the two calls.  A step whose
 * factorisation fails returns DCGP_ERR_NOT_PD and leaves parameters, moments and step count as they were (the update reads the step's
 * status word on the device). */
int dcgp_model_train_step_adam(dcgp_model* model, const double* X, const int32_t* y, int N, double scale,
                               const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0, double lr, double beta1,
                               double beta2, double eps, int t, double* out_host, int* info_host);
/* The training set of a run, resident on the device: X_host [n][H*W*C] float64, Y_host int32 [n] (y_is_f64 == 0) or float64 [n][D] for the
 * float-target likelihoods (y_is_f64 != 0; D the head's outputs) -- what the reference hands its model once as Minibatch tensors and then draws
 * from inside session.run (conv_gp/experiment.py:38-49,84-108).  Uploads once, replaces an earlier set, n == 0 releases it.  The model needs its
 * head (and its likelihood) first: the row length and the kind of target are the model's. */
int dcgp_model_set_dataset(dcgp_model* model, const double* X_host, const void* Y_host, long n, int y_is_f64);
/* `steps` training steps in one call -- gpflow.actions.Loop(self.loop, stop=test_every) over the Adam action of conv_gp/experiment.py:38-49,84-108.
 * Step i is exactly dcgp_model_train_step_adam (its _f64y twin for float targets) on rows idx_host[i][0 .. batch) of the attached set with
 * z_per_layer_host = NULL, seed seed0 + i, learning rate lr_host[i] and t = 0: elbo_host[i], every parameter, both moment buffers, the likelihood
 * parameter and the step count after the run are those of `steps` such calls bit for bit (set_trainable flags and dedup_layer0 apply as there).
 * The rows are gathered on the device (csrc/train_run.hip); the index table crosses the bus once per run, no image does.
 * Checked on the host before anything is enqueued (DCGP_ERR_ARG): a set is attached, 0 <= idx < n for every entry, steps >= 1, batch >= 1, every
 * lr > 0, no enqueued forward step outstanding, the ctx holds one rank.
 * Failure is the per-step loop's: when step j fails (DCGP_ERR_NOT_PD, *info_host = the column) the run returns that code with *steps_done = j and
 * elbo_host[0 .. j) filled; parameters, moments and step count are what step j - 1 left (a failed step's update reads the step's status word on the
 * device and changes nothing, and no later step has been enqueued).
 * The host waits once per step: the kernels take the base kernels' hyper-parameters by value from host-side state that the step's update writes. */
int dcgp_model_train_run_adam(dcgp_model* model, const int32_t* idx_host /* [steps][batch] */, int steps, int batch, double scale,
                              const double* lr_host /* [steps] */, uint64_t seed0, int dedup_layer0, double beta1, double beta2, double eps,
                              double* elbo_host /* [steps] */, int* steps_done, int* info_host);
/* Training-time augmentation of a run's batches, on the device -- what a user of the reference does on the host between session.run calls
 * (its Minibatch tensors, conv_gp/experiment.py:38-49, hold the images as they are; the reference has no augmentation of its own), here without
 * giving up the resident set.  Model state that dcgp_model_train_run_adam consults; nothing else does: evaluation, prediction, input gradients
 * and the per-step entry points see their X as it is.  H, W, C: the caller's image geometry, H * W * C == the model's row length (the unpadded
 * geometry of dcgp_model_set_dataset; a padded first layer still pads afterwards).  Image I of batch position b of step i becomes
 *     F[y][x][c] = I[y][flip ? W - 1 - x : x][c],   out[y][x][c] = F[y - dy][x - dx][c] inside the image, 0.0 outside
 * with (dy, dx, flip) drawn on the device from Philox4x32-10 under the step's seed seed0 + i at counter b (csrc/augment_map.h: the words, the
 * tag that keeps them apart from the layers' noise, dy = word0 % (2 max_shift + 1) - max_shift, dx likewise from word1, flip = hflip ? word2 & 1
 * : 0; modulo bias about (2 max_shift + 1) / 2^32).  Targets are untouched.  With dedup_layer0 an image is augmented once per step: the batch is
 * tiled afterwards.  Step i of an augmenting run is dcgp_model_train_step_adam on dcgp_augment_images(rows idx[i], seed0 + i), bit for bit.
 * max_shift == 0 && hflip == 0 switches augmentation off (H, W, C are then ignored): the run gathers on exactly the code path it had.
 * DCGP_ERR_ARG, with a message: H * W * C is not the model's row length, max_shift < 0, max_shift >= min(H, W), the model has no head yet,
 * enqueued steps are still to be collected.  No parameter: checkpoints do not hold it. */
int dcgp_model_set_augmentation(dcgp_model* model, int H, int W, int C, int max_shift, int hflip);
/* The same transform on a caller's batch: X [N][H][W][C] -> out [N][H][W][C] (device pointers; out may not alias X), image b with the draw of
 * (seed, b) -- the host-side augmentation loop a user of the reference writes around its feed (conv_gp/experiment.py:84-108), as one launch.
 * Every value of out is written.  Asynchronous on the ctx stream.  DCGP_ERR_ARG as above for the geometry and max_shift. */
int dcgp_augment_images(dcgp_ctx* ctx, const double* X, int N, int H, int W, int C, int max_shift, int hflip, uint64_t seed, double* out);
/* Test-time augmentation: the evaluation of a model trained on shifted and flipped images averages its predictive distribution over a few
 * shifted and mirrored views of each test image -- what a user of the reference does on the host around its per-batch predict_y loop
 * (conv_gp/utils/log.py), V passes and a hand-made mean; here inside the one evaluation call.  views_host [V][3] int32 (host): (dy, dx, flip)
 * per view, the transform of dcgp_model_set_augmentation with the draw replaced by the table (flip first, then the shift, zero fill).
 * Model state that dcgp_model_evaluate(_f64y), dcgp_model_predict_density(_f64y) and dcgp_model_evaluate_uncertainty(_f64y) consult; nothing
 * else does: dcgp_model_predict_y, propagate, the ELBO, the training steps and runs, input gradients and patch evidence see their X as it is.
 * With views set, a batch of n images becomes V n images, view v of image i at row v n + i, ONE forward pass on them with S samples leaves
 * head rows [S][V n][K], and since row s V n + v n + i = (s V + v) n + i the tails see S V samples of n images:
 *     p(y | x) = 1 / (S V) sum_{s, v} p(y | f_s(view_v(x))),
 * the log density the log of that mixture, p_mean / y_mean, accuracy / squared error, entropies, BALD and calibration those of the S V members
 * (the mutual information then counts disagreement between views as model uncertainty).  z_per_layer: batch b's table per layer is
 * [S][V n_b][D_l], from S * V * lo_b * D_l on.  Limits: S * V * K + K <= 8192 (+ 48 for the uncertainty tail), S * V * batch < 2^31.
 * H, W, C: the model's unpadded first-layer image (a padded first layer pads the views as it pads any batch).  V == 0 clears the setting
 * (H, W, C are then ignored); the single view (0, 0, 0) evaluates on exactly the code path of no views.
 * DCGP_ERR_ARG, with a message: another geometry than the model's, |dy| or |dx| >= min(H, W), a flip outside {0, 1}, a dense head alone (its
 * inputs are feature vectors), no head yet, enqueued steps still to be collected.  No parameter: checkpoints do not hold it. */
int dcgp_model_set_eval_views(dcgp_model* model, int H, int W, int C, int V, const int32_t* views_host /* [V][3] */);
/* The views of a caller's batch: X [N][H][W][C] -> out [V * N][H][W][C] (device pointers; out may not alias X), view v of image i at row
 * v * N + i -- the gather the evaluation runs per batch, as one launch.  Every value of out is written.  Returns when the launch is done.
 * The gather itself moves values under any shift that leaves a pixel: here the bound is per axis, |dy| < H and |dx| < W (a view of one
 * surviving row or column is allowed), where the model setting keeps the training-time bound min(H, W).  DCGP_ERR_ARG for the geometry, a
 * shift past that bound, a flip outside {0, 1}, V < 1, out aliasing X. */
int dcgp_view_images(dcgp_ctx* ctx, const double* X, int N, int H, int W, int C, int V, const int32_t* views_host /* [V][3] */, double* out);
/* Multi-rank training step (one process per GPU, dcgp_comm_init_rank): how a step's gradient is exchanged inside dcgp_model_train_step_adam.
 * 0 (default): ncclAllReduce of every layer's gradient block, every rank then updates every parameter.  1: ncclReduceScatter of the block
 * (each rank receives the sum of its shard only -- dcgp_shard_range), Adam on that shard of the layer's parameter block, ncclAllGather
 * of the updated parameters: half the bytes on the links of an all-reduce + nothing, and 1 / ranks of the optimiser arithmetic per rank
 * (the counterpart of nothing in the reference, which is single-device).  Frozen groups (dcgp_model_set_trainable)
 * pass through unchanged.  dcgp_elbo_grad on its own always all-reduces: its caller reads whole gradients. */
int dcgp_model_set_grad_exchange(dcgp_model* model, int mode);
/* Shards of a block of n values over nranks ranks: every shard ceil(n / nranks) long (the collectives want equal counts), rank r holds
 * [lo, hi) = [r * shard, min((r + 1) * shard, n)).  deepcgp_amd/dist.py grad_shard_range is the same arithmetic on the host. */
int dcgp_shard_range(long n, int nranks, int rank, long* lo, long* hi, long* shard /* may be NULL */);
/* Debugging aid: one Adam step taken the way `ranks` ranks take it in exchange mode 1, played on this one GPU from rank 0's point of view
 * (shard 0 in place, the others through the staging block and the unstage pass).  Needs the complete gradient (dcgp_elbo_grad).  Bit-identical
 * to dcgp_model_adam_step. */
int dcgp_model_debug_sharded_adam(dcgp_model* model, int ranks, double lr, double beta1, double beta2, double eps, int t);
/* Plain gradient ascent in the same unconstrained space (gpflow.train.GradientDescentOptimizer, the "SGD" branch
 * at conv_gp/experiment.py:100-103). */
int dcgp_model_sgd_step(dcgp_model* model, double lr);
/* The optimiser's own state, so that an interrupted run can go on as the run it was: Adam's moments m, v of one parameter group (in the
 * unconstrained space, the group's own layout) to / from the host, and the step count of its bias correction.  which = "Z", "q_mu", "q_sqrt",
 * "w", "hyper" (3 values: variance, p1, p2 as dcgp_model_get_grad orders them), "ard_lengthscales", "mean_filter", or "likelihood" (1 value:
 * the Gaussian variance / StudentT scale; `layer` ignored).  A model that has never stepped reports zeros and t = 0.  DCGP_ERR_ARG: unknown
 * name, wrong count, a group the layer does not have; set: enqueued steps still to be collected; both: sharded Adam steps were taken
 * (exchange mode 1: the moments are rank-local). */
int dcgp_model_get_adam_state(dcgp_model* model, int layer, const char* which, double* m_host, double* v_host, size_t count);
int dcgp_model_set_adam_state(dcgp_model* model, int layer, const char* which, const double* m_host, const double* v_host, size_t count);
int dcgp_model_get_adam_t(dcgp_model* model, int* t);
int dcgp_model_set_adam_t(dcgp_model* model, int t /* >= 0 */);
/* Clipping by global norm in the device optimiser (tf.clip_by_global_norm on gpflow's unconstrained variables): with g_u the gradient the
 * update uses for every element it moves (softplus factor included; frozen groups and held elements left out), norm = sqrt(sum g_u^2) and
 * c = max_norm / max(norm, max_norm); Adam and SGD step on c g_u.  The norm is formed on the device between the gradient and the update (two
 * small launches); norm <= max_norm gives c = 1.0 exactly and the unclipped step to the bit.  max_norm 0 (default): off, the step is launched
 * as it always was; +inf: the norm is measured, nothing is scaled; negative or NaN: DCGP_ERR_ARG.  The natural-gradient update is not clipped.
 * With clipping on, a sharded update (exchange mode 1 on more than one rank, dcgp_model_debug_sharded_adam) returns DCGP_ERR_ARG: a rank sees
 * only its shard of the gradient. */
int dcgp_model_set_grad_clip(dcgp_model* model, double max_norm);
/* The pre-clip norms of the steps of the most recent optimiser call: one after dcgp_model_adam_step / _sgd_step / _train_step_adam, steps_done
 * after dcgp_model_train_run_adam; none while clipping is off, none for a step that was not positive definite.  *count_out: how many there
 * are; the first min(cap, *count_out) go to out_host. */
int dcgp_model_grad_norms(dcgp_model* model, double* out_host, int cap, int* count_out);
/* One natural-gradient step of size gamma on every layer's (q_mu, q_sqrt) from the gradients of the last dcgp_elbo_grad:
 * gpflow.train.NatGradOptimizer(gamma) on var_list = [(l.q_mu, l.q_sqrt)] (conv_gp/experiment.py:90-99), natural-parameter
 * form theta <- theta + gamma dELBO/d eta.  Returns DCGP_ERR_NOT_PD (nothing written, *info = failing column) when a new
 * precision matrix is not positive definite: the reference's loop then scales gamma by 0.2 and retries (:36-49). */
int dcgp_model_natgrad_step(dcgp_model* model, double gamma, int* info_host);
/* param.set_trainable(False / True) (conv_gp/experiment.py:93-95, models.py:100): parameters switched off are left
 * alone by the Adam / SGD steps.  which = "Z", "q_mu", "q_sqrt", "w", "hyper" (variance and lengthscale), or "mean_filter" (a conv layer
 * with a filter mean, conv_gp/mean_functions.py:6-41, conv_gp/layers.py:133-134: frozen, its gradient is not formed either). */
int dcgp_model_set_trainable(dcgp_model* model, int layer, const char* which, int on);
/* current (constrained) value of a parameter, names as dcgp_model_get_grad; the inverse of dcgp_model_set_param -- what
 * sess.run(param.constrained_tensor) returns when the reference writes its checkpoint (conv_gp/experiment.py:56-64) */
int dcgp_model_get_param(dcgp_model* model, int layer, const char* which, double* out_host, size_t count);
/* DGP_Base.propagate(X, S) -> last layer's Fmean, Fvar [S*N, R] (device buffers owned by caller) */
int dcgp_model_propagate(dcgp_model* model, const double* X, int N, int S,
                         const double* const* z_per_layer_host, uint64_t seed,
                         double* out_fmean, double* out_fvar, int* info_host);
/* DGP_Base.predict_y(X, S) with the RobustMax or Softmax likelihood, device end to end (doubly_stochastic_dgp
 * predict_y -> likelihood.predict_mean_and_var; caller at conv_gp/utils/log.py:62-66): out_p [S*N, K]
 * class probabilities per sample (the predictive variance is p - p^2), out_p_mean [N, K] their mean over
 * the S samples (what AccuracyLogger arg-maxes).  Either output may be NULL, not both.  Device buffers. */
int dcgp_model_predict_y(dcgp_model* model, const double* X, int N, int S,
                         const double* const* z_per_layer_host, uint64_t seed,
                         double* out_p, double* out_p_mean, int* info_host);
/* DS-DGP DGP_Base.predict_density(X, Y, S): per image logsumexp_s log p(y | f_s) - log S, RobustMax or Softmax likelihood. out_logdens [N], device.
 * The class probabilities are dcgp_model_predict_y's; y [N] int32 in [0, K) (device), else DCGP_ERR_ARG.                              */
int dcgp_model_predict_density(dcgp_model* model, const double* X, const int32_t* y, int N, int S,
                               const double* const* z_per_layer, uint64_t seed, double* out_logdens, int* info_host);
/* Input gradients (saliency maps, adversarial examples; the reference's users get them from tf.gradients on predict_density / the ELBO).
 * Per image n of the batch an objective J_n, with the noise fixed by z_per_layer or seed exactly as in dcgp_model_predict_density:
 *   DCGP_OBJECTIVE_DENSITY  J_n = log(1/S sum_s p(y_n | f_sn)), dcgp_model_predict_density's value (RobustMax and Softmax models; a Gaussian or
 *                           Bernoulli model gets DCGP_ERR_ARG, never the other objective),
 *   DCGP_OBJECTIVE_ELBO     J_n = 1/S sum_s E_q[log p(y_n | f_sn)], the image's share of the ELBO's data term, unscaled, without the KL.
 * out_value [N] = J (device, may be NULL), out_dX [N][H*W*C] = dJ_n / dX_n (device; the layers treat images independently, so it is
 * also d(sum_n J_n) / dX).  `objective` may be OR-ed with DCGP_INPUT_GRAD_DEDUP: layer 0's conditional runs on the N distinct images
 * instead of the batch tiled S times (dcgp_elbo_grad's dedup_layer0; the same result up to summation order).
 * One call: a forward pass that keeps the layer outputs, the objective's adjoint at the head, and the data path only of the reverse
 * pass down to layer 0 -- no parameter gradient is formed.  Parameters, the gradient blocks (dcgp_model_get_grad), Adam moments, the step
 * count and the parameter version (dcgp_model_set_factor_reuse keeps its chain, and this call uses it) are left as they were; no atomics,
 * so two calls give the same bits.  y [N] int32 in [0, K) (device), else DCGP_ERR_ARG; DCGP_ERR_NOT_PD with *info_host as elsewhere. */
#define DCGP_OBJECTIVE_DENSITY 0
#define DCGP_OBJECTIVE_ELBO 1
#define DCGP_INPUT_GRAD_DEDUP 0x100
int dcgp_model_input_grad(dcgp_model* model, const double* X, const int32_t* y, int N, int S,
                          const double* const* z_per_layer, uint64_t seed, int objective,
                          double* out_value, double* out_dX, int* info_host);
/* A whole test set in batches of `batch` images, enqueued back to back, ONE stream synchronisation per call -- the loops of the reference's
 * AccuracyLogger (conv_gp/utils/log.py:50-67) and of a test log density over DS-DGP DGP_Base.predict_density, one device call.
 * Batch b = images [b*batch, min((b+1)*batch, N_total)), noise from seed + b (AccuracyLogger's convention), or from
 * z_per_layer: per layer one device buffer holding the batches' [S][n_b][D] tables back to back.
 * out_logdens [N_total], out_p_mean [N_total][K]: device, either may be NULL. out_host[2] = {correct count, sum of logdens}.
 * "Correct": the first arg-max of the sample-mean probabilities (bit-identical to predict_y's out_p_mean) equals the label.
 * Factor reuse (dcgp_model_set_factor_reuse) as for predict_y: in modes 1 and 2 the parameter-only chain runs at most once per call.
 * Rank-local: with a communicator attached nothing is reduced across ranks; each rank evaluates the images it is given.
 * Labels outside [0, K) are DCGP_ERR_ARG (checked on the device, reported after the sync), so are batch <= 0 and K < 2.            */
int dcgp_model_evaluate(dcgp_model* model, const double* X, const int32_t* y, int N_total, int batch, int S,
                        const double* const* z_per_layer, uint64_t seed, double* out_logdens, double* out_p_mean,
                        double* out_host, int* info_host);

/* ---- Gaussian and Bernoulli likelihoods (gpflow 1.x likelihoods.Gaussian / Bernoulli under DS-DGP's BroadcastingLikelihood) ----
 * The likelihood of the model: kind 0 = RobustMax (the default; int32 labels), 1 = Gaussian with one variance s2 > 1e-6 shared by every
 * output (float64 targets y [N, K], K = the head's outputs; gpflow's transforms.positive, s2 = softplus(u) + 1e-6, in the optimiser),
 * 2 = Bernoulli with gpflow's jittered probit link p(f) = Phi(f) (1 - 2e-3) + 1e-3 (`variance` ignored; float64 targets y [N, K], every
 * output an independent binary label: y == 1.0 positive, anything else negative, as gpflow's tf.equal(y, 1)), 3 = Softmax (`variance`
 * ignored; int32 labels, see dcgp_model_set_likelihood_nodes below).  Other kinds are refused.
 * Replaces the likelihood argument of DS-DGP DGP_Base.__init__.  Call after dcgp_model_set_head and before the first gradient: once a
 * gradient was taken the kind is fixed.
 * Bernoulli has no parameter: its gradient block has the RobustMax layout and length, and it has no "likelihood_variance".  Its
 * variational expectation per (row, output) is 20-node Gauss-Hermite quadrature, sum_i w_i / sqrt(pi) log p(y | mu + sqrt(2 var) x_i)
 * (2 var clamped at 1e-10); the gradient is the exact derivative of that sum.  On the _f64y entry points below a Bernoulli model gives:
 * dcgp_model_predict_mean_var out_mean = p = Phi~(mu / sqrt(1 + var)) (Phi~ the jittered probit), out_var = p - p^2;
 * dcgp_model_predict_density_f64y out_logdens [N, K] = logsumexp_s log p(y | p_s) - log S; dcgp_model_evaluate_f64y out_y_mean
 * [N_total][K] = the sample-mean p, out_host[2] = {number of (image, output) entries whose label is 1 exactly where that mean is > 0.5,
 * sum of the per-image log densities}.  The formulas with s2 below are kind 1's.
 * On a Gaussian or Bernoulli model the int32 entry points above (dcgp_elbo_forward, _enqueue, dcgp_elbo_grad, dcgp_model_train_step_adam,
 * dcgp_model_predict_y, dcgp_model_predict_density, dcgp_model_evaluate) return DCGP_ERR_ARG, and so do the _f64y ones below on a
 * RobustMax model.  s2 is "likelihood_variance" in dcgp_model_set_param / _get_param / _get_grad / _set_trainable (`layer` ignored); its
 * gradient is the last slot of the head's gradient block (dcgp_model_grad_block), after the ARD lengthscales. */
int dcgp_model_set_likelihood(dcgp_model* model, int kind, double variance);
/* The Softmax likelihood, dcgp_model_set_likelihood(model, 3, 0.0) (gpflow 1.x likelihoods.SoftMax as a MonteCarloLikelihood, its per-call
 * draw replaced by a fixed table): per head row, with the node table e [Q, K], s = sqrt(max(var, 1e-10)) and f_q = mu + s * e_q,
 *   variational expectation 1/Q sum_q (f_q[y] - logsumexp_k f_q[k]),  class probabilities p = 1/Q sum_q softmax(f_q),
 * the gradient the exact derivative of that sum (d / d var = 0 where the clamp holds), the log density per image log(1/S sum_s p_s[y]).
 * It takes int32 labels in [0, K) through the int32 entry points: dcgp_elbo_forward, _enqueue, dcgp_elbo_grad, dcgp_model_train_step_adam,
 * the SGD and natural-gradient steps, dcgp_model_predict_y, dcgp_model_predict_density, dcgp_model_evaluate,
 * dcgp_model_evaluate_uncertainty and dcgp_model_input_grad with both objectives; the _f64y entry points return DCGP_ERR_ARG on it.  It has
 * no trainable parameter: the gradient blocks have the RobustMax layout and length.  Kind 3 is chosen in place of the default RobustMax
 * (K >= 2): a model already set to a float64-target likelihood (kind 1 or 2) refuses it with DCGP_ERR_ARG.
 * dcgp_model_set_likelihood_nodes copies the host table nodes_host [Q, K] (row q = node q; K = the head's outputs) to the device.
 * 1 <= Q and Q * K <= 4096 (32 KB of LDS), else DCGP_ERR_ARG; Q may differ from call to call.  Allowed whenever no enqueued step is
 * outstanding (else DCGP_ERR_ARG).  The table is no parameter: the call starts no new parameter version, so dcgp_model_set_factor_reuse
 * keeps its chain.  A kind-3 model without a table refuses every step with DCGP_ERR_ARG; on a model of another kind the call is
 * DCGP_ERR_ARG.  Every sum runs in a fixed order (no atomics): two calls give the same bits, whatever the number of ranks. */
int dcgp_model_set_likelihood_nodes(dcgp_model* model, const double* nodes_host, int Q);
/* The StudentT and Poisson likelihoods of a model (gpflow 1.x likelihoods.StudentT(scale, deg_free) / likelihoods.Poisson(invlink=exp, binsize)
 * under DS-DGP's BroadcastingLikelihood; replaces the likelihood argument of DS-DGP DGP_Base.__init__ for them): kind 4 with params_host =
 * {scale, deg_free} (n = 2; scale > 1e-6, deg_free > 2), kind 5 with params_host = {binsize} (n = 1; binsize > 0).  Float64 targets y [N, K]
 * (Poisson: non-negative integer values) through the _f64y entry points, every output an independent target; the formulas are those of
 * dcgp_quad_varexp / _predict / _logdensity above, the gradient the exact derivative of what the forward computes (d / d var = 0 where the
 * clamp holds), dcgp_model_predict_mean_var gives (E_y, V_y), dcgp_model_predict_density_f64y logsumexp_s ld_s - log S per (image, output),
 * dcgp_model_evaluate_f64y what it gives a Gaussian model (the squared error of the sample-mean E_y).  The StudentT scale is trainable: it
 * lives where the Gaussian variance does (the same positive transform softplus + 1e-6, its gradient in the last slot of the head's gradient
 * block) and is "likelihood_scale" in dcgp_model_set_param / _get_param / _get_grad / _set_trainable (`layer` ignored; a value must be
 * > 1e-6; DCGP_ERR_ARG on a model of another kind); deg_free is fixed.  Poisson has no trainable parameter: its gradient blocks have the
 * RobustMax layout.  dcgp_model_predict_y, dcgp_model_evaluate_uncertainty(_f64y), the density objective of dcgp_model_input_grad and the int32
 * entry points return DCGP_ERR_ARG on these models.  DCGP_ERR_ARG too for a bad value, a wrong n, any other kind (dcgp_model_set_likelihood
 * sets those, and itself refuses kinds 4 and 5), a model that has taken steps with int32 labels, enqueued steps outstanding, or another
 * kind than the model's once a gradient was taken. */
int dcgp_model_set_likelihood_params(dcgp_model* model, int kind, const double* params_host, int n);
/* dcgp_elbo_forward / _enqueue with Gaussian targets y [N, K] float64 (device): DGP_Base._build_likelihood with
 * Gaussian.variational_expectations = -0.5 log(2 pi s2) - 0.5 ((y - mu)^2 + var) / s2 summed over the K outputs.  Tickets are
 * collected with dcgp_elbo_forward_collect. */
int dcgp_elbo_forward_f64y(dcgp_model* model, const double* X, const double* y, int N, double scale,
                           const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0, double* out_host,
                           int* info_host);
int dcgp_elbo_forward_enqueue_f64y(dcgp_model* model, const double* X, const double* y, int N, double scale,
                                   const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0, uint64_t* ticket);
/* dcgp_elbo_grad / dcgp_model_train_step_adam with Gaussian targets (TensorFlow autodiff of the same objective; the Adam step also
 * moves s2 unless it was set non-trainable). */
int dcgp_elbo_grad_f64y(dcgp_model* model, const double* X, const double* y, int N, double scale,
                        const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0, double* out_host,
                        int* info_host);
int dcgp_model_train_step_adam_f64y(dcgp_model* model, const double* X, const double* y, int N, double scale,
                                    const double* const* z_per_layer_host, uint64_t seed, int dedup_layer0, double lr, double beta1,
                                    double beta2, double eps, int t, double* out_host, int* info_host);
/* DS-DGP DGP_Base.predict_y with Gaussian.predict_mean_and_var: out_mean = Fmean, out_var = Fvar + s2, each [S*N, K] (device; either
 * may be NULL, not both).  Only the head's outputs are written. */
int dcgp_model_predict_mean_var(dcgp_model* model, const double* X, int N, int S,
                                const double* const* z_per_layer_host, uint64_t seed,
                                double* out_mean, double* out_var, int* info_host);
/* Per-patch evidence maps of the model's patch head: X goes through the hidden layers exactly as in dcgp_model_propagate for the
 * same (S, z, seed); out_c [S*N][P][R] (device) = (w_p/P) sum_m k(z_m, h[p]) beta[m,r] on the head's input h, beta = L^-T q_mu
 * (whitened) or Kuu^-1 q_mu from the chain's own factors; out_fmean [S*N][R] (device, may be NULL) the head's mean, = sum_p out_c.
 * Any likelihood.  Replaces dcgp_model_propagate + dcgp_model_layer_output + dcgp_kuf_patches_rbf + dcgp_gemm_strided and host
 * arithmetic for beta (conv_gp/utils/tensorboard.py:164-195).  A dense RBF head has no patches: DCGP_ERR_ARG.  Rank-local.
 * N == 0: DCGP_OK, nothing written. */
int dcgp_model_patch_evidence(dcgp_model* model, const double* X, int N, int S, const double* const* z_per_layer, uint64_t seed,
                              double* out_c, double* out_fmean, int* info_host);
/* DS-DGP DGP_Base.predict_density with Gaussian.predict_density: out_logdens [N, K] (device) =
 * logsumexp_s log N(y; mu_s, var_s + s2) - log S per image and output. */
int dcgp_model_predict_density_f64y(dcgp_model* model, const double* X, const double* y, int N, int S,
                                    const double* const* z_per_layer, uint64_t seed, double* out_logdens, int* info_host);
/* dcgp_model_input_grad with float64 targets y [N, K] (device) for a Gaussian or Bernoulli model: DCGP_OBJECTIVE_ELBO only, J_n summed
 * over the K outputs. */
int dcgp_model_input_grad_f64y(dcgp_model* model, const double* X, const double* y, int N, int S,
                               const double* const* z_per_layer, uint64_t seed, int objective,
                               double* out_value, double* out_dX, int* info_host);
/* dcgp_model_evaluate for a Gaussian model: out_logdens [N_total] per image (summed over the K outputs), out_y_mean [N_total][K] the
 * sample-mean prediction (device, either may be NULL); out_host[2] = {sum of the squared errors of the sample-mean prediction, sum of
 * the per-image log densities}. */
int dcgp_model_evaluate_f64y(dcgp_model* model, const double* X, const double* y, int N_total, int batch, int S,
                             const double* const* z_per_layer, uint64_t seed, double* out_logdens, double* out_y_mean,
                             double* out_host, int* info_host);
/* dcgp_model_evaluate with the uncertainty of every prediction kept: DS-DGP DGP_Base.predict_y hands its caller the S samples of the class
 * probabilities p[s][k] (the reference's AccuracyLogger, conv_gp/utils/log.py:62-67, averages them and keeps the arg-max); here the device
 * reduces them per image, in nats, to
 *   out_pred_entropy  H(pbar) = -sum_k pbar[k] log pbar[k],  pbar = the sample mean (out_p_mean, bit-identical to dcgp_model_evaluate's),
 *   out_exp_entropy   1/S sum_s H(p[s]),
 *   out_mutual_info   their difference (BALD; the raw difference, >= 0 up to rounding, not clipped),
 *   out_confidence    max_k pbar[k],   out_prediction (int32) its first index,
 * each [N_total], device, any may be NULL; out_logdens [N_total] and out_p_mean [N_total][K] as dcgp_model_evaluate's.  Behind the last batch
 * one launch bins the confidences into `bins` equal-width bins, b = min(bins - 1, floor(confidence * bins)): out_table [bins][3] =
 * {count, sum of confidences, number correct} (device, may be NULL), and out_host[7] = {correct count, sum of logdens, ECE = sum_b
 * count_b / n |accuracy_b - mean confidence_b|, MCE = the largest of those gaps, Brier score 1/n sum_i sum_k (pbar[i][k] - [y_i = k])^2,
 * mean predictive entropy, mean mutual information}.  Batches, seeds (seed + b), z_per_layer layout, factor reuse and the single stream
 * synchronisation are dcgp_model_evaluate's; sums run in a fixed order without atomics, so two calls agree bit for bit.  Rank-local.
 * y may be NULL (unlabelled images: acquisition scores, out-of-distribution checks): out_logdens is not written, the table's third column is
 * 0 and words 0, 1, 2, 3, 4 of out_host are NaN.  DCGP_ERR_ARG: bins < 1, batch <= 0, K < 2, a label outside [0, K) (checked on the device,
 * reported after the sync), S * K + K + 48 > 8192 (the tail's LDS), a Gaussian or Bernoulli model. */
int dcgp_model_evaluate_uncertainty(dcgp_model* model, const double* X, const int32_t* y, int N_total, int batch, int S,
                                    const double* const* z_per_layer, uint64_t seed, int bins, double* out_logdens, double* out_p_mean,
                                    double* out_pred_entropy, double* out_exp_entropy, double* out_mutual_info, double* out_confidence,
                                    int32_t* out_prediction, double* out_table, double* out_host, int* info_host);
/* The same for a Bernoulli model (dcgp_model_evaluate_f64y; DS-DGP DGP_Base.predict_y with gpflow's Bernoulli.predict_mean_and_var):
 * targets y [N_total][K] float64 (may be NULL), every (image, output) pair an entry with p = the jittered probit of mu / sqrt(1 + var) and the
 * binary entropy h(q) = -q log q - (1 - q) log(1 - q) in place of H; confidence = max(pbar, 1 - pbar), prediction = pbar > 0.5, Brier term
 * (pbar - y)^2.  The per-entry outputs are [N_total][K], n = N_total K entries; out_logdens [N_total] is summed over the K outputs.
 * DCGP_ERR_ARG on a RobustMax or Gaussian model. */
int dcgp_model_evaluate_uncertainty_f64y(dcgp_model* model, const double* X, const double* y, int N_total, int batch, int S,
                                         const double* const* z_per_layer, uint64_t seed, int bins, double* out_logdens, double* out_p_mean,
                                         double* out_pred_entropy, double* out_exp_entropy, double* out_mutual_info,
                                         double* out_confidence, int32_t* out_prediction, double* out_table, double* out_host,
                                         int* info_host);
/* Parameter-only state across steps.  The reference's evaluation loops run hundreds of batches at ONE parameter state (AccuracyLogger /
 * LogLikelihoodLogger, conv_gp/utils/log.py:55-68; conv_gp/utils/tensorboard.py:22-42), and every session.run of them factors every Kuu again.
 * Here a step records the parameter version its chain (operand preparation, factorisations, inverses, G / alpha, KL pieces) ran at; every call that writes
 * a parameter -- dcgp_model_set_param, the Adam / SGD / natural-gradient steps -- starts a new version.  mode 0: never reuse; 1 (default):
 * dcgp_model_propagate and dcgp_model_predict_y skip the chain while the version stands; 2: the forward ELBO (dcgp_elbo_forward) as well -- for
 * evaluation sweeps; a TRAINING step's forward pass never reuses it, and bench.py's headline never runs in mode 2 (the reference's step recomputes).
 * Results are bit-identical to a step that runs the chain.  dcgp_model_chain_skips: steps that reused it so far. */
int dcgp_model_set_factor_reuse(dcgp_model* model, int mode);
int dcgp_model_chain_skips(dcgp_model* model, uint64_t* out);
/* The factor groups of the model's most recent step (one batched factorisation chain per distinct padded size Mp = round_up(M, 16)): *count_out groups,
 * none before the first step; for the first min(*count_out, cap) of them the padded size, the number of matrices the chain factors (every layer's Kuu(Z) and,
 * for conv layers, the prior's Kuu(Z0)) and how many of those carried their right-hand sides G / alpha on the chain in that step.  Host arrays of `cap`
 * entries; reads host state only. */
int dcgp_model_factor_groups(dcgp_model* model, int cap, int* count_out, int* Mp_out, int* matrices_out, int* riding_out);
/* Output of layer `layer` from the most recent forward: sample/mean/var [rows, D_l] device->device copy. */
int dcgp_model_layer_output(dcgp_model* model, int layer, double* out_sample, double* out_mean,
                            double* out_var, int* rows, int* width);

/* The strided fp64 GEMM of the training step, as an operator (every tf.matmul / tf.tensordot of the reverse pass, e.g.
 * the adjoints of conv_gp/conditionals.py:50,58, runs on it):
 *   C_b(i, j) (+)= alpha * colscale_b[j] * sum_k A_b(i, k) * kscale_b[k] * B_b(k, j),   b = 0 .. batch-1,
 *   A_b(i, k) = A[b a_bs + i a_rs + k a_cs],  B_b(k, j) = B[b b_bs + k b_rs + j b_cs],  C_b(i, j) = C[b c_bs + i c_rs + j];
 * colscale / kscale may be NULL.  flags bit 0: lower_only -- 0 is written above the diagonal (before accumulation); bit 1 (with bit 0, square
 * results only): mirror -- the entries below the diagonal are also stored transposed and nothing else is written above it (with accumulate:
 * the lower triangle accumulates, the upper one is its mirror image).  0 and 1 are what this argument meant when it was `lower_only`; other
 * bits are refused.  kscale with flags = 3 on A == B (k contiguous, 129 .. 256 rows, K >= 8192) is the reverse pass's W_r, which has a kernel
 * of its own (dcgp_debug_plan_gemm says which kernel serves a call).  Device pointers. */
int dcgp_gemm_strided(dcgp_ctx* ctx, const double* A, long a_rs, long a_cs, long a_bs, const double* B, long b_rs,
                      long b_cs, long b_bs, double* C, long c_rs, long c_bs, int M, int N, int K, int batch,
                      double alpha, int accumulate, const double* colscale, long cs_s, long cs_bs,
                      const double* kscale, long ks_s, long ks_bs, int flags);
/* The same product with the epilogues of the kernel adjoints (dZ = (E X - rowsum(E) o Z) / l^2 and its kin, Murray's Phi of the Cholesky
 * adjoint, symmetric products computed on the lower tiles only):
 *   C_b(i, j) (+)= alpha * (sum_k A_b(i, k) B_b(k, j) - sub_v[b sv_bs + i] * sub_x[b sx_bs + i sx_rs + j])      (sub_v, sub_x: both or neither)
 * flags bit 0: lower_only; bit 1 (with bit 0): mirror -- entries below the diagonal are also stored transposed, nothing else is written
 * above it; bit 2: phi -- the strictly lower part is kept, the diagonal halved, the rest written as zero. */
int dcgp_gemm_strided_ex(dcgp_ctx* ctx, const double* A, long a_rs, long a_cs, long a_bs, const double* B, long b_rs,
                         long b_cs, long b_bs, double* C, long c_rs, long c_bs, int M, int N, int K, int batch,
                         double alpha, int accumulate, const double* sub_v, long sv_bs, const double* sub_x, long sx_rs,
                         long sx_bs, int flags);

/* ---- initialisation ---------------------------------------------------------------------------------------------- */
/* Lloyd's k-means of n points [n, d] (device) into k centres [k, d] (device): the inducing-patch initialisation of
 * PatchInducingFeatures.from_images (conv_gp/kernels.py:147-164: sklearn KMeans(n_clusters=M, init='random')).
 * init_rows_host: k row indices, the 'random' initial centres (drawn by the caller); stops after max_iter iterations or
 * when the summed squared centre shift is <= tol.  Deterministic for given initial rows. */
int dcgp_kmeans(dcgp_ctx* ctx, const double* X, long n, int d, int k, const int32_t* init_rows_host, int max_iter,
                double tol, double* centers, int* iters_out);
/* Greedy conditional-variance selection of k of n candidate points X [n, d] (device, row-major) under a base kernel: a partial pivoted
 * Cholesky factorisation of the candidates' Gram matrix (Burt, Rasmussen & van der Wilk, JMLR 2020; robustgp.ConditionalVariance, the
 * initialisation gpflow's documentation recommends) -- the kernel-aware alternative to the k-means above; the reference has no counterpart.
 * The residual starts at the Gram matrix's diagonal (variance; acos: variance (1 - acos(1 - 1e-15) / pi), the entry dcgp_kuu_acos writes).
 * Pick m takes the candidate of largest residual (ties: lowest index), stops when that is
 * <= min_variance (*n_greedy_out = m), else sets c_m[i] = (k(x_i, x_j) - sum_{t<m} c_t[j] c_t[i]) / sqrt(d_j) (c_m[j] = sqrt(d_j); 0 where d_i is
 * already 0) and d_i = max(d_i - c_m[i]^2, 0), d_j = 0.
 * kernel_type / variance / p1 / p2 as dcgp_model_set_param's "base_kernel" (0 rbf, 1 acos, 2 matern32, 3 matern52; p1 the lengthscale,
 * or for acos the weight variance with p2 the bias variance); k is evaluated as dcgp_kuu_rbf / _acos / _matern evaluate it.
 * ard_lengthscales [d] (device) or NULL: per-dimension lengthscales, rbf only (p1 is then not used).
 * rows_out [k] (device, int32): the picks in order, -1 behind n_greedy.  trace_out [k]: sum_i d_i after every pick (the Nystrom trace
 * tr(K_ff - Q_ff) of the candidates), the last value repeated behind n_greedy.  residual_out [n]: the final d.  factor_out [k, n] or NULL:
 * the rows c_m (zero behind n_greedy): factor_out[:, rows]^T is the lower Cholesky factor of K(X[rows]), factor_out^T factor_out the Nystrom
 * approximation of the candidates' Gram matrix.  n <= 2^31 - 1, k <= 4096, d <= 4096.  One launch per pick, no synchronisation between
 * them; scratch (the transposed candidates, the factor when factor_out is NULL) is allocated and freed inside the call.  Deterministic.
 * A residual that is not finite (candidates that are not) is DCGP_ERR_ARG. */
int dcgp_greedy_variance(dcgp_ctx* ctx, const double* X, long n, int d, int k, int kernel_type, double variance, double p1, double p2,
                         const double* ard_lengthscales, double min_variance, int32_t* rows_out, double* trace_out,
                         double* residual_out, double* factor_out, int* n_greedy_out);
/* out [m, n] = k(a_i, b_j) for A [m, d], B [n, d] (device, row-major) under a base kernel; kernel_type / variance / p1 / p2 / ard_lengthscales
 * as dcgp_greedy_variance.  Every entry is the OFF-diagonal form of the kernel (what dcgp_kuu_* write off their diagonal): no jitter and no
 * diagonal constant, also where a row of B equals a row of A.  x.z, |x|^2 and |z|^2 are accumulated by one chain over d, so coincident rows
 * are at distance exactly 0.  m <= 32 * 65535, n <= 2^31 - 1, d <= 4096.  The ARD lengthscales are not read back: non-positive ones give
 * non-finite entries. */
int dcgp_cross_gram(dcgp_ctx* ctx, const double* A, long m, const double* B, long n, int d, int kernel_type, double variance, double p1,
                    double p2, const double* ard_lengthscales, double* out);
/* q(u) = N(q_mu, q_sqrt_r q_sqrt_r^T) at inducing inputs Z [M, L] projected onto Z_new [M_new, L]: q'(u') = int p(u' | u) q(u) du under the
 * base kernel's prior.  With K = k(Z, Z) + jitter I = L L^T, Kc = k(Z, Z_new) (dcgp_cross_gram) and Kn = k(Z_new, Z_new) + jitter I = L' L'^T
 * (K, Kn as dcgp_kuu_* evaluate them):  B = inv(L) Kc, P = inv(L)^T B, out_q_mu = P^T q_mu, T_r = q_sqrt_r^T P,
 * out_q_sqrt_r = chol(Kn - B^T B + T_r^T T_r): lower triangular, exact zeros above the diagonal, positive diagonal.  u and u' carry
 * independent jitter (the joint prior is positive definite and Kn - B^T B keeps its smallest eigenvalue near 2 jitter), so a transfer onto the
 * same Z is a projection, not the identity.  white != 0: q_mu / q_sqrt arrive and leave in whitened coordinates (L q_mu, L q_sqrt_r are
 * projected; inv(L') of the results is returned -- a product of lower-triangular factors).  q_mu [M, R], q_sqrt [R, M, M] (lower triangle read),
 * out_q_mu [M_new, R], out_q_sqrt [R, M_new, M_new], all device.  M, M_new <= 1024, R <= 64, L <= 4096.
 * Everything is enqueued on the ctx's stream and formed in scratch that lives inside the call; the outputs are written by the last two
 * launches, which read the factorisations' status on the device, and the only host synchronisation is the read of that status.  A matrix
 * that is not positive definite: DCGP_ERR_NOT_PD, the outputs untouched; info_host [2] (may be NULL): [0] = 0, or 1 for K, 2 for Kn,
 * 3 + r for S'_r (the first that failed); [1] = its 1-based failing column.  No atomics: the same bits every run. */
int dcgp_inducing_transfer(dcgp_ctx* ctx, const double* Z, int M, const double* Z_new, int M_new, int L, int kernel_type, double variance,
                           double p1, double p2, const double* ard_lengthscales, double jitter, int white, const double* q_mu,
                           const double* q_sqrt, int R, double* out_q_mu, double* out_q_sqrt, int* info_host);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ------------------------------------------ */
/* Side effect of the two set-up calls below: RCCL prints a version banner to stdout the first time; while the call runs the process's
 * file descriptor 1 points at stderr (so for that window other host threads' stdout lands there too).  The swap is serialised
 * process-wide. */
int dcgp_comm_unique_id(unsigned char* out_128bytes);
int dcgp_comm_init_rank(dcgp_ctx* ctx, int nranks, int rank, const unsigned char* id_128bytes);
int dcgp_comm_destroy(dcgp_ctx* ctx);
/* ranks RCCL itself reports for the ctx's communicator (ncclCommCount); 0 without one */
int dcgp_comm_count(dcgp_ctx* ctx, int* out_ranks);
int dcgp_allreduce_sum_f64(dcgp_ctx* ctx, double* buf_dev, int n);

/* ---- debugging aids: TEST-ONLY entry points (tests/, tools/); nothing of the reference's interface maps onto them and no product path calls them ---- */
/* With a communicator, a FORWARD step kept in flight (dcgp_elbo_forward_enqueue with no reverse pass behind it) hands the data term's all-reduce and
 * the ELBO assembly to a comm stream, so that the next kernels on the main stream do not queue behind the collective (a training step keeps its
 * collectives on the main stream: one communicator's collectives stay on one stream).  The gate lets a test
 * prove it: closed != 0 -- every such all-reduce enqueued from now on first waits (at most ~4 s) for the gate; 0 -- opens and removes it.
 * main_idle_out (may be NULL): bit 0 -- the ctx's main stream has drained (hipStreamQuery), bit 1 -- the comm stream has. */
int dcgp_debug_comm_gate(dcgp_ctx* ctx, int closed, int* main_idle_out);
/* `count` empty launches of `wgs` workgroups, each behind the one before on the ctx's stream; *ms_out = their time by HIP events: what the
 * kernel boundaries of dcgp_greedy_variance's pivot loop cost by themselves (tools/inducing_init_time.py). */
int dcgp_debug_empty_launches(dcgp_ctx* ctx, int count, int wgs, double* ms_out);
/* Device buffer of 8 x 4 x 16 x 16 int64 into which the one-launch conv layer kernel (csrc/conv_fused.hip) stamps the shader
 * clock at its phase boundaries (8 sampled workgroups x 4 strips of a persistent one x 16 waves x 16 stamps = 8192 words); NULL switches it off (tools/fused_trace.py). */
int dcgp_debug_set_fused_trace(dcgp_ctx* ctx, long long* buf_dev);
/* How the most recent launch of that kernel was dealt: out4 = {persistent workgroups (0: one workgroup per strip), items the device counter deals,
 * hand-over slots, distinct strips whose prologue the replicas of a tiled batch share (0: not shared)}. */
int dcgp_debug_fused_plan(dcgp_ctx* ctx, int* out4);
/* The whole plan of such a launch (csrc/fused_plan.h, plan_layer_launch) for a layer described by integers alone: needs no ctx and no device.
 * query[29] = {Mp, M, R, Rp, Kc, P, HWC, L, Lp, Lz, f, C, n_mod, rep, base-kernel type, has_G (the layer has a q_sqrt term), keeps_state (K_uf / A1 are
 *   kept for the reverse pass), has_trace (dcgp_debug_set_fused_trace is on), n_cus (compute units of the device), then the ctx options fused_shape,
 *   fused_large, fused_split, fused_persist, fused_pre, fused_parts, fused_rep_share, fused_wgs, fused_stagger, sweep_no_rows}.
 * plan[24] = {ok (0: the kernel does not cover the layer; the rest is then not set), shape, LDS bytes, lds_main, lds_img, grid, persist (workgroups of a
 *   persistent launch, 0: none), n_strips, n_items (both 0 unless persistent), deal (0: one workgroup per strip, 1: device counter, 2: fixed stride),
 *   split_first, split_q, pre_n, pre_first, pre_sq, pre_D, pre_whole, pre_stride, stagger, cu_slots (the per-CU arrival counters are needed),
 *   patch_rows (the patch-row instance of the sweep), then the makespans of the simulated deals that were compared, in outputs of the second product,
 *   each an IEEE double BIT-CAST into its 64-bit slot (0.0: not simulated): one item per strip, prologues ahead, replicas sharing a prologue}.
 * dcgp_debug_fused_plan's four values are persist, n_items, pre_n and pre_D of the plan of the launch.  DCGP_ERR_ARG unless n_query == 29, n_plan == 24. */
int dcgp_debug_plan_layer_launch(const long long* query, int n_query, long long* plan, int n_plan);
/* How a call of the strided GEMM is launched (csrc/gemm_plan.h, plan_gemm: the function gemm_gen() itself launches from), for a call described by
 * integers alone: needs no ctx and no device.
 * query[24] = {M, N, K, batch, a_rs, a_cs, a_bs, b_rs, b_cs, b_bs, accumulate, colscale given, kscale given, sub_v / sub_x given, lower_only, mirror,
 *   phi, the A pointer is a multiple of 16 bytes, the B pointer is, A and B are the same pointer, one of A / B / C is NULL, then the ctx options
 *   gemm_tile and no_syrk, n_cus (compute units of the device)}.
 * plan[17] = {route (0: nothing to do, 1: gemm_gen_kernel, 2: syrk_kscale_kernel), error (0: none, 1: bad arguments, 2: batch x split > 65535,
 *   3: a lower_only result on the compact grid that is not square; with an error nothing is launched), tile, threads, tile of a wave, ksplit (1: direct
 *   store), kchunk (columns of a range), lower_compact (the grid enumerates the tiles on / below the diagonal only), AKF, BKF, VEC (the kernel's
 *   template switches), grid x, y, z, doubles of the partial buffer, workgroups of the reduction behind it (both 0 unless split), dynamic LDS bytes}.
 * DCGP_ERR_ARG unless n_query == 24, n_plan == 17. */
int dcgp_debug_plan_gemm(const long long* query, int n_query, long long* plan, int n_plan);
/* How launch jp of the factorisation chain is laid out (csrc/chain_plan.h, plan_launch: the function factor_inverse_batched itself launches from) and what
 * every workgroup of its grid decodes to (decode_iso, decode_rhs: the functions chol_rl_kernel itself calls), from integers alone: needs no ctx and no device.
 * query[8] = {Mp, batch, jp, inv(L) is formed, right-hand sides ride, max_R (the largest R of the batch), ChainMode::alone, the ctx option chain_no_iso}.
 * R_of[batch] = R of every matrix (read only where the launch carries right-hand-side items; may be NULL otherwise).
 * plan[24] = {np, j, nt (64-row tiles below the panel), nT (trailing tiles), nct (64-column tiles of the inverse), la_idx (the look-ahead workgroup, -1: none),
 *   the hand-over buffer of the diagonal blocks exists, this launch reads its block from it, leaves the next one in it, publishes block 0 into it,
 *   the launch carries right-hand-side items, rhs_p (the lagged panel they apply, -1: none), rhs_last (they make the last panel final too), rhs_nt (64-row
 *   tiles below the lagged panel), rhs_tpw (row tiles per workgroup, 1 or 2), row groups, rhs_nq (items per Lq_q), rhs_base (first right-hand-side
 *   workgroup), gx (workgroups per matrix; 0: one is launched all the same), iso_per, grid x, grid y, the grid is the XCD-isolated 1-D one, its workgroups}.
 * wgs (may be NULL: the plan only; else n_wgs == grid x * grid y) = [workgroup, blockIdx.y-major][8] = {matrix b, workgroup bx of its row (both -1: the
 *   workgroup exits at once), kind (0: exits at once, 1: trailing tile, 2: inverse tile, 3: look-ahead, 4: the diagonal block alone, 5: right-hand-side
 *   item), then for an inverse tile {row tile (-1: the panel's own rows), column tile}, for a right-hand-side item {q (== R: alpha), column tile ct, row
 *   group g, final_only, the first 64-row tile below the lagged panel that the group updates}, for a trailing tile {0, its number in the lower triangle};
 *   0 beyond}.
 * DCGP_ERR_ARG unless n_query == 8 and n_plan == 24, for a jp beyond the matrix and for right-hand sides without inv(L) or beyond Mp = 256. */
int dcgp_debug_plan_chain(const long long* query, int n_query, const long long* R_of, int n_R, long long* plan, int n_plan, long long* wgs, long n_wgs);
/* The factorisation chain exactly as a model step runs it, on caller buffers (device pointers unless said otherwise): a factor group filled as a model
 * fills one, its run() and finish().  A [batch][Mp][Mp] (Mp a multiple of 16, padded with the identity) is overwritten with the factors; Linv / LinvT
 * [batch][Mp][Mp] or NULL (Linv == NULL: a plain factor).  desc (host, NULL or [batch][7]) = per matrix {R, Rp, Lq, qmu, G, alpha, sums} with the five device
 * pointers as integers, 0 for none (csrc/common.h, ChainRhs: Lq [R][Mp][Mp], qmu / alpha [Mp][Rp], G [R][Mp][Mp], sums [R + 1][np (np + 1) / 2]).
 * flags: bit 0 ChainMode::alone, bit 1 ChainMode::may_ride, bit 2 defer_finish.  snap (host, NULL or [n_snap / 3][3] = {destination, source, bytes}): device
 * copies enqueued between run() and finish() of the first pass.  A_again (NULL or [batch][Mp][Mp]): the chain then runs a second time on the same group
 * with A overwritten by it.  info_host [batch], or [2][batch] with A_again: 0 or the 1-based column at which a matrix turned out not positive definite.
 * DCGP_ERR_ARG where a descriptor asks to ride and the mode or the ctx's options (no_rhs_ride) rule that out. */
int dcgp_debug_factor_chain(dcgp_ctx* ctx, double* A, double* Linv, double* LinvT, int batch, int Mp, const long long* desc, int n_desc, int flags,
                            const long long* snap, int n_snap, const double* A_again, int* info_host);
/* Head rows riding the layer kernel's persistent launch (csrc/fused_plan.h, plan_head_ride; ctx option head_ride, 0: never).
 * dcgp_debug_head_ride: out2 = {head rows the ctx's most recent layer-kernel launch carried (0: none), launches of the ctx that carried any}.
 * dcgp_debug_plan_head_ride (no ctx, no device): the decision for the launch that `query` (as above) is planned as and
 *   ride[8] = {next_is_head, head_form (the head's sweep is the reducing patch-row form), doubles of a head row, LDS bytes of the sweep's workgroup, its Z
 *   fragments, in_flight, chain_beside, the ctx option head_ride (-1: as many rows as the simulated deal's workgroups have room for before the last strip ends;
 *   k > 0: k rows, or all)};
 *   out[8] = {ok, why (0 rides, 1 option off, 2 the next layer is not the head, 3 another form of the sweep, 4 the launch cannot carry rows, 5 state is kept
 *   for a reverse pass, 6 trace on, 7 steps in flight / chain beside the main stream, 8 geometry, 9 no workgroup has room for a row), head rows that ride (the first so many),
 *   item of row 0, item of `row`, first and last
 *   strip whose samples are `row`, the latest item that writes any of them (-1 where it does not ride or `row` is out of range)}. */
int dcgp_debug_head_ride(dcgp_ctx* ctx, long long* out2);
int dcgp_debug_plan_head_ride(const long long* query, int n_query, const long long* ride, int n_ride, long long row, long long* out, int n_out);
/* The head's WHOLE sweep in that launch, so that no sweep launch follows it (csrc/fused_plan.h, plan_head_tail; ctx option head_ride_tail: -1 where the simulated
 * deal has it ahead, 0 never, 1 wherever the launch can carry it, 2 / 4 the same with that many sub-row items per row).  Behind the whole rows of plan_head_ride
 * the counter deals `parts` sub-row items per row that did not ride whole (the last of them also runs the row's Kdiag chunks), then one Kdiag item per row that did.
 * dcgp_debug_head_tail: out4 = {Kdiag items, sub-row items, parts of the ctx's most recent layer-kernel launch (0: it carried no tail), head sweep launches
 *   the ctx has skipped because a layer launch had run the whole sweep}.
 * dcgp_debug_plan_head_tail (no ctx, no device): query and ride as above, tail[2] = {the ctx option head_ride_tail, Kdiag slots per row of the sweep's plan};
 *   out[14] = {ok, why (0 rides, 1 option off, 2 plan_head_ride does not admit the launch, 3 geometry, 4 chosen only with a workgroup on every CU, 5 the simulated
 *   deal has no gain), whole rows in front, parts, Z-fragment units of a part, item of tail item 0, tail items, then of tail item `item`: its row, first and end
 *   unit, whether it runs the row's Kdiag chunks, first and last strip of the row, the latest item that writes samples of it (row -1 where `item` is out of range)}. */
int dcgp_debug_head_tail(dcgp_ctx* ctx, long long* out4);
int dcgp_debug_plan_head_tail(const long long* query, int n_query, const long long* ride, int n_ride, const long long* tail, int n_tail, long long item,
                              long long* out, int n_out);
/* The same for the patch sweeps (csrc/head_units.hip; tools/sweep_trace.py): [n_workgroups][waves per workgroup][8] int64 -- wall clock at entry,
 * shader clock at entry / image staged / set-up done / first unit done / last unit done, wall clock at exit, units run.            */
/* The ceilings bench.py prices kernels against, measured on this device (csrc/peaks.hip): the sustained fp64 MFMA rate (TFLOP/s, 4 waves
 * per SIMD, ~85 ms) and the rate of a pure store sweep writing an [M x N*P] matrix in the K_uf sweep's tile pattern (GB/s).            */
int dcgp_debug_mfma_f64_rate(dcgp_ctx* ctx, double* tflops_out);
int dcgp_debug_store_rate(dcgp_ctx* ctx, int N, int P, int M, double* gbs_out);
int dcgp_debug_set_sweep_trace(dcgp_ctx* ctx, long long* buf_dev, long n_workgroups, const char* family /* "kuf", "kuf_long", "head_sweep"; NULL: any */);
/* The three kernels of a filter mean (csrc/conv_mean.hip; dcgp_model_set_mean_filter) alone, on a conv layer H x W x C with filter f, `stride`, R maps,
 * `rows` images and `rep` replicas of its output, each beside a copy kernel moving the bytes the kernel has to move (tools/conv_mean_time.py): `iters`
 * launches between two events behind a warm-up.  out_us[8] = microseconds per launch {conv_mean_add, its copy, conv_mean_backward_dx, its copy,
 * conv_mean_backward_filter (both stages), its copy, 0, 0}. */
int dcgp_debug_conv_mean_time(dcgp_ctx* ctx, int H, int W, int C, int f, int stride, int R, int rows, int rep, int iters, double* out_us);

/* The three kernels of a mixing (csrc/mix.hip) alone on Kc columns, G latent GPs, R maps, each beside a copy kernel moving the bytes the kernel has to
 * move (tools/mixing_time.py).  out_us[8] = microseconds per launch {mix_forward, its copy, mix_backward_latent, its copy, mix_backward_w (both
 * stages), its copy, 0, 0}. */
int dcgp_debug_mix_time(dcgp_ctx* ctx, int G, int R, long Kc, int iters, double* out_us);

/* The two relayout kernels of a dilated layer (csrc/dilate.hip; dcgp_model_set_dilation) alone on `rows` images H x W x C at rate d, each beside the
 * same relayout walking its source instead of its destination and beside a copy kernel of the same traffic (tools/dilation_time.py).  out_us[8] =
 * microseconds per launch {space-to-batch, the same from the image's side (a memset plus a scatter), a copy of the phase batch's size,
 * batch-to-space, the same from the phase side, a copy of the image batch's size, 0, 0}. */
int dcgp_debug_dilate_time(dcgp_ctx* ctx, int rows, int H, int W, int C, int d, int iters, double* out_us);

#ifdef __cplusplus
}
#endif
#endif /* DCGP_H */

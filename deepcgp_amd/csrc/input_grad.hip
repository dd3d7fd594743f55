// input_grad.hip -- the gradient of a per-image objective with respect to the input pixels (saliency maps, adversarial examples).
// The reference gets it from tf.gradients on the graph of DGP_Base.predict_density / _build_likelihood; here it is
//   a forward pass that keeps the layer outputs and K_uf / A1 (forward_data_impl, model.hip: an evaluation's forward, factor reuse included),
//   the objective's tail adjoint -- (gm, gv) = dJ / d(mean, var) of the head's rows [S N][K], row s N + n --
//   and the DATA PATH of the reverse pass down to and including layer 0 (model_backward_data, grad.hip).
// Objectives, per image n (the layers treat images independently, so row n of the result is dJ_n / dX_n):
//   density  J_n = log(1/S sum_s p(y_n | mean_sn, var_sn))      -- dcgp_model_predict_density's value; RobustMax, Softmax (softmax.hip)
//   elbo     J_n = 1/S sum_s E_q[log p(y_n | f_sn)]             -- the image's share of the ELBO's data term, unscaled; every likelihood
// RobustMax: p = (1 - eps) P + eps / (K - 1) (1 - P) and E_q[log p] = log(1 - eps) P + log(eps / (K - 1)) (1 - P) are both affine in the
// Gauss-Hermite probability P that the label's output is the largest, so both tails are dP / d(mean, var) (robustmax_grad_kernel's terms, grad.hip)
// times a per-row factor: c / S for the variational expectation, (1 - eps - eps / (K - 1)) / (S pbar_n) for the density, where pbar_n needs all S
// rows of the image first -- rm_density_grad_kernel, one workgroup per image.
// Nothing here writes a parameter, a gradient block, an Adam moment or param_version; no atomics: two calls give the same bits.
#include "model_state.h"
#include "tail_dev.h"

namespace {

inline unsigned blocks_for(long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

// ys[i] = y[i] clamped into [0, K); bad[0] = number of labels outside (one workgroup; the kernels behind it index with ys)
__global__ __launch_bounds__(256) void labels_clamp_kernel(const int32_t* __restrict__ y, int n, int K, int32_t* __restrict__ ys, int* __restrict__ bad) {
  __shared__ int cnt[256];
  int c = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int v = y[i];
    const bool out = v < 0 || v >= K;
    c += out ? 1 : 0;
    ys[i] = out ? 0 : v;
  }
  cnt[threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) cnt[threadIdx.x] += cnt[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) bad[0] = cnt[0];
}

// The density objective's tail for RobustMax.  One workgroup per image n; rows s n_img + n, s < S.  Pass over the S rows in groups of DR_ROWS: thread
// (row slot, node g) evaluates node g's terms of P and of dP / d(mean_k, var_k) for every class into LDS (robustmax_grad_kernel's arithmetic, the
// same clips), thread (row slot, k) adds the 20 nodes in a fixed order and stores the UNSCALED derivative; p_s = (1 - eps) P_s + eps / (K - 1) (1 - P_s)
// stays in LDS.  Then pbar_n = 1/S sum_s p_s (s = 0, 1, ...), J[n] = log pbar_n, and the workgroup rescales the rows it wrote by
// (1 - eps - eps / (K - 1)) / (S pbar_n).
constexpr int DR_ROWS = 12, DR_KMAX = kRmDensityMaxK;
__global__ __launch_bounds__(256) void rm_density_grad_kernel(const double* __restrict__ mu, const double* __restrict__ var, const int32_t* __restrict__ y,
                                                              int n_img, int S, int K, double eps, const double* __restrict__ gh,
                                                              double* __restrict__ J, double* __restrict__ gm, double* __restrict__ gv) {
  __shared__ double tm[DR_ROWS][20][DR_KMAX], tv[DR_ROWS][20][DR_KMAX], tp[DR_ROWS][20];
  extern __shared__ double ps[];   // [S]
  __shared__ double coef;
  const int n = blockIdx.x, t = threadIdx.x, lr = t / 20, g = t % 20;
  const int lab = y[n];
  const double inv_sqrt_pi = 0.56418958354775628695, inv_sqrt_2pi = 0.39894228040143267794;
  for (int s0 = 0; s0 < S; s0 += DR_ROWS) {
    const int s = s0 + lr;
    if (lr < DR_ROWS && s < S) {
      const long row = (long)s * n_img + n;
      const double* m = mu + row * K;
      const double* v = var + row * K;
      const double vy = v[lab];
      const bool live_y = 2.0 * vy > 1e-10;
      const double sy = sqrt(fmax(2.0 * vy, 1e-10));
      const double xg = gh[g], wg = gh[20 + g] * inv_sqrt_pi;
      const double X = m[lab] + xg * sy;
      double prod = 1.0;
      for (int k = 0; k < K; ++k) {
        if (k == lab) continue;
        const double d = (X - m[k]) / sqrt(fmax(v[k], 1e-10));
        prod *= 0.5 * (1.0 + erf(d * 0.70710678118654752440)) * (1.0 - 2e-4) + 1e-4;
      }
      double qs = 0.0;
      for (int k = 0; k < K; ++k) {
        if (k == lab) continue;
        const double sig = sqrt(fmax(v[k], 1e-10));
        const double d = (X - m[k]) / sig;
        const double cdf = 0.5 * (1.0 + erf(d * 0.70710678118654752440)) * (1.0 - 2e-4) + 1e-4;
        const double q = wg * prod / cdf * exp(-0.5 * d * d) * inv_sqrt_2pi * (1.0 - 2e-4);
        tm[lr][g][k] = -q / sig;
        tv[lr][g][k] = v[k] > 1e-10 ? -q * d / (2.0 * v[k]) : 0.0;
        qs += q / sig;
      }
      tm[lr][g][lab] = qs;
      tv[lr][g][lab] = live_y ? qs * xg / sy : 0.0;
      tp[lr][g] = prod * wg;
    }
    __syncthreads();
    for (int idx = t; idx < DR_ROWS * K; idx += 256) {
      const int r2 = idx / K, k = idx % K, s2 = s0 + r2;
      if (s2 >= S) continue;
      double a = 0.0, b = 0.0;
      for (int gg = 0; gg < 20; ++gg) { a += tm[r2][gg][k]; b += tv[r2][gg][k]; }
      const long row = (long)s2 * n_img + n;
      gm[row * K + k] = a;
      gv[row * K + k] = b;
      if (k == 0) {
        double P = 0.0;
        for (int gg = 0; gg < 20; ++gg) P += tp[r2][gg];
        ps[s2] = P * (1.0 - eps) + (1.0 - P) * (eps / (K - 1.0));
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += ps[s];
    const double pbar = acc / (double)S;
    if (J) J[n] = log(pbar);
    coef = (1.0 - eps - eps / (K - 1.0)) / ((double)S * pbar);
  }
  __syncthreads();   // (also orders this workgroup's own stores to gm / gv in front of the loads below)
  const double c = coef;
  for (int idx = t; idx < S * K; idx += 256) {
    const long o = ((long)(idx / K) * n_img + n) * K + idx % K;
    gm[o] *= c;
    gv[o] *= c;
  }
}

// J[n] = 1/S sum_s ve[s n_img + n]
__global__ void sample_mean_rows_kernel(const double* __restrict__ ve, int S, int n_img, double* __restrict__ J) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_img) return;
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc += ve[(long)s * n_img + n];
  J[n] = acc / (double)S;
}

// res[0] = first non-positive pivot of the factorisations the forward used (0: none), res[1] = labels outside [0, K)
__global__ void ig_status_kernel(FactorStatus st, const int* __restrict__ bad, double* __restrict__ res) {
  if (blockIdx.x || threadIdx.x) return;
  const int pivot = first_bad_pivot(st);
  res[0] = (double)pivot;
  res[1] = bad ? (double)bad[0] : 0.0;
}

}  // namespace

// ---- the patch adjoint fused with its scatter ---------------------------------------------------------------------------------------------------
// dX of a scalar-lengthscale RBF patch layer from E = dK o K [M][ld] (column n P + p) and cs = its column sums:
//   dX[n] = fold_p( (sum_m E[m][n P + p] Z[m][:] - cs[n P + p] x_np) / l^2 (+ extra[n P + p][:]) ),   x_np the patch p of image n.
// One workgroup of four waves per image row.  The product runs on v_mfma_f64_16x16x4_f64: a wave owns the 16-patch tiles w, w + 4, ... of the
// image (TPW of them) and every 16-wide tile of the patch length (NL), accumulators in registers; E is read once, straight into the A operand
// (lane = (patch lcol, m lrow): 16 consecutive columns of a row of E per quarter wave); Z goes through LDS in chunks of 16 rows shared by the
// four waves.  The image sits in LDS: the correction cs o x reads the pixel a patch element came from (patches are never materialised), and the
// overlapping patches are folded into an H W C tile in LDS in f * f ordered phases -- within phase (kh, kw) distinct (patch, channel) pairs hit
// distinct pixels, so plain LDS adds behind a barrier per phase are free of conflicts and their order is fixed.  Each pixel is stored once.
// Result fragment of the MFMA: acc[v] = D[row lrow + 4 v][col lcol] (rows = patches, columns = patch elements).
namespace {
struct PaArgs {
  const double* E; long ld; const double* cs; const double* Z; const double* X; const double* extra; double* dX;
  int M, L, P, Wo, H, W, C, f, s, n_mod; double inv_l2;
};
constexpr int PA_MC = 16;
template <int NL, int TPW>
__global__ __launch_bounds__(256) void patch_adjoint_fused_kernel(PaArgs a) {
  extern __shared__ double pa_sm[];
  constexpr int ZLD = 16 * NL + 4;
  const int HWC = a.H * a.W * a.C;
  double* Xs = pa_sm;
  double* dXs = pa_sm + HWC;
  double* Zs = pa_sm + 2 * HWC;   // [PA_MC][ZLD]
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lcol = lane & 15, lrow = lane >> 4;
  const double* __restrict__ img = a.X + (long)(n % a.n_mod) * HWC;
  for (int i = tid; i < HWC; i += 256) { Xs[i] = img[i]; dXs[i] = 0.0; }
  const long c0 = (long)n * a.P;
  d4 acc[TPW][NL];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int y = 0; y < NL; ++y) acc[t][y] = d4{0.0, 0.0, 0.0, 0.0};
  for (int m0 = 0; m0 < a.M; m0 += PA_MC) {
    double av[PA_MC / 4][TPW];
#pragma unroll
    for (int k4 = 0; k4 < PA_MC / 4; ++k4)
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int m = m0 + 4 * k4 + lrow, p = 16 * (w + 4 * t) + lcol;
        av[k4][t] = (m < a.M && p < a.P) ? a.E[(long)m * a.ld + c0 + p] : 0.0;
      }
    __syncthreads();   // the previous chunk of Z is used up
    for (int idx = tid; idx < PA_MC * 16 * NL; idx += 256) {
      const int r = idx / (16 * NL), l = idx - r * (16 * NL), m = m0 + r;
      Zs[r * ZLD + l] = (m < a.M && l < a.L) ? a.Z[(long)m * a.L + l] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k4 = 0; k4 < PA_MC / 4; ++k4) {
      double b[NL];
#pragma unroll
      for (int y = 0; y < NL; ++y) b[y] = Zs[(4 * k4 + lrow) * ZLD + 16 * y + lcol];
#pragma unroll
      for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int y = 0; y < NL; ++y) acc[t][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[k4][t], b[y], acc[t][y], 0, 0, 0);
    }
  }
  // this lane's patch elements l = 16 y + lcol: phase (kh f + kw) and channel; -1 beyond the patch length
  int lph[NL], lch[NL];
#pragma unroll
  for (int y = 0; y < NL; ++y) {
    const int l = 16 * y + lcol;
    lph[y] = l < a.L ? l / a.C : -1;
    lch[y] = l % a.C;
  }
  // (sum - cs o x) / l^2 (+ extra) in place
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int p = 16 * (w + 4 * t) + lrow + 4 * v;
      if (p >= a.P) continue;
      const int oh = p / a.Wo, ow = p - oh * a.Wo;
      const double csv = a.cs[c0 + p];
#pragma unroll
      for (int y = 0; y < NL; ++y) {
        if (lph[y] < 0) continue;
        const int kh = lph[y] / a.f, kw = lph[y] - kh * a.f;
        const int pix = ((oh * a.s + kh) * a.W + ow * a.s + kw) * a.C + lch[y];
        double val = a.inv_l2 * (acc[t][y][v] - csv * Xs[pix]);
        if (a.extra) val += a.extra[(c0 + p) * a.L + 16 * y + lcol];
        acc[t][y][v] = val;
      }
    }
  // the fold: one phase per (kh, kw)
  const int phases = a.f * a.f;
  for (int ph = 0; ph < phases; ++ph) {
    const int kh = ph / a.f, kw = ph - kh * a.f;
#pragma unroll
    for (int y = 0; y < NL; ++y) {
      if (lph[y] != ph) continue;
#pragma unroll
      for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int p = 16 * (w + 4 * t) + lrow + 4 * v;
          if (p >= a.P) continue;
          const int oh = p / a.Wo, ow = p - oh * a.Wo;
          dXs[((oh * a.s + kh) * a.W + ow * a.s + kw) * a.C + lch[y]] += acc[t][y][v];
        }
    }
    __syncthreads();
  }
  double* __restrict__ out = a.dX + (long)n * HWC;
  for (int i = tid; i < HWC; i += 256) out[i] = dXs[i];
}

template <int NL, int TPW>
int pa_launch(dcgp_ctx* ctx, const PaArgs& a, int rows, size_t lds) {
  ScopedTimer tm(ctx, "patch_adjoint_fused");
  hipLaunchKernelGGL((patch_adjoint_fused_kernel<NL, TPW>), dim3((unsigned)rows), dim3(256), lds, ctx->stream, a);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}
// the instantiation for (tiles of the patch length, patch tiles per wave), or 0: (2,3) up to 32 patch elements of up to 192 patches per image (cfg2's
// first layer), (4,3) up to 64 elements.  Measured and dropped: (16,1) for cfg2's head (250 elements, 64 patches) -- 365 us against 138
// for the product + col2im pair; one workgroup per image also leaves most of the chip idle under 256 rows, so those go through the pair as well
constexpr long PA_MIN_ROWS = 256;
int pa_pick(int nl, int tpw) {
  if (nl <= 2 && tpw <= 3) return 1;
  if (nl <= 4 && tpw <= 3) return 2;
  return 0;
}
size_t pa_lds(const LayerState& L, int which) {
  const int nl = which == 1 ? 2 : 4;
  return ((size_t)2 * L.v.H * L.v.W * L.v.C + (size_t)PA_MC * (16 * nl + 4)) * sizeof(double);
}
}  // namespace

bool patch_adjoint_fused_ok(const LayerState& L, long rows) {
  if (L.base_type != 0 || L.in_scale || rows < PA_MIN_ROWS || rows > 0x7fffffffL || rows * L.v.P > 0x7fffffffL) return false;
  const int which = pa_pick((L.v.L + 15) / 16, ((L.v.P + 15) / 16 + 3) / 4);
  return which != 0 && pa_lds(L, which) <= 65536;
}

int patch_adjoint_fused(dcgp_ctx* ctx, const LayerState& L, const double* E, long ld, const double* cs, const double* Xin, int rows, int n_mod,
                        const double* extra, double* dXin) {
  if (!patch_adjoint_fused_ok(L, rows)) return ctx_fail(ctx, DCGP_ERR_ARG, "patch_adjoint_fused: shape not covered");
  const int which = pa_pick((L.v.L + 15) / 16, ((L.v.P + 15) / 16 + 3) / 4);
  PaArgs a;
  a.E = E; a.ld = ld; a.cs = cs; a.Z = L.Z; a.X = Xin; a.extra = extra; a.dX = dXin;
  a.M = L.M; a.L = L.v.L; a.P = L.v.P; a.Wo = L.v.Wo; a.H = L.v.H; a.W = L.v.W; a.C = L.v.C; a.f = L.v.f; a.s = L.v.s; a.n_mod = n_mod;
  a.inv_l2 = 1.0 / (L.ls * L.ls);
  const size_t lds = pa_lds(L, which);
  switch (which) {
    case 1: return pa_launch<2, 3>(ctx, a, rows, lds);
    default: return pa_launch<4, 3>(ctx, a, rows, lds);
  }
}

int rm_density_grad(dcgp_ctx* ctx, const double* mu, const double* var, const int32_t* y, int n_img, int S, int K, double eps, double* J, double* gm,
                    double* gv) {
  const double* gh = gauss_hermite_table(ctx);
  if (!gh) return DCGP_ERR_ALLOC;
  if (S > 256) return   // (static LDS of the kernel + S doubles within 64 KiB)
    ctx_fail(ctx, DCGP_ERR_ARG, "input_grad: S = %d samples exceed the tail's LDS", S);
  hipLaunchKernelGGL(rm_density_grad_kernel, dim3((unsigned)n_img), dim3(256), (size_t)S * sizeof(double), ctx->stream, mu, var, y, n_img, S, K, eps, gh, J,
                     gm, gv);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

namespace {

int input_grad_run(dcgp_model* model, const double* X, const int32_t* y, const double* yf, int N, int S, const double* const* zs, uint64_t seed,
                   int objective, double* out_value, double* out_dX, int* info_host, const char* who) {
  if (!model) return DCGP_ERR_ARG;
  dcgp_ctx* ctx = model->ctx;
  if (info_host) *info_host = 0;
  const int obj = objective & 0xff, dedup = (objective & DCGP_INPUT_GRAD_DEDUP) ? 1 : 0;
  if (!X || !(y || yf) || N <= 0 || S <= 0 || !out_dX) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: bad args (N %d, S %d)", who, N, S);
  if ((objective & ~(0xff | DCGP_INPUT_GRAD_DEDUP)) || (obj != DCGP_OBJECTIVE_DENSITY && obj != DCGP_OBJECTIVE_ELBO))
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: objective %d (0 density, 1 elbo)", who, objective);
  if (!model->has_head) return ctx_fail(ctx, DCGP_ERR_ARG, "model has no head layer");
  const int nl = (int)model->layers.size();
  const int K = model->layers[nl - 1]->R;
  const Likelihood lik = model->lik();
  DCGP_TRY(lik_check_targets(ctx, lik, Targets::of(y, yf, K), who));
  if (yf && obj == DCGP_OBJECTIVE_DENSITY)
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: the density objective exists for the RobustMax and Softmax likelihoods only; a Gaussian or Bernoulli model takes the elbo objective", who);
  if (model->enq_seq != model->col_seq) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: enqueued steps are still to be collected", who);
  if (!yf && (K < 2 || K > lik_density_max_k(lik))) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: %d classes (2 to %d)", who, K, lik_density_max_k(lik));
  const std::string mp = "m" + std::to_string(model->id) + "_";
  double* res = (double*)ws_get(ctx, mp + "ig_res", 2 * sizeof(double));
  int* bad = (int*)ws_get(ctx, mp + "ig_bad", sizeof(int));
  int32_t* ys = y ? (int32_t*)ws_get(ctx, mp + "ig_y", (size_t)N * sizeof(int32_t)) : nullptr;
  if (!res || !bad || (y && !ys)) return DCGP_ERR_ALLOC;

  // the forward pass, with what the reverse pass reads left behind; the model's flags are put back whichever way this ends
  struct Flags {
    dcgp_model* m; bool ko, ks, dg;
    explicit Flags(dcgp_model* mm) : m(mm), ko(mm->keep_outputs), ks(mm->keep_state), dg(mm->data_grad) { m->keep_outputs = m->keep_state = m->data_grad = true; }
    ~Flags() { m->keep_outputs = ko; m->keep_state = ks; m->data_grad = dg; }
  } flags(model);
  int rows = 0;
  int rc = forward_data_impl(model, X, N, S, zs, seed, dedup, &rows);
  auto run = [&]() -> int {
    const auto& o = model->outs[nl - 1];
    if (rows <= 0 || rows % N || o.width != K) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: head rows %d x %d for %d images", who, rows, o.width, N);
    const int Sh = rows / N;   // S, or 1: a head-only model under dedup_layer0 has one row per image (its S samples are identical)
    double* gm = (double*)ws_get(ctx, mp + "g_gm_head", (size_t)rows * K * sizeof(double));
    double* gv = (double*)ws_get(ctx, mp + "g_gv_head", (size_t)rows * K * sizeof(double));
    double* J = out_value ? out_value : (double*)ws_get(ctx, mp + "ig_J", (size_t)N * sizeof(double));
    if (!gm || !gv || !J) return DCGP_ERR_ALLOC;
    if (y) {
      hipLaunchKernelGGL(labels_clamp_kernel, dim3(1), dim3(256), 0, ctx->stream, y, N, K, ys, bad);
      LAUNCH_CHECK(ctx);
    }
    if (obj == DCGP_OBJECTIVE_DENSITY) {
      DCGP_TRY(lik_density_grad(ctx, lik, o.mean, o.var, ys, N, Sh, K, J, gm, gv));
    } else {
      // the variational expectations of the rows (the ELBO step's tail launch without its assembly), their mean per image, and the step's own seeds
      double* ve = (double*)ws_get(ctx, mp + "ig_ve", (size_t)rows * sizeof(double));
      double* scal = (double*)ws_get(ctx, mp + "ig_scal", 64 * sizeof(double));
      if (!ve || !scal) return DCGP_ERR_ALLOC;
      const double w = 1.0 / Sh;
      const Targets t = Targets::of(ys, yf, K);   // (labels: the clamped copy)
      double* gs2 = lik.n_params() ? (double*)ws_get(ctx, mp + "ig_gs2", sizeof(double)) : nullptr;   // (the variance's gradient: not reported)
      DCGP_TRY(lik_elbo_tail(ctx, lik, o.mean, o.var, t, rows, N, K, ve, w, scal, ElboFinish()));
      DCGP_TRY(lik_grad_seeds(ctx, lik, o.mean, o.var, t, rows, N, K, w, gm, gv, gs2));
      hipLaunchKernelGGL(sample_mean_rows_kernel, dim3(blocks_for(N)), dim3(256), 0, ctx->stream, ve, Sh, N, J);
      LAUNCH_CHECK(ctx);
    }
    DCGP_TRY(model_backward_data(model, X, N, S, dedup, gm, gv, out_dX));
    FactorStatus st;
    DCGP_TRY(fill_status(model, &st));
    hipLaunchKernelGGL(ig_status_kernel, dim3(1), dim3(64), 0, ctx->stream, st, y ? bad : nullptr, res);
    LAUNCH_CHECK(ctx);
    return DCGP_OK;
  };
  if (rc == DCGP_OK) rc = run();
  double h[2] = {0.0, 0.0};
  if (rc == DCGP_OK && hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = ctx_fail(ctx, DCGP_ERR_HIP, "%s: read-back failed", who);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == DCGP_OK) rc = ctx_fail(ctx, DCGP_ERR_HIP, "%s: the stream failed", who);
  DCGP_TRY(rc);
  if (h[1] > 0) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: %d labels outside [0, %d)", who, (int)h[1], K);
  const int pivot = (int)h[0];
  if (info_host) *info_host = pivot;
  if (pivot) return ctx_fail(ctx, DCGP_ERR_NOT_PD, "Cholesky: matrix not positive definite at column %d", pivot);
  return DCGP_OK;
}

}  // namespace

extern "C" {

int dcgp_model_input_grad(dcgp_model* model, const double* X, const int32_t* y, int N, int S, const double* const* z_per_layer, uint64_t seed,
                          int objective, double* out_value, double* out_dX, int* info_host) {
  return input_grad_run(model, X, y, nullptr, N, S, z_per_layer, seed, objective, out_value, out_dX, info_host, "input_grad");
}

int dcgp_model_input_grad_f64y(dcgp_model* model, const double* X, const double* y, int N, int S, const double* const* z_per_layer, uint64_t seed,
                               int objective, double* out_value, double* out_dX, int* info_host) {
  return input_grad_run(model, X, nullptr, y, N, S, z_per_layer, seed, objective, out_value, out_dX, info_host, "input_grad_f64y");
}

}  // extern "C"

// transfer.hip -- moving a layer's q(u) to a new set of inducing inputs: the projection q'(u') = int p(u' | u) q(u) du of q(u) = N(m, S_r = Lq_r Lq_r^T)
// at Z onto Z', and the cross Gram matrix k(A, B) it is built from.  With K = k(Z, Z) + j I = L L^T, Kc = k(Z, Z'), Kn = k(Z', Z') + j I = L' L'^T:
//   B = inv(L) Kc,  P = inv(L)^T B  (M x M'),   m' = P^T m,   T_r = Lq_r^T P,   S'_r = Kn - B^T B + T_r^T T_r,   Lq'_r = chol(S'_r).
// u and u' carry INDEPENDENT jitter: the joint prior [[K + jI, Kc], [Kc^T, Kn + jI]] is positive definite, Kn - B^T B keeps its smallest eigenvalue
// near 2 j, and chol(S'_r) succeeds however small Lq_r is (a conv layer starts at 1e-5).  The price: a transfer onto the SAME Z is a projection, not
// the identity (Kc's diagonal has no jitter).  white: m, Lq arrive and leave in whitened coordinates (m = L m_w, Lq = L Lq_w in; inv(L') of both out).
//
// Launch structure: everything on the ctx's stream -- the two Gram matrices as dcgp_kuu_* form them (rbf_gram_padded), the cross Gram kernel below,
// the factorisation chain of chol_fused.hip on K and Kn (factor + inverse), the batched potrf of chol.hip on the S'_r, the products through gemm_gen
// (fp64 MFMA; k-splits summed in a fixed order).  No atomics: a call gives the same bits every run.  The results are formed in scratch; the two commit
// kernels at the end read the status word ON THE DEVICE and copy to the caller's buffers only when every factorisation succeeded, so the one host
// synchronisation of a call is the read of that status word.
#include <cmath>

#include "model_state.h"
#include "gemm_gen.h"

namespace {

constexpr int TR_MAX_M = 1024, TR_MAX_R = 64, TR_MAX_L = 4096;

inline unsigned nblk(long n) { return (unsigned)((n + 255) / 256); }

// out[i][j] = k(a_i, b_j), 32 x 32 tile per 256-thread block, rows staged through LDS 32 elements at a time (ard: divided by the lengthscales on the
// way in).  Plain fused multiply-adds, not the matrix pipe, on purpose: x.z, |x|^2 and |z|^2 are accumulated by the SAME chain over l, as
// rbf_gram_kernel does, so that on coincident rows all three are the same bits -- the distance is then an exact 0 and the ArcCosine's cosine an exact
// 1 (one ulp of the cosine there moves the entry by ~1e-9 variance).  Every entry goes through BaseKernel::eval, the off-diagonal form: no jitter, no
// eval_diag, also where b_j == a_i.
__global__ __launch_bounds__(256) void cross_gram_kernel(const double* __restrict__ A, long m, const double* __restrict__ B, long n, int d,
                                                         BaseKernel bk, const double* __restrict__ ard, double* __restrict__ out, long ldo) {
  __shared__ double Ai[32][33], Bj[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const long i0 = (long)blockIdx.y * 32, j0 = (long)blockIdx.x * 32;
  double dot[4] = {0, 0, 0, 0}, ni[4] = {0, 0, 0, 0}, nj = 0.0;
  for (int l0 = 0; l0 < d; l0 += 32) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < 32 * 32; idx += 256) {
      const int r = idx >> 5, c = idx & 31;
      const bool in_l = l0 + c < d;
      const double s = (ard && in_l) ? ard[l0 + c] : 1.0;
      double a = (i0 + r < m && in_l) ? A[(i0 + r) * d + l0 + c] : 0.0;
      double b = (j0 + r < n && in_l) ? B[(j0 + r) * d + l0 + c] : 0.0;
      if (ard) { a /= s; b /= s; }
      Ai[r][c] = a;
      Bj[r][c] = b;
    }
    __syncthreads();
#pragma unroll 8
    for (int l = 0; l < 32; ++l) {
      const double b = Bj[tx][l];
      nj = fma(b, b, nj);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double a = Ai[ty + 8 * q][l];
        dot[q] = fma(a, b, dot[q]);
        ni[q] = fma(a, a, ni[q]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long i = i0 + ty + 8 * q, j = j0 + tx;
    if (i < m && j < n) out[i * ldo + j] = bk.eval(dot[q], ni[q], nj);
  }
}

// out[i][l] = Z[i][l] / lengthscale_l: the rows dcgp_kuu_rbf is given for an ARD kernel
__global__ void tr_scale_rows_kernel(const double* __restrict__ Z, long total, int d, const double* __restrict__ ard, double* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) out[i] = Z[i] / ard[i % d];
}

// S_r <- sym(Kn - B^T B + T_r^T T_r) on the Mn x Mn block (S_r arrives holding T_r^T T_r), identity on the padding; one lane per entry on or below the
// diagonal, which also writes its mirror image.  grid (ceil(Np / 256), Np, R)
__global__ void tr_assemble_kernel(const double* __restrict__ Kn, const double* __restrict__ BB, double* __restrict__ S, int Mn, int Np) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= Np || j > i) return;
  double* Sr = S + (long)blockIdx.z * Np * Np;
  double v;
  if (i < Mn) {   // (j <= i)
    const double bb = 0.5 * (BB[(long)i * Mn + j] + BB[(long)j * Mn + i]);
    const double tt = 0.5 * (Sr[(long)i * Np + j] + Sr[(long)j * Np + i]);
    v = (Kn[(long)i * Np + j] - bb) + tt;
  } else {
    v = i == j ? 1.0 : 0.0;
  }
  Sr[(long)i * Np + j] = v;
  Sr[(long)j * Np + i] = v;
}

// status[0] = 0, or which matrix was not positive definite: 1 K, 2 Kn, 3 + r S'_r (the first of them); status[1] = its 1-based failing column
__global__ void tr_status_kernel(const int* __restrict__ infoK, const int* __restrict__ infoKn, const int* __restrict__ infoS, int R,
                                 int* __restrict__ status) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int which = 0, col = 0;
  if (infoK[0]) { which = 1; col = infoK[0]; }
  else if (infoKn[0]) { which = 2; col = infoKn[0]; }
  else
    for (int r = 0; r < R; ++r)
      if (infoS[r]) { which = 3 + r; col = infoS[r]; break; }
  status[0] = which;
  status[1] = col;
}

// the two commits: nothing is written unless the status word is 0.
// q_sqrt'[r][i][j] = src_r[i][j] on and below the diagonal, an exact 0 above it.  grid (ceil(Mn / 256), Mn, R)
__global__ void tr_commit_tril_kernel(const int* __restrict__ status, const double* __restrict__ src, int ld, long bs, int Mn, double* __restrict__ out) {
  if (status[0] != 0) return;
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= Mn) return;
  out[((long)blockIdx.z * Mn + i) * Mn + j] = j <= i ? src[(long)blockIdx.z * bs + (long)i * ld + j] : 0.0;
}
__global__ void tr_commit_copy_kernel(const int* __restrict__ status, const double* __restrict__ src, long total, double* __restrict__ out) {
  if (status[0] != 0) return;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) out[i] = src[i];
}

GenGemm mk(const double* A, long ars, long acs, long abs_, const double* B, long brs, long bcs, long bbs, double* C, long crs, long cbs, int M, int N,
           int K, int batch) {
  GenGemm g;
  g.A = A; g.a_rs = ars; g.a_cs = acs; g.a_bs = abs_; g.B = B; g.b_rs = brs; g.b_cs = bcs; g.b_bs = bbs;
  g.C = C; g.c_rs = crs; g.c_bs = cbs; g.M = M; g.N = N; g.K = K; g.batch = batch;
  return g;
}

// device buffers and pointer tables of one call: freed on every way out (the caller has synchronised the stream by then)
struct TrScratch {
  dcgp_ctx* ctx;
  std::vector<void*> ptrs;
  FactorGroup fK, fKn, fS;
  explicit TrScratch(dcgp_ctx* c) : ctx(c) {}
  ~TrScratch() {
    fK.release(); fKn.release(); fS.release();
    for (void* p : ptrs) dev_free(ctx, p);
  }
  double* get(size_t doubles, const char* label) {
    void* p = nullptr;
    if (dev_alloc(ctx, &p, (doubles ? doubles : 1) * sizeof(double), label) != hipSuccess) {
      ctx_fail(ctx, DCGP_ERR_ALLOC, "inducing_transfer: allocation of %zu doubles ('%s') failed", doubles, label);
      return nullptr;
    }
    ptrs.push_back(p);
    return (double*)p;
  }
};

int kernel_args(dcgp_ctx* ctx, const char* who, int kernel_type, double variance, double p1, double p2, const double* ard, BaseKernel* bk) {
  if (kernel_type < 0 || kernel_type > 3)
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: unknown kernel_type %d (0 rbf, 1 acos, 2 matern32, 3 matern52)", who, kernel_type);
  if (ard && kernel_type != 0) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: ard_lengthscales go with kernel_type 0 (rbf), got %d", who, kernel_type);
  if (!(variance > 0.0 && std::isfinite(variance))) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: variance must be positive, got %g", who, variance);
  if (!(p1 > 0.0 && std::isfinite(p1)))
    return ctx_fail(ctx, DCGP_ERR_ARG, "%s: p1 (%s) must be positive, got %g", who, kernel_type == 1 ? "weight variance" : "lengthscale", p1);
  if (kernel_type == 1 && !(p2 >= 0.0 && std::isfinite(p2))) return ctx_fail(ctx, DCGP_ERR_ARG, "%s: p2 (bias variance) must not be negative, got %g", who, p2);
  bk->type = kernel_type; bk->variance = variance; bk->p2 = 0.0;
  if (kernel_type == 1) { bk->p1 = p1; bk->p2 = p2; }
  else bk->p1 = ard ? 1.0 : 1.0 / (p1 * p1);   // ARD: the rows are divided by the lengthscales, the unit-lengthscale kernel evaluated (gpflow's form)
  return DCGP_OK;
}

int cross_gram_enqueue(dcgp_ctx* ctx, const double* A, long m, const double* B, long n, int d, const BaseKernel& bk, const double* ard, double* out) {
  ScopedTimer t(ctx, "cross_gram");
  hipLaunchKernelGGL(cross_gram_kernel, dim3((unsigned)((n + 31) / 32), (unsigned)((m + 31) / 32)), dim3(256), 0, ctx->stream, A, m, B, n, d, bk, ard,
                     out, n);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

struct TrCall {
  const double *Z, *Zn, *ard, *q_mu, *q_sqrt;
  double *out_q_mu, *out_q_sqrt;
  int M, Mn, L, R, white;
  double jitter;
  BaseKernel bk;
};

// one matrix through the factorisation chain: factor over A, inverse and its transpose beside it
int chain_one(dcgp_ctx* ctx, FactorGroup& fg, double* A, double* Ainv, double* AinvT, int Mp) {
  fg.Mp = Mp;
  fg.K = {A}; fg.Linv = {Ainv}; fg.LinvT = {AinvT};
  DCGP_TRY(fg.upload(ctx));
  HIP_TRY(ctx, hipMemsetAsync(fg.d_info, 0, sizeof(int), ctx->stream));
  return factor_inverse_batched(ctx, fg.dK, fg.dLinv, fg.dLinvT, 1, Mp, Mp, fg.d_info);
}

int transfer_enqueue(dcgp_ctx* ctx, const TrCall& c, TrScratch& s, int** status_out) {
  const int M = c.M, Mn = c.Mn, L = c.L, R = c.R;
  const int Mp = round_up(M, 16), Np = round_up(Mn, 16);
  const long mm = (long)Mp * Mp, nn = (long)Np * Np, mq = (long)M * M, mx = (long)M * Mn, nq = (long)Mn * Mn;
#define TR_GET(var, count, label) \
  double* var = s.get((size_t)(count), label); \
  if (!var) return DCGP_ERR_ALLOC
  TR_GET(Kp, mm, "transfer_K");  TR_GET(KLi, mm, "transfer_Linv");   TR_GET(KLiT, mm, "transfer_LinvT");
  TR_GET(Kn0, nn, "transfer_Kn"); TR_GET(Knp, nn, "transfer_Ln"); TR_GET(KnLi, nn, "transfer_LnInv"); TR_GET(KnLiT, nn, "transfer_LnInvT");
  TR_GET(Kc, mx, "transfer_Kc"); TR_GET(Bm, mx, "transfer_B"); TR_GET(P, mx, "transfer_P"); TR_GET(BB, nq, "transfer_BtB");
  TR_GET(Lq, (long)R * mq, "transfer_Lq"); TR_GET(T, (long)R * mx, "transfer_T"); TR_GET(S, (long)R * nn, "transfer_S");
  TR_GET(mn, (long)Mn * R, "transfer_mu");
  int* status = (int*)s.get(1, "transfer_status");
  if (!status) return DCGP_ERR_ALLOC;
  *status_out = status;
  const double *Zk = c.Z, *Znk = c.Zn;
  if (c.ard) {
    TR_GET(Zs, (long)M * L, "transfer_Zs"); TR_GET(Zns, (long)Mn * L, "transfer_Zns");
    hipLaunchKernelGGL(tr_scale_rows_kernel, dim3(nblk((long)M * L)), dim3(256), 0, ctx->stream, c.Z, (long)M * L, L, c.ard, Zs);
    LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(tr_scale_rows_kernel, dim3(nblk((long)Mn * L)), dim3(256), 0, ctx->stream, c.Zn, (long)Mn * L, L, c.ard, Zns);
    LAUNCH_CHECK(ctx);
    Zk = Zs; Znk = Zns;
  }
  // the three kernel matrices.  Kn twice: the chain factors one copy in place, the assembly reads the other
  DCGP_TRY(rbf_gram_padded(ctx, Zk, M, L, c.bk, c.jitter, Kp, Mp, Mp));
  DCGP_TRY(rbf_gram_padded(ctx, Znk, Mn, L, c.bk, c.jitter, Kn0, Np, Np));
  DCGP_TRY(rbf_gram_padded(ctx, Znk, Mn, L, c.bk, c.jitter, Knp, Np, Np));
  DCGP_TRY(cross_gram_enqueue(ctx, c.Z, M, c.Zn, Mn, L, c.bk, c.ard, Kc));
  DCGP_TRY(chain_one(ctx, s.fK, Kp, KLi, KLiT, Mp));       // Kp <- L (strict upper triangle zeroed), KLi = inv(L), KLiT its transpose
  DCGP_TRY(chain_one(ctx, s.fKn, Knp, KnLi, KnLiT, Np));   // Knp <- L'
  // B = inv(L) Kc,  P = inv(L)^T B
  DCGP_TRY(gemm_gen(ctx, mk(KLi, Mp, 1, 0, Kc, Mn, 1, 0, Bm, Mn, 0, M, Mn, M, 1)));
  DCGP_TRY(gemm_gen(ctx, mk(KLiT, Mp, 1, 0, Bm, Mn, 1, 0, P, Mn, 0, M, Mn, M, 1)));
  // q(u) in unwhitened coordinates: the lower triangle of q_sqrt (whatever the caller keeps above it), m
  const double* mu = c.q_mu;
  const double* Lqu = Lq;
  DCGP_TRY(pad_copy(ctx, c.q_sqrt, M, M, M, Lq, M, M, M, 1, R, mq, mq));
  if (c.white) {
    TR_GET(Lq2, (long)R * mq, "transfer_Lq_unwhite"); TR_GET(mu2, (long)M * R, "transfer_mu_unwhite");
    DCGP_TRY(gemm_gen(ctx, mk(Kp, Mp, 1, 0, Lq, M, 1, mq, Lq2, M, mq, M, M, M, R)));
    DCGP_TRY(gemm_gen(ctx, mk(Kp, Mp, 1, 0, c.q_mu, R, 1, 0, mu2, R, 0, M, R, M, 1)));
    Lqu = Lq2; mu = mu2;
  }
  // m' = P^T m,  T_r = Lq_r^T P,  B^T B,  T_r^T T_r (into S_r's corner)
  DCGP_TRY(gemm_gen(ctx, mk(P, 1, Mn, 0, mu, R, 1, 0, mn, R, 0, Mn, R, M, 1)));
  DCGP_TRY(gemm_gen(ctx, mk(Lqu, 1, M, mq, P, Mn, 1, 0, T, Mn, mx, M, Mn, M, R)));
  DCGP_TRY(gemm_gen(ctx, mk(Bm, 1, Mn, 0, Bm, Mn, 1, 0, BB, Mn, 0, Mn, Mn, M, 1)));
  DCGP_TRY(gemm_gen(ctx, mk(T, 1, Mn, mx, T, Mn, 1, mx, S, Np, nn, Mn, Mn, M, R)));
  hipLaunchKernelGGL(tr_assemble_kernel, dim3(nblk(Np), Np, R), dim3(256), 0, ctx->stream, Kn0, BB, S, Mn, Np);
  LAUNCH_CHECK(ctx);
  // chol(S'_r), all r in one batch (factor only: potrf_batched leaves the strict upper triangle as it was, the commit does not read it)
  s.fS.Mp = Np;
  for (int r = 0; r < R; ++r) { s.fS.K.push_back(S + (long)r * nn); s.fS.Linv.push_back(S + (long)r * nn); s.fS.LinvT.push_back(S + (long)r * nn); }
  DCGP_TRY(s.fS.upload(ctx));
  DCGP_TRY(potrf_batched(ctx, s.fS.dK, nullptr, R, Np, Np, s.fS.d_info));
  hipLaunchKernelGGL(tr_status_kernel, dim3(1), dim3(64), 0, ctx->stream, s.fK.d_info, s.fKn.d_info, s.fS.d_info, R, status);
  LAUNCH_CHECK(ctx);
  const double* mu_out = mn;
  const double* Ls_out = S;
  int ld_out = Np;
  long bs_out = nn;
  if (c.white) {   // inv(L') of both; a product of lower-triangular factors is a lower factor of the same covariance
    TR_GET(Lnew, (long)R * nq, "transfer_Lnew"); TR_GET(Lw, (long)R * nq, "transfer_Lnew_white"); TR_GET(mw, (long)Mn * R, "transfer_mu_white");
    DCGP_TRY(pad_copy(ctx, S, Mn, Mn, Np, Lnew, Mn, Mn, Mn, 1, R, nn, nq));
    GenGemm g = mk(KnLi, Np, 1, 0, Lnew, Mn, 1, nq, Lw, Mn, nq, Mn, Mn, Mn, R);
    g.lower_only = 1;
    DCGP_TRY(gemm_gen(ctx, g));
    DCGP_TRY(gemm_gen(ctx, mk(KnLi, Np, 1, 0, mn, R, 1, 0, mw, R, 0, Mn, R, Mn, 1)));
    mu_out = mw; Ls_out = Lw; ld_out = Mn; bs_out = nq;
  }
#undef TR_GET
  hipLaunchKernelGGL(tr_commit_copy_kernel, dim3(nblk((long)Mn * R)), dim3(256), 0, ctx->stream, status, mu_out, (long)Mn * R, c.out_q_mu);
  LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(tr_commit_tril_kernel, dim3(nblk(Mn), Mn, R), dim3(256), 0, ctx->stream, status, Ls_out, ld_out, bs_out, Mn, c.out_q_sqrt);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

}  // namespace

#define TR_ARG(cond, ...) \
  do { if (!(cond)) return ctx_fail(ctx, DCGP_ERR_ARG, __VA_ARGS__); } while (0)

extern "C" int dcgp_cross_gram(dcgp_ctx* ctx, const double* A, long m, const double* B, long n, int d, int kernel_type, double variance, double p1,
                               double p2, const double* ard_lengthscales, double* out) {
  if (!ctx) return DCGP_ERR_ARG;
  TR_ARG(A && B && out, "cross_gram: A, B or out is NULL");
  TR_ARG(m >= 1 && m <= 32L * 65535, "cross_gram: m = %ld outside 1 .. %ld", m, 32L * 65535);
  TR_ARG(n >= 1 && n <= 0x7fffffffL, "cross_gram: n = %ld outside 1 .. 2^31 - 1", n);
  TR_ARG(d >= 1 && d <= TR_MAX_L, "cross_gram: d = %d outside 1 .. %d", d, TR_MAX_L);
  BaseKernel bk;
  DCGP_TRY(kernel_args(ctx, "cross_gram", kernel_type, variance, p1, p2, ard_lengthscales, &bk));
  DCGP_TRY(cross_gram_enqueue(ctx, A, m, B, n, d, bk, ard_lengthscales, out));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return DCGP_OK;
}

extern "C" int dcgp_inducing_transfer(dcgp_ctx* ctx, const double* Z, int M, const double* Z_new, int M_new, int L, int kernel_type, double variance,
                                      double p1, double p2, const double* ard_lengthscales, double jitter, int white, const double* q_mu,
                                      const double* q_sqrt, int R, double* out_q_mu, double* out_q_sqrt, int* info_host) {
  if (!ctx) return DCGP_ERR_ARG;
  if (info_host) info_host[0] = info_host[1] = 0;
  TR_ARG(Z && Z_new && q_mu && q_sqrt && out_q_mu && out_q_sqrt, "inducing_transfer: a NULL array");
  TR_ARG(M >= 1 && M <= TR_MAX_M, "inducing_transfer: M = %d outside 1 .. %d", M, TR_MAX_M);
  TR_ARG(M_new >= 1 && M_new <= TR_MAX_M, "inducing_transfer: M' = %d outside 1 .. %d", M_new, TR_MAX_M);
  TR_ARG(R >= 1 && R <= TR_MAX_R, "inducing_transfer: R = %d outside 1 .. %d", R, TR_MAX_R);
  TR_ARG(L >= 1 && L <= TR_MAX_L, "inducing_transfer: L = %d outside 1 .. %d", L, TR_MAX_L);
  TR_ARG(jitter >= 0.0 && std::isfinite(jitter), "inducing_transfer: jitter must not be negative, got %g", jitter);
  TrCall c;
  DCGP_TRY(kernel_args(ctx, "inducing_transfer", kernel_type, variance, p1, p2, ard_lengthscales, &c.bk));
  c.Z = Z; c.Zn = Z_new; c.ard = ard_lengthscales; c.q_mu = q_mu; c.q_sqrt = q_sqrt; c.out_q_mu = out_q_mu; c.out_q_sqrt = out_q_sqrt;
  c.M = M; c.Mn = M_new; c.L = L; c.R = R; c.white = white ? 1 : 0; c.jitter = jitter;
  TrScratch s(ctx);
  int* status = nullptr;
  const int rc = transfer_enqueue(ctx, c, s, &status);
  if (rc != DCGP_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }   // nothing of this call is in flight when its buffers go
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_info, status, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const int which = ctx->h_info[0], col = ctx->h_info[1];
  if (info_host) { info_host[0] = which; info_host[1] = col; }
  if (which == 1) return ctx_fail(ctx, DCGP_ERR_NOT_PD, "inducing_transfer: K(Z, Z) + jitter I is not positive definite at column %d", col);
  if (which == 2) return ctx_fail(ctx, DCGP_ERR_NOT_PD, "inducing_transfer: K(Z', Z') + jitter I is not positive definite at column %d", col);
  if (which >= 3) return ctx_fail(ctx, DCGP_ERR_NOT_PD, "inducing_transfer: S' of output %d is not positive definite at column %d", which - 3, col);
  return DCGP_OK;
}

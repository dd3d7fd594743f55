// chol_fused.hip -- right-looking blocked Cholesky with the inverse of the factor folded into the same launches.
//
// The replicated M x M stage is a serial chain; what it costs is the NUMBER of dependent launches and the latency
// inside each (launch + memory round trips), not flops.  A textbook right-looking potrf (panel, update) followed by
// a recursive-doubling trtri took 23 dependent launches at M = 256.  Here panel j is ONE launch whose workgroups
// are independent of each other because each recomputes the small shared pieces it needs:
//     every workgroup : L_jj = chol(A[j,j])   (one wavefront: registers + LDS broadcast line), and the 32-column
//                       panel rows it touches, L[rows,j] = A[rows,j] L_jj^-T (one row per lane)
//     trailing tile   : A[ri,rc] -= L[ri,j] L[rc,j]^T                      (matrix cores, k = 32)
//     inverse tile    : with Y the running product of block Gauss transforms applied to I (inv(L) row blocks
//                       < j are final):  Ynew = inv(L_jj) Y[j,cols]  ->  final rows of inv(L);
//                       Y[rows,cols] -= L[rows,j] Ynew for the rows below (matrix cores, k = 32)
// so every launch has constant depth (k = 32) and the chain is M/32 launches + 1 (finish) for both
// tf.cholesky (conv_gp/conditionals.py:29, layers.py:151,156) and the inverse the triangular solves
// (conditionals.py:31-33,44-47) are applied with.  Final values go to separate buffers (other workgroups of the
// same launch still read the working copies).  All matrices of a model are batched in grid.y.
// (Handing panels between the workgroups of ONE launch, through coherent flags and payloads instead of launch boundaries, was built,
// measured slower and removed: DESIGN.md, "One launch for the whole chain".)
#include "chol_dev.h"
#include "chain_plan.h"

using namespace chol_dev;
static_assert(chain_plan::kNB == NB, "chain_plan.h plans the panels of this kernel");

// phase timestamps for tools/chol_trace.hip (compiled out of the library)
#ifdef CHOL_TRACE
__device__ long long g_chol_trace[64 * 32];
#define TR(k)                                                                                              \
  if (tid == 0 && b == 0 && (bx == 0 || bx == a.gx_trace - 1))                                             \
    g_chol_trace[(a.j / NB) * 32 + (bx == 0 ? 0 : 16) + (k)] = wall_clock64();
#else
#define TR(k)
#endif

namespace {

// LDS of chol_rl_kernel is a budget: beside a patch sweep -- which claims 53 KB per workgroup so that a chain workgroup fits the moment one of its
// three per CU ends, head_units.hip -- a kernel of 54144 bytes ran the head-only model's chain at 150 us and its sweep at 178, one of 53760 at 108 and
// 168: 4250 -> 4350 steps/s, 4500 -> 4780 in flight.  The line's sink (col, of the diagonal block's factorisation) is therefore 16 slots, not one per lane.
constexpr int COL_N = 48;

struct RlArgs {
  double* const* A;      // working matrices (destroyed): trailing part updated in place
  double* Lout;          // [batch][Mp][ld] final factor (lower), then copied back over A by the finish kernel
  double* Y;             // [batch][Mp][ld] running inverse (scratch) or nullptr
  double* const* Linv;   // final inv(L) or nullptr; every element is written by the chain (zeros included)
  double* const* LinvT;  // its transpose, written in the same pass, or nullptr
  int Mp, ld, j, nt, nT, nct;
  int* info;
  // Look-ahead across the launch boundary.  Xin != nullptr: L_jj and inv(L_jj) of THIS panel were produced by the previous launch
  // ([batch][2][NB][NB]: factor, inverse) and are read instead of recomputed by every workgroup.  Xnext != nullptr: one extra
  // workgroup (blockIdx.x == la_idx) forms the NEXT diagonal block -- A[jn,jn] - P P^T, P = A[jn,j] inv(L_jj)^T, a 32 x 32 solve
  // and update -- factors and inverts it while the other workgroups do the trailing update, and leaves both for the next launch.
  // The 32-step pivot recurrence (5.5 us, the only inherently serial part of a panel) thereby runs BESIDE the trailing tiles of
  // the previous panel instead of in front of every one of them: 14.4 -> ~11 us per panel.
  const double* Xin = nullptr;
  double* Xnext = nullptr;
  int la_idx = -1;
  // Right-hand sides riding the chain (round 5): G_r = inv(L) Lq_r and alpha = inv(L) q_mu -- the conditional's small operands, one launch
  // of their own until now (prep_solve, 13 us behind the last panel) -- by block forward substitution ONE PANEL BEHIND the factorisation:
  // launch jp applies panel p = jp - 1, whose rows of L (Lout) and inverse diagonal block (Xall slot p) the previous launch left in memory;
  // the last launch also applies the last panel.  Workgroups [rhs_base, ...) of a launch: (right-hand side q, 32-column tile ct, row tile rt).
  const ChainRhs* rhs = nullptr;   // per matrix of the batch
  const double* Xall = nullptr;    // [np][batch][2][NB][NB]: factor and inverse of every diagonal block (slot 0 written by launch 0's first workgroup)
  double* Xself = nullptr;         // launch 0: where its first workgroup leaves block 0 (slot 0 of Xall)
  int rhs_base = 0, rhs_p = -1, rhs_last = 0, rhs_nt = 0, rhs_nq = 0, rhs_tpw = 1, batch = 0, np = 0;
  // XCD isolation (iso_per > 0: 1-D grid).  Workgroup i of a launch runs on XCD i % 8.  fp64 MFMAs of ANY wave hold a SIMD for 64 cycles
  // during which no other wave's VALU instruction issues there -- wave priorities do not help -- and the look-ahead workgroup's
  // recurrence is one issue-bound wave: with the right-hand sides' ~700 workgroups in the launch, three to a CU, every panel launch took
  // 1.3 us longer.  So the look-ahead workgroups of all matrices sit alone on one XCD and every other tile on the seven others (right-hand
  // sides first: the longest).  Which XCD: workgroups of XCD 7 start 0.7 us before those of XCD 0 (stamps of the first instruction: a launch's
  // look-ahead workgroups ended +8.2-8.9 us after its first workgroup on XCD 7, +9.0-10.5 on XCD 0 or 3).
  int iso_per = 0;
  int gx_trace = 0;

};

// The prologue loads are written as fully unrolled register batches (all global loads issued, then all LDS stores):
// as rolled loops each iteration waited for its own load -- 4 + 8 + 8 serial memory latencies per workgroup.
__device__ __forceinline__ void load_diag(const double* __restrict__ A, int ld, int j, int nb, double (*D)[NB + 1], int tid) {
  double t[NB * NB / 256];
#pragma unroll
  for (int e = 0; e < NB * NB / 256; ++e) {
    const int idx = tid + e * 256, r = idx / NB, c = idx % NB;
    t[e] = (r == c) ? 1.0 : 0.0;
    if (r < nb && c < nb && c <= r) t[e] = A[(long)(j + r) * ld + j + c];
  }
#pragma unroll
  for (int e = 0; e < NB * NB / 256; ++e) {
    const int idx = tid + e * 256;
    D[idx / NB][idx % NB] = t[e];
  }
}
// rows [r0, r0+64) of the panel columns -> U[64][33] (zero beyond the matrix)
__device__ __forceinline__ void load_panel_rows(const double* __restrict__ A, int ld, int Mp, int j, int nb, int r0,
                                                double (*U)[NB + 1], int tid) {
  double t[64 * NB / 256];
#pragma unroll
  for (int e = 0; e < 64 * NB / 256; ++e) {
    const int idx = tid + e * 256, i = idx / NB, c = idx % NB;
    t[e] = (r0 + i < Mp && c < nb) ? A[(long)(r0 + i) * ld + j + c] : 0.0;
  }
#pragma unroll
  for (int e = 0; e < 64 * NB / 256; ++e) {
    const int idx = tid + e * 256;
    U[idx / NB][idx % NB] = t[e];
  }
}
// P = U inv(L_jj)^T on the matrix cores (64 x 32 x 32): P[i][c] = sum_q U[i][q] X[c][q].  Wave (wm, wn) owns rows
// wm*32 .. +31 and columns wn*16 .. +15; the result goes back over U after a barrier (both waves of a row block read
// all of its columns).
__device__ __forceinline__ void panel_solve_mfma(double (*U)[NB + 1], const double (*X)[NB + 1], int wm, int wn, int lrow,
                                                 int lcol, d4 (&p)[2]) {
  p[0] = d4{0.0, 0.0, 0.0, 0.0};
  p[1] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < NB; kk += 4) {
    const double bv = X[wn * 16 + lcol][kk + lrow];
#pragma unroll
    for (int x = 0; x < 2; ++x) p[x] = __builtin_amdgcn_mfma_f64_16x16x4f64(U[wm * 32 + x * 16 + lcol][kk + lrow], bv, p[x], 0, 0, 0);
  }
}
__device__ __forceinline__ void panel_store(double (*U)[NB + 1], int wm, int wn, int lrow, int lcol, const d4 (&p)[2]) {
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int v = 0; v < 4; ++v) U[wm * 32 + x * 16 + lrow + 4 * v][wn * 16 + lcol] = p[x][v];
}


// ---- right-hand sides riding the chain (RlArgs::rhs): workgroup `idx` of the launch's right-hand-side part ----
// Item (q, ct, g): right-hand side q (q < R: Lq_q, lower triangular; q == R: q_mu), columns [32 ct, 32 ct + 32), row group g.  Every item forms
// Ynew = inv(L_pp) Y_p (the 32 x 32 block of the lagged panel p: 8 MFMAs a wave, cheaper than waiting for another workgroup); group 0 stores
// it (final rows of G_q / alpha) and its sum of squares; group g then updates the 64-row tiles 2g and 2g + 1 below, Y -= L[rows, p] Ynew.
// (Two row tiles per workgroup: with one, a launch carried ~700 workgroups against 672-768 resident slots, and the few that had to wait for
// a slot made every panel launch 1.4 us longer; the dispatcher also needs ~10 ns per workgroup.)  In the LAST launch the row tile that holds the
// last panel's rows goes on to make them final with the inverse block this launch was handed, and one more item per right-hand side
// (ct == p + 1: the diagonal block of Lq, first touched by the last panel) does only that.  Values a panel touches first come from the
// right-hand side itself, later ones from the scratch Yw.  The item on the diagonal also writes the structural zeros to the right of its
// final rows, so G needs no clearing.
__device__ __forceinline__ void rhs_tile(const RlArgs& a, const int b, const int idx, double (*D)[NB + 1], double (*Xs)[NB + 1], double (&col)[COL_N],
                                         double (*Tp)[17], double (*Ui)[NB + 1], double* UcTs, double* sc) {
  double (*Ts)[64 + 1] = reinterpret_cast<double (*)[64 + 1]>(UcTs);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane >> 4, lcol = lane & 15;
  const ChainRhs d = a.rhs[b];
  const int Mp = a.Mp, ld = a.ld, np = a.np, p = a.rhs_p;
  // decode: R blocks of rhs_nq items (Lq_q), then alpha's
  const int tpw = a.rhs_tpw, ng = chain_plan::rhs_groups(a.rhs_nt, tpw);   // row tiles per workgroup (1 or 2), row groups
  const chain_plan::RhsItem item = chain_plan::decode_rhs(idx, d.R, a.rhs_nq, p, a.rhs_last, ng);
  if (!item.live) return;
  const int q = item.q, ct = item.ct, g = item.g;
  const bool final_only = item.final_only;
  const bool is_alpha = q == d.R;
  const double* __restrict__ B = is_alpha ? d.qmu : (d.Lq ? d.Lq + (long)q * Mp * ld : nullptr);
  if (!B) return;
  const int ldb = is_alpha ? d.Rp : ld, ncol = is_alpha ? d.Rp : Mp, c0 = ct * 32;
  if (c0 >= ncol) return;
  const bool lagged = !final_only;
  const int j = 32 * (p < 0 ? 0 : p);
  double* __restrict__ Yq = d.Yw + (long)(is_alpha ? d.R : q) * Mp * ld;          // (alpha's scratch behind the R matrices; its rows are ldb wide)
  double* __restrict__ Cq = is_alpha ? d.alpha : (d.G ? d.G + (long)q * Mp * ld : nullptr);
  double* __restrict__ sq = d.sums + (long)q * (np * (np + 1) / 2);
  const double* __restrict__ Lout = a.Lout + (long)b * Mp * ld;
  const int jl = 32 * (np - 1), nbl = Mp - jl;                                     // the last panel
  const int t0 = chain_plan::rhs_first_tile(g, tpw);
  const int r0[2] = {j + 32 + 64 * t0, j + 32 + 64 * t0 + 64};                     // this group's row tiles
  const bool live[2] = {lagged && r0[0] < Mp, lagged && tpw == 2 && r0[1] < Mp};
  const bool cont = live[0] && a.rhs_last && g == 0;                               // the first row tile holds the last panel's rows (r0 == jl)
  const bool have_x = a.Xin != nullptr;

  // ---- every global read, in one latency ----
  double tx[NB * NB / 256], tl[NB * NB / 256], tt[NB * NB / 256], tu[2][64 * NB / 256], old[2][2][4];
#pragma unroll
  for (int e = 0; e < NB * NB / 256; ++e) { tx[e] = 0.0; tl[e] = 0.0; }
  if (lagged) {
    const double* __restrict__ xp = a.Xall + ((long)p * a.batch + b) * 2 * NB * NB + NB * NB;
#pragma unroll
    for (int e = 0; e < NB * NB / 256; ++e) tx[e] = xp[tid + e * 256];
  }
  if ((cont || final_only) && have_x) {
    const double* __restrict__ xl = a.Xin + (long)b * 2 * NB * NB + NB * NB;
#pragma unroll
    for (int e = 0; e < NB * NB / 256; ++e) tl[e] = xl[tid + e * 256];
  }
  {
    const bool first = final_only || (is_alpha ? p == 0 : ct == p);
    const double* __restrict__ src = first ? B : Yq;
    const int jr = final_only ? jl : j;
#pragma unroll
    for (int e = 0; e < NB * NB / 256; ++e) {
      const int i2 = tid + e * 256, qr = i2 >> 5, c = i2 & 31;
      tt[e] = (jr + qr < Mp && c0 + c < ncol) ? src[(long)(jr + qr) * ldb + c0 + c] : 0.0;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int i = r0[t] + 16 * wave + lrow + 4 * v, gc = c0 + 16 * y + lcol;
          old[t][y][v] = (live[t] && i < Mp && gc < ncol) ? src[(long)i * ldb + gc] : 0.0;
        }
#pragma unroll
      for (int e = 0; e < 64 * NB / 256; ++e) {
        const int i2 = tid + e * 256, i = i2 / NB, c = i2 % NB;
        tu[t][e] = (live[t] && r0[t] + i < Mp) ? Lout[(long)(r0[t] + i) * ld + j + c] : 0.0;
      }
    }
  }
  if (final_only && !have_x) load_diag(a.A[b], ld, 0, min(NB, Mp), D, tid);   // one-panel matrix: this launch factors it, every workgroup for itself
  else {
#pragma unroll
    for (int e = 0; e < NB * NB / 256; ++e) { const int i2 = tid + e * 256; D[i2 / NB][i2 % NB] = tx[e]; }
  }
  if (have_x) {
#pragma unroll
    for (int e = 0; e < NB * NB / 256; ++e) { const int i2 = tid + e * 256; Xs[i2 / NB][i2 % NB] = tl[e]; }
  }
#pragma unroll
  for (int e = 0; e < NB * NB / 256; ++e) { const int i2 = tid + e * 256; Ts[i2 >> 5][i2 & 31] = tt[e]; }
  if (live[0]) {
#pragma unroll
    for (int e = 0; e < 64 * NB / 256; ++e) { const int i2 = tid + e * 256; Ui[i2 / NB][i2 % NB] = tu[0][e]; }
  }
  __syncthreads();
  if (final_only && !have_x) {
    potrf_inv32_wg<NB + 1>(D, Xs, col, Tp, sc, tid);
    __syncthreads();
  }

  // Ts (32 x 32) <- Xm Ts: wave w owns the 16 x 16 block (w >> 1, w & 1)
  auto ynew = [&](const double (*Xm)[NB + 1]) {
    const int bm = wave >> 1, bn = wave & 1;
    d4 y = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < NB; kk += 4) y = __builtin_amdgcn_mfma_f64_16x16x4f64(Xm[bm * 16 + lcol][kk + lrow], Ts[kk + lrow][bn * 16 + lcol], y, 0, 0, 0);
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 4; ++v) Ts[bm * 16 + lrow + 4 * v][bn * 16 + lcol] = y[v];
    __syncthreads();
  };
  // rows [jr, jr + nbr) of the result are final: store, zeros to the right of a diagonal tile, sum of squares -> slot
  auto finish = [&](int jr, int nbr, int pc) {
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < NB * NB / 256; ++e) {
      const int i2 = tid + e * 256, qr = i2 >> 5, c = i2 & 31;
      if (qr < nbr && c0 + c < ncol) {
        const double x = Ts[qr][c];
        s = fma(x, x, s);
        if (Cq) Cq[(long)(jr + qr) * ldb + c0 + c] = x;
      }
    }
    if (Cq && !is_alpha && ct == pc) {
      const int z0 = 32 * (pc + 1), zw = Mp - z0;
      for (int i2 = tid; i2 < nbr * zw; i2 += 256) Cq[(long)(jr + i2 / zw) * ldb + z0 + i2 % zw] = 0.0;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
    if (lane == 0) col[wave] = s;
    __syncthreads();
    if (tid == 0) sq[is_alpha ? pc : pc * (pc + 1) / 2 + ct] = (col[0] + col[1]) + (col[2] + col[3]);
  };

  if (final_only) {
    ynew(Xs);
    finish(jl, nbl, np - 1);
    return;
  }
  ynew(D);
  if (g == 0) finish(j, NB, p);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (!live[t]) break;
    if (t == 1) {   // the second tile's rows of L waited in registers
      __syncthreads();
#pragma unroll
      for (int e = 0; e < 64 * NB / 256; ++e) { const int i2 = tid + e * 256; Ui[i2 / NB][i2 % NB] = tu[1][e]; }
      __syncthreads();
    }
    d4 acc[2] = {d4{0.0, 0.0, 0.0, 0.0}, d4{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
    for (int kk = 0; kk < NB; kk += 4) {
      const double av = Ui[16 * wave + lcol][kk + lrow];
#pragma unroll
      for (int y = 0; y < 2; ++y) acc[y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Ts[kk + lrow][16 * y + lcol], acc[y], 0, 0, 0);
    }
    if (t == 0 && cont) {
      // the last panel's rows, updated through panel p: final with this launch's inverse block
      __syncthreads();
      if (wave < 2) {
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
          for (int v = 0; v < 4; ++v) Ts[16 * wave + lrow + 4 * v][16 * y + lcol] = old[0][y][v] - acc[y][v];
      }
      __syncthreads();
      ynew(Xs);
      finish(jl, nbl, np - 1);
      return;
    }
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int i = r0[t] + 16 * wave + lrow + 4 * v, gc = c0 + 16 * y + lcol;
        if (i < Mp && gc < ncol) Yq[(long)i * ldb + gc] = old[t][y][v] - acc[y][v];
      }
  }
}

__global__ __launch_bounds__(256, 2) void chol_rl_kernel(RlArgs a) {
  __shared__ double D[NB][NB + 1];
  __shared__ __attribute__((aligned(16))) double col[COL_N];
  __shared__ double Ui[64][NB + 1];
  __shared__ double UcTs[64 * (NB + 1)];   // trailing tiles: second panel row block; inverse tiles: the Y tile
  __shared__ double Xs[NB][NB + 1];   // inv(L_jj)
  __shared__ double Tp[16][17];       // scratch of the diagonal block's factorisation
  __shared__ double sc[64];           // ... (reciprocal pivots and scalings)
  double (*Uc)[NB + 1] = reinterpret_cast<double (*)[NB + 1]>(UcTs);
  double (*Ts)[64 + 1] = reinterpret_cast<double (*)[64 + 1]>(UcTs);   // [NB][65]: old Y rows, then new
  static_assert(NB * 65 <= 64 * (NB + 1), "Y tile fits the shared slot");
  // the chain is latency: when it shares CUs with a throughput kernel (the head sweep of a head-first model, the previous step's layer
  // kernel with steps in flight) its waves go first in the issue arbitration
  // (the look-ahead workgroup is the launch's critical path and issue-bound: the other workgroups of the chain sharing its SIMDs yield to it)
  int b = blockIdx.y, bx = blockIdx.x;
  if (a.iso_per > 0) {
    // the look-ahead workgroups on one XCD, the right-hand sides and then the trailing / inverse tiles on the seven others (chain_plan.h)
    const chain_plan::Wg w = chain_plan::decode_iso(blockIdx.x, a.batch, a.iso_per, a.la_idx, a.rhs != nullptr, a.rhs_base);
    if (!w.live) return;
    b = w.b; bx = w.bx;
  }
  if (bx == a.la_idx) __builtin_amdgcn_s_setprio(3);
  else __builtin_amdgcn_s_setprio(2);
  if (a.rhs && bx >= a.rhs_base) {   // a right-hand side riding the chain
    rhs_tile(a, b, bx - a.rhs_base, D, Xs, col, Tp, Ui, UcTs, sc);
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, lrow = lane >> 4, lcol = lane & 15;
  const int Mp = a.Mp, ld = a.ld, j = a.j, nb = min(NB, Mp - j);
  double* __restrict__ A = a.A[b];
  double* __restrict__ Lout = a.Lout + (long)b * Mp * ld;
  double* __restrict__ Y = a.Y ? a.Y + (long)b * Mp * ld : nullptr;
  const int below0 = j + NB;   // first row below the panel block

  // ---- prologue: every global read of this workgroup is issued here, in one latency ----
  TR(0)
  const bool have_x = a.Xin != nullptr;
  const bool is_la = bx == a.la_idx;
  if (have_x) {   // factor and inverse of this panel's diagonal block: left by the previous launch's look-ahead workgroup
    const double* __restrict__ xin = a.Xin + (long)b * 2 * NB * NB;
    double t[2 * NB * NB / 256];
#pragma unroll
    for (int e = 0; e < 2 * NB * NB / 256; ++e) t[e] = xin[tid + e * 256];
#pragma unroll
    for (int e = 0; e < 2 * NB * NB / 256; ++e) {
      const int idx = tid + e * 256, r = (idx & (NB * NB - 1)) / NB, c = idx % NB;
      if (idx < NB * NB) D[r][c] = t[e]; else Xs[r][c] = t[e];
    }
  } else {
    load_diag(A, ld, j, nb, D, tid);
  }
  const bool only_diag = a.nT == 0 && a.nct == 0 && !is_la;
  const bool is_trailing = bx < a.nT;
  int ti = 0, tc = 0, rt = -1, ct = 0;
  double old[2][2][4];   // values the final read-modify-write subtracts from
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int v = 0; v < 4; ++v) old[x][y][v] = 0.0;
  const int jn = j + NB, nbn = min(NB, Mp - jn);
  double la_u[NB * NB / 256], la_d[NB * NB / 256];   // look-ahead: A[jn.., j..] and the lower triangle of A[jn.., jn..]
  if (only_diag) {
  } else if (is_la) {
#pragma unroll
    for (int e = 0; e < NB * NB / 256; ++e) {
      const int idx = tid + e * 256, r = idx / NB, c = idx % NB;
      la_u[e] = (r < nbn && c < nb) ? A[(long)(jn + r) * ld + j + c] : 0.0;
      la_d[e] = (r == c) ? 1.0 : 0.0;
      if (r < nbn && c < nbn && c <= r) la_d[e] = A[(long)(jn + r) * ld + jn + c];
    }
  } else if (is_trailing) {
    int pair = bx;
    while (pair >= a.nt - tc) {   // column-major enumeration of the lower triangle: tc <= ti
      pair -= a.nt - tc;
      ++tc;
    }
    ti = tc + pair;
    load_panel_rows(A, ld, Mp, j, nb, below0 + ti * 64, Ui, tid);
    if (tc != ti) load_panel_rows(A, ld, Mp, j, nb, below0 + tc * 64, Uc, tid);
    const int ri0 = below0 + ti * 64, rc0 = below0 + tc * 64;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int i = ri0 + wm * 32 + x * 16 + lrow + 4 * v, jj = rc0 + wn * 32 + y * 16 + lcol;
          if (i < Mp && jj < Mp && jj <= i) old[x][y][v] = A[(long)i * ld + jj];
        }
  } else {
    const int yy = bx - a.nT;
    rt = yy / a.nct - 1;   // -1: the panel's own row block, else row tile below
    ct = yy % a.nct;
    const int c0 = ct * 64;
    if (rt >= 0) {
      load_panel_rows(A, ld, Mp, j, nb, below0 + rt * 64, Ui, tid);
      const int r0 = below0 + rt * 64;
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int i = r0 + wm * 32 + x * 16 + lrow + 4 * v, gc = c0 + wn * 32 + y * 16 + lcol;
            if (i < Mp && gc < j) old[x][y][v] = Y[(long)i * ld + gc];   // identity part is zero below the diagonal
          }
    }
    // Y[j + q, c0 + c] before this step: stored values left of column j, identity inside [j, j+32), zero beyond
    double tt[NB * 64 / 256];
#pragma unroll
    for (int e = 0; e < NB * 64 / 256; ++e) {
      const int idx = tid + e * 256, q = idx >> 6, c = idx & 63, gc = c0 + c;
      tt[e] = 0.0;
      if (q < nb && gc < j) tt[e] = Y[(long)(j + q) * ld + gc];
      else if (gc == j + q) tt[e] = 1.0;
    }
#pragma unroll
    for (int e = 0; e < NB * 64 / 256; ++e) {
      const int idx = tid + e * 256;
      Ts[idx >> 6][idx & 63] = tt[e];
    }
  }
  __syncthreads();
  TR(1)
  // ---- L_jj and inv(L_jj) (unless the previous launch left them); the look-ahead workgroup then the NEXT diagonal block too ----
  // ONE call site of the block routine for both (a loop of up to two passes): inlined twice, its ~1500 straight-line instructions made the kernel
  // large enough to evict a co-running sweep's code and its own (head-only model: sweep 168 -> 177 us, chain 141 -> 152 beside each other).
  int fail_j = 0, fail_n = 0;
  double* __restrict__ xn = is_la ? a.Xnext + (long)b * 2 * NB * NB : nullptr;
  for (int pass = have_x ? 1 : 0; pass < (is_la ? 2 : 1); ++pass) {
    if (pass == 1) {
      // ---- the next diagonal block: P = U inv(L_jj)^T, D_next = A[jn,jn] - P P^T ----
      double (*U)[NB + 1] = Ui;
      double (*Pm)[NB + 1] = reinterpret_cast<double (*)[NB + 1]>(UcTs);
#pragma unroll
      for (int e = 0; e < NB * NB / 256; ++e) { const int idx = tid + e * 256; U[idx / NB][idx % NB] = la_u[e]; }
      __syncthreads();
      const int bm = wave >> 1, bn = wave & 1;
      {
        d4 pacc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < NB; kk += 4)
          pacc = __builtin_amdgcn_mfma_f64_16x16x4f64(U[bm * 16 + lcol][kk + lrow], Xs[bn * 16 + lcol][kk + lrow], pacc, 0, 0, 0);
#pragma unroll
        for (int v = 0; v < 4; ++v) Pm[bm * 16 + lrow + 4 * v][bn * 16 + lcol] = pacc[v];
      }
      __syncthreads();   // (also: everyone is done with D = L_jj, which the first workgroup of the launch publishes from its own copy)
#pragma unroll
      for (int e = 0; e < NB * NB / 256; ++e) { const int idx = tid + e * 256; D[idx / NB][idx % NB] = la_d[e]; }
      __syncthreads();
      {
        d4 dacc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < NB; kk += 4)
          dacc = __builtin_amdgcn_mfma_f64_16x16x4f64(Pm[bm * 16 + lcol][kk + lrow], Pm[bn * 16 + lcol][kk + lrow], dacc, 0, 0, 0);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int r = bm * 16 + lrow + 4 * v, c = bn * 16 + lcol;
          if (c <= r && r < nbn) D[r][c] -= dacc[v];
        }
      }
      __syncthreads();
      TR(3)
    }
    const int fail = potrf_inv32_wg<NB + 1>(D, Xs, col, Tp, sc, tid);   // (all four waves; the status is wave 0's)
    __syncthreads();
    if (pass == 0) {
      TR(2)
      if (tid < 64) fail_j = fail;
      // (with a look-ahead workgroup in the launch it is the one writer of the status word: it sees this panel's failure too)
      if (tid == 0 && bx == 0 && a.la_idx < 0 && (j == 0 || (fail && a.info[b] == 0))) a.info[b] = fail ? j + fail : 0;
    } else {
      TR(4)
      if (tid < 64) fail_n = fail;
    }
  }
  if (is_la) {
#pragma unroll
    for (int e = 0; e < NB * NB / 256; ++e) {
      const int idx = tid + e * 256, r = idx / NB, c = idx % NB;
      xn[idx] = D[r][c];
      xn[NB * NB + idx] = Xs[r][c];
      if (r < nbn && c < nbn) Lout[(long)(jn + r) * ld + jn + c] = D[r][c];
    }
    if (tid == 0) {   // status word: first failing column of the chain so far (launch 0 initialises it)
      const int mine = fail_j ? j + fail_j : (fail_n ? jn + fail_n : 0);
      if (j == 0) a.info[b] = mine;
      else if (mine && a.info[b] == 0) a.info[b] = mine;
    }
    TR(5)
    return;
  }
  if (bx == 0 && !have_x) {   // publish L_jj (final; with Xin the previous launch's look-ahead workgroup already has)
    for (int idx = tid; idx < nb * nb; idx += 256) {
      const int r = idx / nb, c = idx % nb;
      Lout[(long)(j + r) * ld + j + c] = D[r][c];
    }
    if (a.Xself) {   // ... and block 0 with its inverse where the right-hand sides of the next launch read them
      double* __restrict__ xs = a.Xself + (long)b * 2 * NB * NB;
      for (int idx = tid; idx < NB * NB; idx += 256) { xs[idx] = D[idx / NB][idx % NB]; xs[NB * NB + idx] = Xs[idx / NB][idx % NB]; }
    }
  }
  if (only_diag) return;

  d4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = d4{0.0, 0.0, 0.0, 0.0};

  if (is_trailing) {
    // ---- trailing tile (ti, tc): panel rows L[r,j] = A[r,j] inv(L_jj)^T, then A[ri, rc] -= L[ri,j] L[rc,j]^T ----
    d4 pi[2], pc[2];
    panel_solve_mfma(Ui, Xs, wm, wn, lrow, lcol, pi);
    if (tc != ti) panel_solve_mfma(Uc, Xs, wm, wn, lrow, lcol, pc);
    __syncthreads();
    panel_store(Ui, wm, wn, lrow, lcol, pi);
    if (tc != ti) panel_store(Uc, wm, wn, lrow, lcol, pc);
    __syncthreads();
    TR(3)
    const int ri0 = below0 + ti * 64, rc0 = below0 + tc * 64;
    double (*Ub)[NB + 1] = (tc == ti) ? Ui : Uc;
    if (tc == ti) {   // the diagonal tiles publish the panel rows of L (final)
      for (int idx = tid; idx < 64 * NB; idx += 256) {
        const int i = idx / NB, c = idx % NB;
        if (ri0 + i < Mp && c < nb) Lout[(long)(ri0 + i) * ld + j + c] = Ui[i][c];
      }
    }
#pragma unroll
    for (int kk = 0; kk < NB; kk += 4) {
      double avv[2], bvv[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) avv[x] = Ui[wm * 32 + x * 16 + lcol][kk + lrow];
#pragma unroll
      for (int y = 0; y < 2; ++y) bvv[y] = Ub[wn * 32 + y * 16 + lcol][kk + lrow];
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(avv[x], bvv[y], acc[x][y], 0, 0, 0);
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int i = ri0 + wm * 32 + x * 16 + lrow + 4 * v, jj = rc0 + wn * 32 + y * 16 + lcol;
          // (the next diagonal block is the look-ahead workgroup's: it reads it as the previous panel left it, concurrently with this
          // launch -- nobody may update it in place, and nobody reads it from A afterwards)
          const bool la_block = a.la_idx >= 0 && i < below0 + NB && jj < below0 + NB;
          if (i < Mp && jj < Mp && jj <= i && !la_block) A[(long)i * ld + jj] = old[x][y][v] - acc[x][y][v];
        }
    TR(4)
    return;
  }

  // ---- inverse tile (rt, ct): columns [c0, c0+64) of the running inverse ----
  double* __restrict__ Linv = a.Linv[b];
  const int c0 = ct * 64;
  // Ynew = inv(L_jj) * Yold  (32 x 32 times 32 x 64) on the matrix cores: wave w owns columns w*16 .. +15
  d4 yn[2] = {d4{0.0, 0.0, 0.0, 0.0}, d4{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
  for (int kk = 0; kk < NB; kk += 4) {
    const double bv = Ts[kk + lrow][wave * 16 + lcol];
#pragma unroll
    for (int x = 0; x < 2; ++x) yn[x] = __builtin_amdgcn_mfma_f64_16x16x4f64(Xs[x * 16 + lcol][kk + lrow], bv, yn[x], 0, 0, 0);
  }
  d4 pi[2];
  if (rt >= 0) panel_solve_mfma(Ui, Xs, wm, wn, lrow, lcol, pi);
  __syncthreads();
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int v = 0; v < 4; ++v) Ts[x * 16 + lrow + 4 * v][wave * 16 + lcol] = yn[x][v];
  if (rt >= 0) panel_store(Ui, wm, wn, lrow, lcol, pi);
  __syncthreads();
  TR(4)
  if (rt < 0) {
    // final rows j .. j+31 of inv(L) -- and the same block of the transpose; the structural zeros to the right of the
    // diagonal block are written too (the last column tile also covers everything beyond the tiles), so neither
    // output needs clearing beforehand
    double* __restrict__ LinvT = a.LinvT ? a.LinvT[b] : nullptr;
    const int cend = (ct == a.nct - 1) ? Mp : c0 + 64;
    for (int cb = c0; cb < cend; cb += 64)
      for (int idx = tid; idx < NB * 64; idx += 256) {
        const int r = idx >> 6, c = idx & 63, gc = cb + c;
        if (r < nb && gc < Mp) Linv[(long)(j + r) * ld + gc] = (cb == c0 && gc < j + nb) ? Ts[r][c] : 0.0;
      }
    if (LinvT)
      for (int cb = c0; cb < cend; cb += 64)
        for (int idx = tid; idx < NB * 64; idx += 256) {
          const int r = idx & 31, c = idx >> 5, gc = cb + c;   // r fastest: rows of the transpose are contiguous in r
          if (r < nb && gc < Mp) LinvT[(long)gc * ld + j + r] = (cb == c0 && gc < j + nb) ? Ts[r][c] : 0.0;
        }
    return;
  }
  // rows below: Y[rows, cols] -= L[rows,j] Ynew
  const int r0 = below0 + rt * 64;
#pragma unroll
  for (int kk = 0; kk < NB; kk += 4) {
    double avv[2], bvv[2];
#pragma unroll
    for (int x = 0; x < 2; ++x) avv[x] = Ui[wm * 32 + x * 16 + lcol][kk + lrow];
#pragma unroll
    for (int y = 0; y < 2; ++y) bvv[y] = Ts[kk + lrow][wn * 32 + y * 16 + lcol];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(avv[x], bvv[y], acc[x][y], 0, 0, 0);
  }
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int i = r0 + wm * 32 + x * 16 + lrow + 4 * v, gc = c0 + wn * 32 + y * 16 + lcol;
        if (i < Mp && gc < j + nb) Y[(long)i * ld + gc] = old[x][y][v] - acc[x][y][v];
      }
  TR(5)
}

// final factor back over A (lower triangle from Lout, strict upper triangle zero).  grid (Mp, batch)
__global__ void chol_finish_kernel(double* const* __restrict__ Ap, const double* __restrict__ Lout, int Mp, int ld) {
  double* __restrict__ A = Ap[blockIdx.y];
  const double* __restrict__ L = Lout + (long)blockIdx.y * Mp * ld;
  const int i = blockIdx.x;
  for (int c = threadIdx.x; c < Mp; c += blockDim.x) A[(long)i * ld + c] = (c <= i) ? L[(long)i * ld + c] : 0.0;
}

}  // namespace

// Cholesky factor in place (strict upper triangle zeroed) and, when d_Linv != nullptr, inv(L) (+ its transpose).
bool chain_can_ride(const dcgp_ctx* ctx, int Mp, ChainMode mode) {
  return mode.may_ride && Mp <= kChainRhsMaxMp && !ctx->opt.no_rhs_ride;
}

int factor_inverse_batched(dcgp_ctx* ctx, double* const* d_A, double* const* d_Linv, double* const* d_LinvT, int batch,
                           int Mp, int ld, int* d_info, bool defer_finish, const ChainRhs* d_rhs, int max_R, ChainMode mode) {
  if (batch <= 0) return DCGP_OK;
  if (d_rhs && (!d_Linv || !chain_can_ride(ctx, Mp, mode))) return ctx_fail(ctx, DCGP_ERR_ARG, "factorisation chain: right-hand sides cannot ride this route");
  ScopedTimer t(ctx, "factor_chain");
  const size_t mm = (size_t)Mp * ld;
  double* Lout = (double*)ws_get(ctx, "chol_Lout" + ctx->ws_tag, (size_t)batch * mm * sizeof(double));
  double* Y = d_Linv ? (double*)ws_get(ctx, "chol_Y" + ctx->ws_tag, (size_t)batch * mm * sizeof(double)) : nullptr;
  if (!Lout || (d_Linv && !Y)) return DCGP_ERR_ALLOC;
  const int np_la = (Mp + NB - 1) / NB;
  double* Xla = nullptr;   // [np][batch][2][NB][NB]: factor and inverse of every diagonal block, handed from launch to launch
  if (d_Linv && np_la > 1) {
    Xla = (double*)ws_get(ctx, "chol_Xla" + ctx->ws_tag, (size_t)np_la * batch * 2 * NB * NB * sizeof(double));
    if (!Xla) return DCGP_ERR_ALLOC;
  }
  for (int j = 0; j < Mp; j += NB) {
    RlArgs a;
    a.A = d_A; a.Lout = Lout; a.Y = Y; a.Linv = d_Linv; a.LinvT = d_Linv ? d_LinvT : nullptr; a.Mp = Mp; a.ld = ld; a.j = j; a.info = d_info;
    // every number of the launch is plan_launch's (chain_plan.h), which the CPU suite reaches through dcgp_debug_plan_chain
    chain_plan::Query q;
    q.Mp = Mp; q.batch = batch; q.jp = j / NB; q.has_inv = d_Linv != nullptr; q.rides = d_rhs != nullptr; q.max_R = max_R;
    q.alone = mode.alone; q.no_iso = ctx->opt.chain_no_iso != 0;
    const chain_plan::Launch l = chain_plan::plan_launch(q);
    a.nt = l.nt; a.nT = l.nT; a.nct = l.nct; a.la_idx = l.la_idx;
    const size_t slot = (size_t)batch * 2 * NB * NB;
    if (l.has_xin) a.Xin = Xla + (size_t)q.jp * slot;
    if (l.has_xnext) a.Xnext = Xla + (size_t)(q.jp + 1) * slot;
    if (d_rhs) {   // the right-hand sides: panel jp - 1 here, and the last panel too in the last launch
      a.np = l.np; a.Xall = Xla;
      if (l.has_xself) a.Xself = Xla;
      if (l.has_rhs) {
        a.rhs = d_rhs; a.rhs_p = l.rhs_p; a.rhs_last = l.rhs_last; a.rhs_nt = l.rhs_nt; a.rhs_tpw = l.rhs_tpw; a.rhs_nq = l.rhs_nq; a.rhs_base = l.rhs_base;
      }
    }
    a.batch = batch; a.iso_per = l.iso_per;
    // gx == 0: last panel of a plain potrf -- only L_jj is left; one workgroup factors and publishes it
    a.gx_trace = l.gx > 0 ? l.gx : 1;
    hipLaunchKernelGGL(chol_rl_kernel, dim3(l.grid_x, l.grid_y), dim3(256), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
  }
  if (defer_finish) return DCGP_OK;   // inv(L) is complete; the caller copies the factor back (factor_finish_batched) off its critical path
  return factor_finish_batched(ctx, d_A, batch, Mp, ld);
}

// final factor from the chain's scratch back over A (lower triangle; strict upper triangle zeroed)
int factor_finish_batched(dcgp_ctx* ctx, double* const* d_A, int batch, int Mp, int ld) {
  if (batch <= 0) return DCGP_OK;
  auto it = ctx->ws.find("chol_Lout" + ctx->ws_tag);
  if (it == ctx->ws.end()) return ctx_fail(ctx, DCGP_ERR_ARG, "factor_finish: no factorisation to finish");
  hipLaunchKernelGGL(chol_finish_kernel, dim3(Mp, batch), dim3(128), 0, ctx->stream, d_A, (const double*)it->second.first, Mp, ld);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// debugging aid (tests, no device needed): the layout of launch jp of a chain from a flat query, and what every workgroup of its grid decodes to; field
// orders in include/dcgp.h.  The same plan_launch / decode_iso / decode_rhs that factor_inverse_batched and chol_rl_kernel call.
extern "C" int dcgp_debug_plan_chain(const long long* query, int n_query, const long long* R_of, int n_R, long long* plan, int n_plan, long long* wgs,
                                     long n_wgs) {
  using chain_plan::Launch;
  using chain_plan::Query;
  if (!query || !plan || n_query != Query::kFields || n_plan != Launch::kFields) return DCGP_ERR_ARG;
  Query q;
  q.Mp = (int)query[0]; q.batch = (int)query[1]; q.jp = (int)query[2]; q.has_inv = query[3] != 0; q.rides = query[4] != 0; q.max_R = (int)query[5];
  q.alone = query[6] != 0; q.no_iso = query[7] != 0;
  if (q.Mp <= 0 || q.batch <= 0 || q.jp < 0 || q.jp >= chain_plan::panels(q.Mp) || q.max_R < 0) return DCGP_ERR_ARG;
  if (q.rides && (!q.has_inv || q.Mp > kChainRhsMaxMp)) return DCGP_ERR_ARG;   // (factor_inverse_batched refuses these)
  const Launch l = chain_plan::plan_launch(q);
  const long long flat[Launch::kFields] = {l.np, l.j, l.nt, l.nT, l.nct, l.la_idx, l.has_xla, l.has_xin, l.has_xnext, l.has_xself, l.has_rhs, l.rhs_p,
                                           l.rhs_last, l.rhs_nt, l.rhs_tpw, l.rhs_ng, l.rhs_nq, l.rhs_base, l.gx, l.iso_per, l.grid_x, l.grid_y,
                                           l.iso_per > 0, (long long)l.grid_x * l.grid_y};
  for (int e = 0; e < Launch::kFields; ++e) plan[e] = flat[e];
  if (!wgs) return DCGP_OK;
  if (n_wgs != (long)l.grid_x * l.grid_y) return DCGP_ERR_ARG;
  if (l.has_rhs && (!R_of || n_R != q.batch)) return DCGP_ERR_ARG;
  for (int y = 0; y < l.grid_y; ++y)
    for (int x = 0; x < l.grid_x; ++x) {
      long long* o = wgs + ((long)y * l.grid_x + x) * 8;
      for (int e = 0; e < 8; ++e) o[e] = 0;
      o[0] = o[1] = -1;
      int b = y, bx = x;   // chol_rl_kernel's own walk from here on
      if (l.iso_per > 0) {
        const chain_plan::Wg w = chain_plan::decode_iso(x, q.batch, l.iso_per, l.la_idx, l.has_rhs != 0, l.rhs_base);
        if (!w.live) continue;
        b = w.b; bx = w.bx;
      }
      o[0] = b; o[1] = bx;
      if (l.has_rhs && bx >= l.rhs_base) {
        const chain_plan::RhsItem it = chain_plan::decode_rhs(bx - l.rhs_base, (int)R_of[b], l.rhs_nq, l.rhs_p, l.rhs_last, l.rhs_ng);
        if (!it.live) continue;
        o[2] = 5; o[3] = it.q; o[4] = it.ct; o[5] = it.g; o[6] = it.final_only; o[7] = chain_plan::rhs_first_tile(it.g, l.rhs_tpw);
      } else if (bx == l.la_idx) o[2] = 3;
      else if (l.nT == 0 && l.nct == 0) o[2] = 4;
      else if (bx < l.nT) { o[2] = 1; o[4] = bx; }
      else { o[2] = 2; o[3] = (bx - l.nT) / l.nct - 1; o[4] = (bx - l.nT) % l.nct; }
    }
  return DCGP_OK;
}

// conv_fused.hip -- ConvLayer.conditional_ND + Layer.sample_from_conditional of ONE column strip in ONE workgroup
// (conv_gp/layers.py:96-135 -> views.py:40-44, layers.py:23-32, conditionals.py:29-65, layers.py:128-134, reparameterize).
//
// The unfused route passes the [M x P*N'] matrix through HBM three times (K_uf written, A1 = inv(L) K_uf written and read
// back R + 2 times by 128 x 128 tiles, each of which re-stages both operands through LDS behind a barrier per k-tile).
// Here a workgroup owns BN = 16 * FN patch columns for the whole layer:
//   0. the strip's images (at most a few: columns are n*P + p) are staged in LDS, |x_p|^2 per column;
//   1. K_uf[:, strip] from the LDS images (patch gather as MFMA B operand, inducing patches Z^T streamed from L2 as A
//      operand, fp64 exp) straight into the LDS-resident strip [Mp][BN] -- never written to HBM;
//   2. A1 = inv(L) K_uf in place (lower-triangular product; every wave keeps its rows in registers until all waves
//      have read the strip), sum_m A1^2 from the accumulators;
//   3. for r < R: T_r = G_r^T A1 (upper-triangular product), sum_m T_r^2 from the accumulators, T never stored;
//      then mean = alpha^T A1;
//   4. var = Knn - s1 + s2, sample = mean + z sqrt(var + jitter), written in the N x (P*R) layout of layers.py:128-131.
// The B operand of every product is the resident strip; the A operand (inv(L)^T, G_r, alpha, Z^T: a few MB that every
// workgroup reads, L2 / Infinity-Cache resident) goes from global memory STRAIGHT into MFMA A registers: each wave streams
// only the 16 columns of its own row fragment and only its live k-tiles, CF_D tiles ahead -- no LDS staging, no barrier
// inside any k loop (5 barriers per workgroup in all), HBM traffic = the images in and the samples out.
// Row fragments are dealt to the waves boustrophedon (w, 2W-1-w, 2W+w, ...) so that every wave carries the same number
// of live k-tiles of the triangular products.
#include <cstring>
#include <tuple>

#include "fused_plan.h"
#include "head_units_dev.h"
#include "layer.h"
#include "rng.h"

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// the scheduler otherwise sinks each sub-step's LDS reads behind the previous sub-step's MFMAs and into the same registers: one buffer, every
// sub-step waits a full LDS latency (the source order -- reads one sub-step ahead -- is what is meant)
#define CF_SB __builtin_amdgcn_sched_barrier(0)
#define CF_DW 2
#define CF_P1 50
#define CF_P2 75
#define CF_P3 90
constexpr int CF_D_DEFAULT = 3;   // A-operand k-tiles in flight per wave beside the one being multiplied

__device__ __forceinline__ void set_prio(int p) {   // s_setprio takes an immediate
  switch (p) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
  }
}
// i / d for 0 <= i, d < 2^23 without the ~40-instruction integer division (quarter-rate multiplies among them): the float quotient of i + 1/2,
// put right by one step where rounding tipped it over (full-rate 24-bit multiply).  A strip's set-up and epilogue held ~560 VALU instructions of
// divisions per wave -- a third of everything the launch issues outside its MFMAs, and VALU cycles are MFMA cycles on this part.
__device__ __forceinline__ int fdiv(int i, int d, float inv_d) {
  int q = (int)(((float)i + 0.5f) * inv_d);
  const int r = i - (int)__umul24((unsigned)q, (unsigned)d);
  return q + (r >= d ? 1 : 0) - (r < 0 ? 1 : 0);
}
__device__ __forceinline__ int frag_of(int w, int W, int c) { return (c >> 1) * 2 * W + ((c & 1) ? 2 * W - 1 - w : w); }

// phase timestamps for tools/fused_trace.py: [8 sampled workgroups][4 strips of a persistent workgroup][wave][16] shader-clock ticks
#define CF_TR(k) \
  if (tr_slot >= 0 && lane == 0) a.trace[(tr_slot * 16 + wave) * 16 + (k)] = (long long)__builtin_readcyclecounter();

// FN: 16-column fragments per strip.  NS: the W = NT/64 waves form NS teams of TW = W/NS; the row fragments are dealt to the
// TW members of a team (boustrophedon), and the teams split the rest of the work: the columns of the strip in the sweep and in
// the first product (FN/NS fragments each), the outputs r = team, team + NS, ... in the R-batched second product (all FN
// column fragments, so that an A tile is still fetched by exactly one wave).  NS = 2 puts 16 waves = 4 per SIMD on a
// 64-column strip: the fp64 MFMA pipe reaches 92 % of its rate from two waves per SIMD and 98 % from four.
// MAXF: row fragments per wave at most.  ABL: timing experiments only (wrong results): 1 = second product without its
// A-operand loads, 2 = without the LDS reads of the B operand, 4 = two more A tiles in flight.
// BTP: 0 RBF, 1 ArcCosine, 2 RBF on 5 x 5 x 10 patches (the in-kernel sweep walks patch rows; an instance of its own so that the others do not carry its registers),
// 3 Matern32, 4 Matern52 (ArcCosine's route: raw dot products, the norms applied after the sweep)
// HEAD: the launch also carries the rows of the head's patch sweep (a.head_n items behind the last strip item: below).  An instance of its own, launched only where
// fused_plan::plan_head_ride says so: every other launch runs the code it ran before.  HEAD = 2: and behind the rows the rest of the head's sweep (a.tail_n tail
// items; fused_plan::plan_head_tail) -- again an instance of its own, so that the launch that carries rows alone is the code it was.
template <int FN, int NS, int MAXF, int NT, int BTP, int ABL = 0, int HEAD = 0>
__global__ __launch_bounds__(NT) void conv_fused_kernel(ConvFusedArgs a_in) {
  constexpr int BT = BTP == 1 ? 1 : (BTP == 3 ? 2 : (BTP == 4 ? 3 : 0));   // BaseKernel type
  // The arguments are read through the kernarg pointer, which every strip of a persistent workgroup sees as a new value: as a by-value
  // struct the loop-invariant loads of all ~70 words are hoisted out of the strip loop, live across it, and spill (240 VGPRs at 16 waves)
  typedef const __attribute__((address_space(4))) ConvFusedArgs KArgs;
  KArgs* ap = (KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  KArgs& a = *ap;
  constexpr int BN = FN * 16, W = NT / 64, TW = W / NS, FNS = FN / NS, KG = W / FN;
  static_assert(FN % NS == 0 && W % NS == 0 && W % FN == 0, "team split");
  constexpr int CF_D = ((ABL & 4) ? 2 : 0) + (NT >= 1024 ? CF_DW : CF_D_DEFAULT);   // 128-register budget at 16 waves: two tiles ahead
  extern __shared__ __attribute__((aligned(16))) double smem[];

  // A persistent launch (a.persist: one workgroup per slot of the chip): the workgroup walks the strips blockIdx, blockIdx + grid, ...
  // The second workgroup to arrive on a CU holds back for a.stagger ticks of the 100 MHz clock, so that its sweep / first product / epilogue -- the
  // stretches that leave the matrix pipe thin -- fall into the other's second product and the other's into its own, strip after strip.
  int cu_word = -1;
  if (a.persist && a.cu_slots) {
    int* word = reinterpret_cast<int*>(smem);
    if (threadIdx.x == 0) {
      unsigned xcc, hwid;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
      cu_word = (int)(((xcc & 7u) << 7) | ((hwid >> 8) & 0x7fu));   // XCC, SE_ID [15:13], SH_ID [12], CU_ID [11:8]
      word[0] = atomicAdd(a.cu_slots + cu_word, 1);
    }
    __syncthreads();
    const int arrival = word[0];
    __syncthreads();
    if ((arrival & 1) && a.stagger > 0) {
      const long long t0 = wall_clock64();
      while (wall_clock64() - t0 < a.stagger) __builtin_amdgcn_s_sleep(64);
    }
  }
  int strip_next = blockIdx.x;
  if (HEAD || a.pre_n > 0) {   // (head rows: a row's strips must be held by running workgroups, like a prologue's)
    // Prologues ahead: EVERY item, a workgroup's first included, comes off the counter -- an item is then held by a workgroup that is running.  (Dealt by
    // blockIdx, a prologue item could belong to a workgroup that is not resident yet -- the chip shared with another kernel, a CU-masked stream -- while a
    // running one already waits for its A1.)
    int* tk = reinterpret_cast<int*>(smem);
    if (threadIdx.x == 0) tk[0] = atomicAdd(a.dyn, 1);
    __syncthreads();
    strip_next = __builtin_amdgcn_readfirstlane(tk[0]);
    __syncthreads();
  }
  // (a workgroup that starts when every item has been dealt -- more workgroups than CUs it may run on -- has nothing to do but sign off)
  const int first_limit = HEAD ? a.n_items + a.head_n + a.tail_n : (a.pre_n > 0 ? a.n_items : 0x7fffffff);
  for (int it = 0; strip_next < first_limit; ++it) {
  // every strip sees the kernarg pointer and the thread index as new values: nothing of a strip's set-up (argument words, per-lane offsets of every
  // phase) is then loop-invariant, hoisted and kept live across the whole body -- as plain invariants they cost 240 spilled VGPRs at 16 waves
  int tid = threadIdx.x;
  asm volatile("" : "+s"(ap), "+v"(tid));
  KArgs& a = *ap;
  if constexpr (HEAD) {
    // ---- a head row (item a.n_items + row): the head's Kzx units of that row, one Z fragment per wave, by the device code of head_units_kernel itself
    // (head_units_dev.h: a.head is that launch's argument block with one workgroup per row) -- the values go where the head's conditional reads them.
    // The row's input is this layer's sample of the strips that cover its columns: each sets its flag word to the launch's epoch behind its coherent
    // stores.  Head rows are dealt behind every strip item, so a strip a row waits for is an earlier item, held by a workgroup that is running and that
    // waits for nothing a head row produces (the invariant of the A1 hand-over; the same bounded spin, and a row that gave up leaves NaNs).
    // Tail items (behind the a.head_n whole rows; fused_plan.h: plan_head_tail, the same decoding as fused_plan::tail_item): the rest of the head's sweep, so that
    // no sweep launch follows.  Item t < (rows - head_n) parts: part q = t % parts of row head_n + t / parts -- the Z-fragment units [q upp, q upp + upp), one per
    // wave, and behind the last part's units the row's Kdiag chunks.  The head_n items behind those: the Kdiag chunks of a row that rode whole, one per wave.
    // A chunk is the one the stand-alone launch's plan gives the row (a.head.seg[1 ..]: the plan's Kdiag segments -- chunk size, count and first row of
    // each), so its partial sum lands in the same kd slot with the same boundaries.  A tail item waits for its row's strips like a whole row, and the invariant is the same: tail items are dealt behind every strip item and every
    // whole row, the strips they wait for are earlier items held by running workgroups, and no item waits for a head item.
    if (strip_next >= a.n_items) {
      int* tk = reinterpret_cast<int*>(smem + a.lds_main + a.lds_img + BN);
      const int hit = strip_next - a.n_items;
      int row = hit, kz_lo = 0, kz_n = -1, kd = 0;   // kz_n < 0: a whole row, unit (wave + row) % W on every wave
      if (HEAD > 1 && hit >= a.head_n) {
        const int t = hit - a.head_n, n_sub = a.tail_n - a.head_n;
        if (t >= n_sub) { row = t - n_sub; kz_n = 0; kd = 1; }
        else {
          const int j = t, rr = j / a.tail_parts, part = j - rr * a.tail_parts;
          row = a.head_n + rr;
          kz_lo = part * a.tail_upp;
          kz_n = min(a.tail_upp, a.head.nfm - kz_lo);
          kd = part == a.tail_parts - 1 ? 1 : 0;
        }
      }
      if (tid == 0) {
        const int s_hi = (row * a.P + a.P - 1) / BN;
        int ok = 1;
        for (int st = (row * a.P) / BN; st <= s_hi && ok; ++st) {
          ok = 0;
          for (int spin = 0; spin < (1 << 24) && !ok; ++spin) {
            ok = __hip_atomic_load(a.head_flag + st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.head_epoch ? 1 : 0;
            if (!ok) __builtin_amdgcn_s_sleep(2);
          }
        }
        tk[1] = ok;
      }
      __syncthreads();
      if (tk[1]) {
        if constexpr (HEAD > 1) {
        // what this wave runs: (segment, unit) -- segment 0 is the Kzx units, a unit past its segment's count is no work
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
        int sg = 0, u = 0x7fff;
        if (kz_n < 0) u = (wv + row) & (W - 1);
        else if (wv < kz_n) u = kz_lo + wv;
        else if (kd) {
          sg = 1;
          for (int q = 2; q < 6; ++q)
            if (q < a.head.nseg && row >= a.head.seg[q].img0) sg = q;
          u = wv - kz_n;
        }
        head_units_dev::head_units_body<0, 50, 0, NT, true, true>(ap->head, row, sg, u);
        } else {
          head_units_dev::head_units_body<0, 50, 0, NT, true>(ap->head, row);
        }
      } else {
        const int m_lo = kz_n < 0 ? 0 : 16 * kz_lo, m_hi = kz_n < 0 ? a.head.kzx_rows : min(16 * (kz_lo + kz_n), a.head.kzx_rows);
        for (int m = m_lo + tid; m < m_hi; m += NT) a.head.kzx[(long)m * a.head.ldk + row] = __builtin_nan("");
        if (HEAD > 1 && kd && tid < a.head.n_kd) a.head.kd[(long)row * a.head.n_kd + tid] = __builtin_nan("");
      }
      if (tid == 0) tk[0] = atomicAdd(a.dyn, 1);
      __syncthreads();   // (and every wave is done with the row's image)
      strip_next = __builtin_amdgcn_readfirstlane(tk[0]);
      if (strip_next >= first_limit) break;
      continue;
    }
  }
  const int Mp = a.Mp, nf = Mp >> 4, R = a.R;
  const int lane = tid & 63, lrow = lane >> 4, lcol = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % TW, sp = NS == 1 ? 0 : wave / TW;   // member index within the team, team
  double* strip = smem;                                  // [Mp / 4][FN][4][16]: rows in fours (below)
  double* aux = smem + a.lds_main;                       // images of the strip; after phase 1: [TW][BN] partial sums of A1^2
  double* xn = aux + a.lds_img;                          // [BN] |x_p|^2
  int* ticket = reinterpret_cast<int*>(xn + BN);         // persistent launch: the next strip of this workgroup
  int* koff = reinterpret_cast<int*>(xn + BN + 2);       // [Lp]
  const int jmax = a.Kc - 1;
  // row fragments of this wave: frag_of(wm, TW, c), c < nfw
  int nfw = 0;
#pragma unroll
  for (int c = 0; c < MAXF; ++c) nfw += frag_of(wm, TW, c) < nf ? 1 : 0;
  nfw = __builtin_amdgcn_readfirstlane(nfw);
  int fr[MAXF];   // fragments beyond the matrix repeat the first one (their loads stay in range, their results are dropped)
#pragma unroll
  for (int c = 0; c < MAXF; ++c) fr[c] = c < nfw ? frag_of(wm, TW, c) : min(wm, nf - 1);
  // strips of the launch's partial last round are shared by SQ workgroups: each runs phases 0 - 2 and the outputs r = sq, sq + SQ, ...
  int sidx = strip_next, sq = 0, SQ = 1;
  if (sidx >= a.split_first) {
    const int t = sidx - a.split_first;
    SQ = a.split_q;
    sidx = a.split_first + t / SQ;
    sq = t - (sidx - a.split_first) * SQ;
  }
  // Prologues ahead (a.pre_n > 0, a persistent launch whose strips do not fill its last round: DESIGN 4i).  The items of the launch, in the order the
  // counter deals them: the strips [0, pre_first) whole -- one per workgroup of the partial FIRST round --, then pre_n items that run only phases 0 - 2
  // of the strips [pre_first, pre_first + pre_n) and leave A1 (the LDS image of the strip) and the partial sums of A1^2 in a.pre_buf: they fill the
  // first round's spare workgroups; then the remaining strips whole; then the pre_n strips again, which fetch their A1 and go straight to phase 3.
  // Same arithmetic in the same order as a whole strip: bit-identical.
  // Replicas share a prologue (a.pre_D > 0: the rows are a batch of n_mod images tiled, n_mod * P columns = pre_D whole strips, so that strip i shows the images
  // of strip i % pre_D at the same patches: K_uf, A1 and the partial sums of A1^2 are the same numbers).  One item per strip, strip i the i-th the counter deals:
  // the strips below pre_D run whole AND leave their A1 in slot i of a.pre_buf on the way (mode 3), the other strips below pre_whole (the rest of the first
  // round) run whole, every later strip fetches slot i % pre_D.  A slot's writer is an earlier item than any of its readers and waits for nobody.
  bool pre_fail = false;
  int mode = 0, pre_slot = 0;   // 0: a whole strip; 1: phases 0 - 2 only, A1 left in a.pre_buf; 2: A1 fetched from a.pre_buf, phases 3 - 4; 3: whole, A1 left as well
  if (a.pre_D > 0) {
    if (strip_next < a.pre_D) { mode = 3; pre_slot = strip_next; }
    else if (strip_next >= a.pre_whole) { mode = 2; pre_slot = strip_next % a.pre_D; }
  } else if (a.pre_n > 0) {
    if (strip_next >= a.n_strips) {   // (pre_sq > 1: part sq of the strip's SQ, the split of a shared last round applied to a strip whose A1 is fetched)
      mode = 2;
      const int t = strip_next - a.n_strips;
      SQ = a.pre_sq;
      pre_slot = SQ > 1 ? t / SQ : t;
      sq = t - pre_slot * SQ;
      sidx = a.pre_first + pre_slot;
    }
    else if (strip_next >= a.pre_first && strip_next < a.pre_first + a.pre_n) { mode = 1; pre_slot = strip_next - a.pre_first; }
  }
  const int j0 = sidx * BN;
  int tr_slot = -1;
  if (a.trace) {
    const int every = a.persist ? max((int)gridDim.x / 8, 1) : 90;
    if (blockIdx.x % every == 0 && blockIdx.x / every < 8 && it < 4) tr_slot = (blockIdx.x / every) * 4 + it;
  }
  CF_TR(0)
  if (tr_slot >= 0 && lane == 0) a.trace[(tr_slot * 16 + wave) * 16 + 10] = (long long)wall_clock64();
  // Two workgroups share a CU in a persistent launch.  The stretches that cannot fill the matrix pipe by themselves (images, sweep, first product,
  // epilogue: latency- and barrier-bound) issue ahead of the other workgroup's second product, which takes what they leave: at equal or lower
  // priority a sweep beside a second product took 110 us instead of 25 (profiles/r06_fused_persistent_static_trace.txt) while the second product,
  // alone on two waves per SIMD, cannot use more than 81 % of the pipe
  __builtin_amdgcn_s_setprio(3);

  // ---- the A-operand stream ---------------------------------------------------------------------------------------
  // lane (lrow, lcol) of k-substep q of k-tile kt needs Wt[kt*16 + 4q + lrow][16 f + lcol]: per-lane byte offset voff[q],
  // everything else (matrix r, k-tile, fragment) is a scalar byte offset
  unsigned voff[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) voff[q] = (unsigned)(((4 * q + lrow) * Mp + lcol) * 8);
  auto ldw = [&](const __amdgpu_buffer_rsrc_t& rs, int soff, double (&dst)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)voff[q], soff, 0);
      __builtin_memcpy(&dst[q], &v, 8);
    }
  };
  constexpr int QS = 4 * BN;
  if (mode != 2) {
  // ---- phase 0: images of the strip -> LDS, patch-element offsets, |x|^2 per column -----------------------------
  const int n_first = j0 / a.P;
  const int n_last = min(j0 + BN - 1, jmax) / a.P;
  {
    const int total = (n_last - n_first + 1) * a.HWC;
    for (int i0 = 0; i0 < total; i0 += 4 * NT) {
      double t[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + e * NT + tid;
        const int n = fdiv(i, a.HWC, a.inv_HWC), o = i - n * a.HWC;
        const int nn = n_first + n, img = nn - fdiv(nn, a.n_mod, a.inv_nmod) * a.n_mod;
        t[e] = (i < total) ? a.X[(long)img * a.HWC + o] : 0.0;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + e * NT + tid;
        if (i < total) aux[i] = BT == 0 ? t[e] * a.csq : t[e];   // RBF: the sweep's operands carry the kernel's scales (sweep_dev.h)
      }
    }
    if (it == 0)
    for (int l = tid; l < (BT == 0 ? a.Lz : a.Lp); l += NT) {
      const int ll = l < a.L ? l : 0;
      const int c = ll % a.C, t = ll / a.C;
      const int kw = t % a.f, kh = t / a.f;
      koff[l] = (kh * a.W + kw) * a.C + c;
    }
  }
  // LDS offset of the patch of strip column c (columns beyond the matrix repeat the last one: finite, never written out)
  auto patch_off = [&](int c) {
    const int j = min(j0 + c, jmax);
    const int n = fdiv(j, a.P, a.inv_P), p = j - n * a.P;
    const int oh = fdiv(p, a.Wo, a.inv_Wo), ow = p - oh * a.Wo;
    return (n - n_first) * a.HWC + (oh * a.s * a.W + ow * a.s) * a.C;
  };
  // acos, Matern: |z_m|^2 of this lane's accumulator rows: fetched here, needed after the sweep (RBF: the norms ride in the product)
  double znv[BT == 0 ? 1 : MAXF][4];
  if (BT != 0) {
#pragma unroll
    for (int c = 0; c < MAXF; ++c)
#pragma unroll
      for (int v = 0; v < 4; ++v) znv[c][v] = a.zn[16 * fr[c] + lrow + 4 * v];
  }
  __syncthreads();
  if (tid < 8 * BN) {   // 8 threads per column
    const int c = tid >> 3, sub = tid & 7;
    const int pb = patch_off(c);
    double s = 0.0;
    for (int l = sub; l < a.L; l += 8) {
      const double v = aux[pb + koff[l]];
      s = fma(v, v, s);
    }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    if (sub == 0) xn[c] = BT == 0 ? -0.5 * s : s;   // RBF: the column's norm slot, -c |x|^2 / 2 (the image is already scaled)
  }
  __syncthreads();
  CF_TR(1)

  // The strip in LDS: rows in fours, element (row k, column 16 y + i) at (k >> 2) * 4 BN + 64 y + 16 (k & 3) + i: a B fragment (rows k0 .. k0 + 3 by lrow,
  // k0 a multiple of 4; columns 16 y + lcol) is 512 contiguous bytes, lane l at l * 8 -- no bank conflicts, and every address of the kernel is the lane
  // index plus compile-time offsets (column group, sub-step, accumulator row: multiples of 512 bytes, the unit of ds_read2st64_b64) plus a scalar
  // (k-tile).  On gfx950 a VALU instruction issues in the fp64 MFMA's place: the row-major strip with its column groups XOR-swizzled by the row spent
  // 10 - 14 of them per k-tile of the second product on addresses (4 - 5 % of its 1024 MFMA cycles), this one spends 1
  // ---- phase 1: K_uf[:, strip] -> strip: this wave's row fragments x its team's FNS column fragments ----------------
  {
    int pb[FNS];
#pragma unroll
    for (int y = 0; y < FNS; ++y) pb[y] = patch_off((sp * FNS + y) * 16 + lcol);
    const int nk4 = (BT == 0 ? a.Lz : a.Lp) >> 2;
    d4 kacc[MAXF][FNS];
#pragma unroll
    for (int c = 0; c < MAXF; ++c)
#pragma unroll
      for (int y = 0; y < FNS; ++y) kacc[c][y] = d4{0.0, 0.0, 0.0, 0.0};
    // RBF: ZS = sqrt(c) Z^T with the rows (-c |z|^2 / 2 + log2 variance, 1) behind the patch, against columns
    // (sqrt(c) x, 1, -c |x|^2 / 2): the accumulator is log2 of the kernel value (sweep_dev.h, head_units.hip)
    // (through a buffer descriptor: one 32-bit per-lane offset per row fragment, the k sub-step a scalar offset -- as a 64-bit pointer per load the address
    // arithmetic was ~8 VALU instructions per sub-step in the MFMA stream, more than the sub-step's own 4 MFMAs at a long patch)
    const __amdgpu_buffer_rsrc_t zrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(BT == 0 ? a.ZS : a.ZT), 0, nk4 * 4 * Mp * 8, 0x00020000);
    unsigned zoff[MAXF];
#pragma unroll
    for (int c = 0; c < MAXF; ++c) zoff[c] = (unsigned)((lrow * Mp + 16 * fr[c] + lcol) * 8);
    double xnv[FNS];
#pragma unroll
    for (int y = 0; y < FNS; ++y) xnv[y] = xn[(sp * FNS + y) * 16 + lcol];
    constexpr int D4 = 4;
    double ring[D4 + 1][MAXF];
#pragma unroll
    for (int c = 0; c < MAXF; ++c) ring[D4][c] = 0.0;   // (defined on every path: an undefined slot would be carried from strip to strip of a persistent workgroup)
    auto ldz = [&](int k4, double (&dst)[MAXF]) {
#pragma unroll
      for (int c = 0; c < MAXF; ++c) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(zrs, (int)zoff[c], k4 * 4 * Mp * 8, 0);
        __builtin_memcpy(&dst[c], &v, 8);
      }
    };
    auto kstep = [&](int k4, const double (&w)[MAXF]) {
      const int k = 4 * k4 + lrow;
      const int ko = koff[k];
      double bv[FNS];
      if (BT == 0) {
        // slots behind the patch: k == L carries 1, k == L + 1 the column's norm, anything further 0
        const double f_real = k < a.L ? 1.0 : 0.0, f_one = k == a.L ? 1.0 : 0.0, f_nrm = k == a.L + 1 ? 1.0 : 0.0;
#pragma unroll
        for (int y = 0; y < FNS; ++y) bv[y] = fma(aux[pb[y] + ko], f_real, fma(xnv[y], f_nrm, f_one));
      } else {
        const bool kin = k < a.L;
#pragma unroll
        for (int y = 0; y < FNS; ++y) {
          const double v = aux[pb[y] + ko];
          bv[y] = kin ? v : 0.0;
        }
      }
#pragma unroll
      for (int c = 0; c < MAXF; ++c)
#pragma unroll
        for (int y = 0; y < FNS; ++y) kacc[c][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[c], bv[y], kacc[c][y], 0, 0, 0);
    };
    // sub-steps that hold patch elements only (every lane's k < L): the gathered value IS the operand -- the slot selects and the two FMAs per column
    // fragment of the general sub-step are VALU instructions in the MFMA stream (a long patch, L = 250, walks 62 such sub-steps of 63: cfg3's second layer)
    // (the patch-element offsets of a group of sub-steps are read a group ahead: offset -> gather -> MFMA inside one sub-step is two LDS round trips)
    auto kstep_fast = [&](int ko, const double (&w)[MAXF]) {
      double bv[FNS];
#pragma unroll
      for (int y = 0; y < FNS; ++y) bv[y] = aux[pb[y] + ko];
#pragma unroll
      for (int c = 0; c < MAXF; ++c)
#pragma unroll
        for (int y = 0; y < FNS; ++y) kacc[c][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[c], bv[y], kacc[c][y], 0, 0, 0);
    };
    const int nfast = min(a.L >> 2, nk4);
#pragma unroll
    for (int u = 0; u < D4; ++u) ldz(min(u, nk4 - 1), ring[u]);
    // 5 x 5 x 10 patches (a layer behind a 10-map conv layer: cfg3's second layer): f = 5 rows of 50 contiguous image elements, and lane group lrow's element
    // of sub-step s, k = 4 s + lrow, walks a row at +4 doubles per sub-step -- the 12 aligned sub-steps of a row gather at ONE per-lane address per column fragment +
    // immediates, two rows and the sub-step that straddles them are a period of 25 (head_units.hip: the patch-row form of the streamed sweep; same operands into
    // the same MFMAs in the same order).  No offset table, no address per gather.
    if constexpr (BTP == 2) {   // (the launcher checks: f C == 50, f odd, L == f f C)
      constexpr int NA = 12;
      static_assert(D4 + 1 == 5, "the ring of Z sub-steps closes over a period of 25");
      const int RSd = a.W * a.C;                       // doubles from one patch row to the next in the image
      const int sdl = lrow < 2 ? NA * 4 : RSd - 2;     // the straddling sub-step: lane groups 0, 1 end the row, 2, 3 open the next
      int pA[FNS], pS[FNS], pB[FNS];
#pragma unroll
      for (int y = 0; y < FNS; ++y) pA[y] = pb[y] + lrow;
      int sc = 0;
      auto sub = [&](int SL, const int (&base)[FNS], int off) __attribute__((always_inline)) {   // (SL, off: constants once the callers' loops are unrolled)
        ldz(min(sc + D4, nk4 - 1), ring[(SL + D4) % (D4 + 1)]);
        double bv[FNS];
#pragma unroll
        for (int y = 0; y < FNS; ++y) bv[y] = aux[base[y] + off];
#pragma unroll
        for (int c = 0; c < MAXF; ++c)
#pragma unroll
          for (int y = 0; y < FNS; ++y) kacc[c][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(ring[SL][c], bv[y], kacc[c][y], 0, 0, 0);
        ++sc;
      };
      const int nper = (a.f - 1) >> 1;
      for (int tp = 0; tp < nper; ++tp) {
#pragma unroll
        for (int y = 0; y < FNS; ++y) { pS[y] = pA[y] + sdl; pB[y] = pA[y] + (RSd + 2); }
#pragma unroll
        for (int i = 0; i < NA; ++i) sub(i % (D4 + 1), pA, 4 * i);
        sub(NA % (D4 + 1), pS, 0);
#pragma unroll
        for (int i = 0; i < NA; ++i) sub((NA + 1 + i) % (D4 + 1), pB, 4 * i);
#pragma unroll
        for (int y = 0; y < FNS; ++y) pA[y] += 2 * RSd;
      }
#pragma unroll
      for (int i = 0; i < NA; ++i) sub(i % (D4 + 1), pA, 4 * i);
      kstep(nk4 - 1, ring[NA % (D4 + 1)]);             // the last two elements and the two norm slots
    } else {
    int t = 0;
    int kc[D4 + 1], kn[D4 + 1];
#pragma unroll
    for (int u = 0; u <= D4; ++u) kc[u] = koff[4 * min(u, nk4 - 1) + lrow];
    for (; t + D4 + 1 <= nfast; t += D4 + 1) {
#pragma unroll
      for (int u = 0; u <= D4; ++u) kn[u] = koff[4 * min(t + D4 + 1 + u, nk4 - 1) + lrow];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u <= D4; ++u) {
        ldz(min(t + u + D4, nk4 - 1), ring[(u + D4) % (D4 + 1)]);
        kstep_fast(kc[u], ring[u]);
      }
#pragma unroll
      for (int u = 0; u <= D4; ++u) kc[u] = kn[u];
    }
    for (; t + D4 + 1 <= nk4; t += D4 + 1) {
#pragma unroll
      for (int u = 0; u <= D4; ++u) {
        ldz(min(t + u + D4, nk4 - 1), ring[(u + D4) % (D4 + 1)]);
        kstep(t + u, ring[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < D4; ++u)
      if (t + u < nk4) kstep(t + u, ring[u]);
    }
#pragma unroll
    for (int c = 0; c < MAXF; ++c) {
      if (c < nfw) {
        double kv[FNS * 4];   // this fragment's accumulator values: their exponentials interleaved
#pragma unroll
        for (int y = 0; y < FNS; ++y)
#pragma unroll
          for (int v = 0; v < 4; ++v) kv[y * 4 + v] = kacc[c][y][v];
        if (BT == 0) {
          exp2_n<FNS * 4>(kv);
        } else {
          double n1[FNS * 4], n2[FNS * 4];
#pragma unroll
          for (int y = 0; y < FNS; ++y)
#pragma unroll
            for (int v = 0; v < 4; ++v) { n1[y * 4 + v] = xnv[y]; n2[y * 4 + v] = znv[BT == 0 ? 0 : c][v]; }
          BaseKernel bk;
          bk.type = a.bk.type; bk.variance = a.bk.variance; bk.p1 = a.bk.p1; bk.p2 = a.bk.p2;
          bk.template eval_n<BT, FNS * 4>(kv, n1, n2);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int m = 16 * fr[c] + lrow + 4 * v;
#pragma unroll
          for (int y = 0; y < FNS; ++y) strip[(4 * fr[c] + v) * QS + (sp * FNS + y) * 64 + lane] = (m < a.M) ? kv[y * 4 + v] : 0.0;
        }
      }
    }
  }
  CF_TR(2)
  __syncthreads();
  CF_TR(3)
  // training step: the reverse pass reads K_uf and A1 from HBM (k-major [Mp][ldk], column j)
  auto store_strip = [&](double* __restrict__ out) {
    for (int idx = tid; idx < Mp * BN; idx += NT) {
      const int m = idx / BN, c = idx - m * BN;
      const int j = j0 + c;
      if (j <= jmax) out[(long)m * a.ldk + j] = strip[(m >> 2) * QS + (c >> 4) * 64 + (m & 3) * 16 + (c & 15)];
    }
  };
  if (a.Kuf_out && sq == 0) store_strip(a.Kuf_out);

  // ---- phase 2: A1 = inv(L) K_uf (lower-triangular W: fragment f needs k-tiles 0 .. f), FNS column fragments per wave ----
  const __amdgpu_buffer_rsrc_t lrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(a.LinvT), 0, Mp * Mp * 8, 0x00020000);
  d4 a1[MAXF][FNS];
#pragma unroll
  for (int c = 0; c < MAXF; ++c)
#pragma unroll
    for (int y = 0; y < FNS; ++y) a1[c][y] = d4{0.0, 0.0, 0.0, 0.0};
  {
    double s1acc[FNS];
#pragma unroll
    for (int y = 0; y < FNS; ++y) s1acc[y] = 0.0;
    d4 acc[FNS];
    auto ldb = [&](int kt, int q, double (&dst)[FNS]) {
      const double* b = strip + (kt * 4 + q) * QS + lane;
#pragma unroll
      for (int y = 0; y < FNS; ++y) dst[y] = b[(sp * FNS + y) * 64];
    };
    auto mf = [&](double w, const double (&b)[FNS]) {
#pragma unroll
      for (int y = 0; y < FNS; ++y) acc[y] = __builtin_amdgcn_mfma_f64_16x16x4f64(w, b[y], acc[y], 0, 0, 0);
    };
    auto tile = [&](int kt, int kt_next, const double (&w)[4], double (&b0)[FNS]) {
      double b1[FNS], b2[FNS], b3[FNS];
      ldb(kt, 1, b1);
      mf(w[0], b0);
      ldb(kt, 2, b2);
      mf(w[1], b1);
      ldb(kt, 3, b3);
      mf(w[2], b2);
      ldb(kt_next, 0, b0);
      mf(w[3], b3);
    };
#pragma unroll
    for (int c = 0; c < MAXF; ++c) {
      if (c < nfw) {
        const int f = fr[c];
        const int fo = 16 * f * 8;
        const int n1 = f + 1;   // tiles 0 .. f
#pragma unroll
        for (int y = 0; y < FNS; ++y) acc[y] = d4{0.0, 0.0, 0.0, 0.0};
        double ring[CF_D + 1][4], b0[FNS];
#pragma unroll
        for (int q = 0; q < 4; ++q) ring[CF_D][q] = 0.0;
#pragma unroll
        for (int u = 0; u < CF_D; ++u) ldw(lrs, fo + min(u, f) * 16 * Mp * 8, ring[u]);
        ldb(0, 0, b0);
        int kt = 0;
        for (; kt + CF_D + 1 <= n1; kt += CF_D + 1) {   // full groups: no conditionals, the load counters stay exact
#pragma unroll
          for (int u = 0; u <= CF_D; ++u) {
            ldw(lrs, fo + min(kt + u + CF_D, f) * 16 * Mp * 8, ring[(u + CF_D) % (CF_D + 1)]);
            tile(kt + u, min(kt + u + 1, f), ring[u], b0);
          }
        }
#pragma unroll
        for (int u = 0; u < CF_D; ++u) {
          if (kt + u < n1) tile(kt + u, min(kt + u + 1, f), ring[u], b0);
        }
#pragma unroll
        for (int y = 0; y < FNS; ++y) {
          a1[c][y] = acc[y];
#pragma unroll
          for (int v = 0; v < 4; ++v) s1acc[y] = fma(acc[y][v], acc[y][v], s1acc[y]);
        }
      }
    }
    CF_TR(4)
    __syncthreads();   // every wave is done reading K_uf (and the images)
#pragma unroll
    for (int y = 0; y < FNS; ++y) {   // sum over this wave's rows of A1^2, per column: joined over the team in phase 4
      double s = s1acc[y];
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      if (lrow == 0) aux[wm * BN + (sp * FNS + y) * 16 + lcol] = s;
    }
  }
#pragma unroll
  for (int c = 0; c < MAXF; ++c) {
    if (c < nfw) {
#pragma unroll
      for (int y = 0; y < FNS; ++y)
#pragma unroll
        for (int v = 0; v < 4; ++v) strip[(4 * fr[c] + v) * QS + (sp * FNS + y) * 64 + lane] = a1[c][y][v];
    }
  }
  __syncthreads();   // A1 published
  CF_TR(5)
  if (a.A1_out && sq == 0) store_strip(a.A1_out);
  if (mode & 1) {
    // the strip as it lies in LDS and the [TW][BN] partial sums behind it, by coherent (sc1) stores another XCD's loads see (chol_fused.hip: ldg / stg);
    // acknowledged before the barrier in front of the flag
    double* __restrict__ dst = a.pre_buf + (long)pre_slot * a.pre_stride;
    for (int i0 = 0; i0 < Mp * BN; i0 += 8 * NT) {
      double t[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = strip[min(i0 + e * NT + tid, Mp * BN - 1)];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (i0 + e * NT + tid < Mp * BN) __hip_atomic_store(dst + i0 + e * NT + tid, t[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int i = tid; i < TW * BN; i += NT) __hip_atomic_store(dst + Mp * BN + i, aux[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (tid == 0) __hip_atomic_store(a.pre_flag + pre_slot, a.pre_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  } else {
    // ---- A1 of the strip and its partial sums from the workgroup that ran phases 0 - 2 (dealt earlier: it is running or done) ----
    if (tid == 0) {
      // (its holder is running and waits for nobody, so this ends within a prologue's time; bounded all the same -- a launch must not hang the device --
      // and a strip that gave up says so: its samples come out as NaNs)
      int ok = 0;
      for (int spin = 0; spin < (1 << 24) && !ok; ++spin) {
        ok = __hip_atomic_load(a.pre_flag + pre_slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.pre_epoch ? 1 : 0;
        if (!ok) __builtin_amdgcn_s_sleep(2);
      }
      ticket[1] = ok;
    }
    __syncthreads();
    pre_fail = ticket[1] == 0;
    const double* __restrict__ src = a.pre_buf + (long)pre_slot * a.pre_stride;
    for (int i0 = 0; i0 < Mp * BN; i0 += 8 * NT) {
      double t[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = __hip_atomic_load(src + min(i0 + e * NT + tid, Mp * BN - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (i0 + e * NT + tid < Mp * BN) strip[i0 + e * NT + tid] = t[e];
    }
    for (int i = tid; i < TW * BN; i += NT) aux[i] = __hip_atomic_load(src + Mp * BN + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    CF_TR(5)
  }
  if (mode != 1) {

  // ---- phase 3: T_r = G_r^T A1 for r = r0, r0 + rstep, ... (r0 = sp, rstep = NS for a whole strip) (upper-triangular W: fragment f needs k-tiles f .. nf-1): one flat
  // stream over (r, fragment, k-tile), all FN column fragments.  s2 of this wave's i-th output is parked in the lanes with
  // lrow == (i & 3) of keep[i >> 2][.]
  constexpr int KEEP = (16 / NS + 3) / 4;
  double keep[KEEP][FN];
#pragma unroll
  for (int i = 0; i < KEEP; ++i)
#pragma unroll
    for (int y = 0; y < FN; ++y) keep[i][y] = 0.0;
  d4 acc[FN];
#pragma unroll
  for (int y = 0; y < FN; ++y) acc[y] = d4{0.0, 0.0, 0.0, 0.0};
  auto ldb = [&](int kt, int q, double (&dst)[FN]) {
    const double* b = strip + (kt * 4 + q) * QS + lane;
#pragma unroll
    for (int y = 0; y < FN; ++y) dst[y] = (ABL & 2) ? (double)(lane + y + q) : b[y * 64];
  };
  auto mf = [&](double w, const double (&b)[FN]) {
#pragma unroll
    for (int y = 0; y < FN; ++y) acc[y] = __builtin_amdgcn_mfma_f64_16x16x4f64(w, b[y], acc[y], 0, 0, 0);
  };
  // one k-tile: b0 holds sub-step 0 of tile kt on entry and of tile kt_next on exit -- the LDS reads of every sub-step are
  // issued one sub-step ahead of the MFMAs that consume them, across the scalar bookkeeping between two tiles as well
  auto tile = [&](int kt, int kt_next, const double (&w)[4], double (&b0)[FN]) {
    double b1[FN];
    ldb(kt, 1, b1);
    CF_SB;
    mf(w[0], b0);
    CF_SB;
    ldb(kt, 2, b0);
    CF_SB;
    mf(w[1], b1);
    CF_SB;
    ldb(kt, 3, b1);
    CF_SB;
    mf(w[2], b0);
    CF_SB;
    ldb(kt_next, 0, b0);
    CF_SB;
    mf(w[3], b1);
    CF_SB;
  };
  const int r0 = sq + SQ * sp, rstep = SQ * NS;
  const int nr = r0 < R ? (R - 1 - r0) / rstep + 1 : 0;   // outputs of this team
  if (a.G && nfw > 0 && nr > 0) {
    const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(a.G), 0, R * Mp * Mp * 8, 0x00020000);
    int steps_per_r = 0;
    for (int c = 0; c < nfw; ++c) steps_per_r += nf - frag_of(wm, TW, c);
    const int total = nr * steps_per_r;
    // load cursor / compute cursor over the flat sequence of (r, fragment c, k-tile); the load cursor stops on the last tile
    const int f0 = frag_of(wm, TW, 0);
    int lr = r0, lc = 0, lf = f0, lk = f0, lleft = total - 1;
    int ci = 0, cc = 0, ck = f0, cleft = total - 1;
    auto lsoff = [&]() { return ((lr * Mp + lk * 16) * Mp + 16 * lf) * 8; };
    auto ladv = [&]() {
      if (lleft > 0) {
        --lleft;
        if (++lk >= nf) {
          if (++lc == nfw) { lc = 0; lr += rstep; }
          lf = frag_of(wm, TW, lc);
          lk = lf;
        }
      }
    };
    double s2acc[FN];
#pragma unroll
    for (int y = 0; y < FN; ++y) s2acc[y] = 0.0;
    double ring[CF_D + 1][4], b0[FN];
#pragma unroll
    for (int q = 0; q < 4; ++q) ring[CF_D][q] = 0.0;
#pragma unroll
    for (int u = 0; u < CF_D; ++u) { ldw(grs, lsoff(), ring[u]); ladv(); }
    ldb(ck, 0, b0);
    auto step = [&](const double (&w)[4]) {
      const int kcur = ck;
      const bool frag_end = kcur == nf - 1;
      bool r_end = false;
      if (cleft > 0) {   // advance the compute cursor first: the next tile's first B sub-step is fetched under this tile's MFMAs
        --cleft;
        if (frag_end) {
          if (++cc == nfw) { cc = 0; r_end = true; }
          ck = frag_of(wm, TW, cc);
        } else {
          ++ck;
        }
      } else {
        r_end = true;
      }
      tile(kcur, ck, w, b0);
      if (frag_end) {   // fragment done: fold its rows into the column sums of squares
#pragma unroll
        for (int y = 0; y < FN; ++y) {
#pragma unroll
          for (int v = 0; v < 4; ++v) s2acc[y] = fma(acc[y][v], acc[y][v], s2acc[y]);
          // (starting a fragment's first MFMAs from the constant 0 in their C operand instead of these sixteen moves, on a second copy of the
          // k-tile body: +17 us on the cfg2 launch -- profiles/r06_fused_ab.txt)
          acc[y] = d4{0.0, 0.0, 0.0, 0.0};
        }
        if (r_end) {   // output done
#pragma unroll
          for (int y = 0; y < FN; ++y) {
            double s = s2acc[y];
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
#pragma unroll
            for (int i = 0; i < KEEP; ++i) keep[i][y] = ((ci >> 2) == i && (ci & 3) == lrow) ? s : keep[i][y];
            s2acc[y] = 0.0;
          }
          ++ci;
        }
      }
    };
    int t = 0;
    for (; t + CF_D + 1 <= total; t += CF_D + 1) {   // full groups: no conditionals around the loads
      // issue priority falls with progress: the arbiter favours the oldest wave of a SIMD, which then finishes this phase 50 us (of 160) ahead of the
      // youngest and leaves it the pipe to itself at the end; a wave ahead yields.  The steps shorten towards the end (1/2, 3/4, 9/10 of the stream): what the
      // waves of a SIMD differ by when they finish is about half the last step.  cfg2 launch: this schedule 576 us, quarters 3..0 579, thirds 2..0 581
      // (profiles/r06_fused_ab.txt); rotating the priorities per group measured like the quarters, pinning the LDS reads with sched_group_barrier +1 %
      set_prio(100 * t < CF_P1 * total ? 3 : (100 * t < CF_P2 * total ? 2 : (100 * t < CF_P3 * total ? 1 : 0)));
#pragma unroll
      for (int u = 0; u <= CF_D; ++u) {
        if (!(ABL & 1)) ldw(grs, lsoff(), ring[(u + CF_D) % (CF_D + 1)]);
        ladv();
        step(ring[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < CF_D; ++u) {
      if (t + u < total) step(ring[u]);
    }
  }
  __builtin_amdgcn_s_setprio(3);
  CF_TR(6)

  // ---- mean = alpha^T A1: wave (y, g) = (wave % FN, wave / FN) takes column fragment y and the k-tiles g, g + KG, ... -------
  d4 macc = d4{0.0, 0.0, 0.0, 0.0};
  {
    const int y = wave % FN, g = wave / FN;
    const double* __restrict__ al = a.alpha + lcol;
    for (int kt = g; kt < nf; kt += KG) {
      double w[4], b[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        w[q] = al[(long)(kt * 16 + 4 * q + lrow) * a.Rp];
        b[q] = strip[(kt * 4 + q) * QS + y * 64 + lane];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) macc = __builtin_amdgcn_mfma_f64_16x16x4f64(w[q], b[q], macc, 0, 0, 0);
    }
  }
  CF_TR(7)
  __syncthreads();   // the strip is dead: reuse it as [TW][R][BN] s2 | [KG][16][BN] mean partials
  double* s1p = aux;
  double* s2p = smem;
  double* mup = s2p + TW * R * BN;
#pragma unroll
  for (int y = 0; y < FN; ++y) {
    const int c = y * 16 + lcol;
#pragma unroll
    for (int i = 0; i < KEEP; ++i) {
      const int r = r0 + rstep * (4 * i + lrow);
      if (r < R) s2p[(wm * R + r) * BN + c] = keep[i][y];
    }
  }
  {
    const int y = wave % FN, g = wave / FN;
#pragma unroll
    for (int v = 0; v < 4; ++v) mup[(g * 16 + lrow + 4 * v) * BN + y * 16 + lcol] = macc[v];
  }
  __syncthreads();

  CF_TR(8)
  RngMap rmap;
  rmap.W = a.rmap.W; rmap.Nl = a.rmap.Nl; rmap.Ng = a.rmap.Ng; rmap.lo = a.rmap.lo;
  // ---- phase 4: var, mean, sample in the N x (P*R) layout (column j, output r at j*R + r) ----------------------------
  for (int idx = tid; idx < BN * R; idx += NT) {
    const int c = fdiv(idx, R, a.inv_R), r = idx - c * R;
    const int j = j0 + c;
    if (j > jmax || (SQ > 1 && r % SQ != sq)) continue;
    double s1 = 0.0, s2 = 0.0, m = 0.0;
    for (int w = 0; w < TW; ++w) {
      s1 += s1p[w * BN + c];
      s2 += s2p[(w * R + r) * BN + c];
    }
    for (int g = 0; g < KG; ++g) m += mup[(g * 16 + r) * BN + c];
    const double v = (a.knn - s1) + s2;
    if (pre_fail) m = __builtin_nan("");
    if (a.idm && r == 0) {   // Conv2dMean (conv_gp/mean_functions.py:28-41): centre pixel of channel 0 onto map 0
      const int n = j / a.P, p = j - n * a.P;
      const int oh = p / a.Wo, ow = p - oh * a.Wo, c0 = a.f / 2;
      m += a.X[(((long)(n % a.n_mod) * a.H + oh * a.s + c0) * a.W + ow * a.s + c0) * a.C];
    }
    const long e = (long)j * R + r;
    for (int s = 0; s < a.rep; ++s) {
      const long o = (long)s * a.rep_stride + e;
      if (a.out_mean) a.out_mean[o] = m;
      if (a.out_var) a.out_var[o] = v;
      if (a.out_sample) {
        const double zz = a.z ? a.z[o] : philox_normal(a.seed, a.stream_id, rng_index(rmap, o));
        const double smp = m + zz * sqrt(v + a.jitter);
        if constexpr (HEAD) __hip_atomic_store(a.out_sample + o, smp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a head row reads it on another XCD)
        else a.out_sample[o] = smp;
      }
    }
  }
  CF_TR(9)
  }   // mode != 1
  if (tr_slot >= 0 && lane == 0) a.trace[(tr_slot * 16 + wave) * 16 + 11] = (long long)wall_clock64();
  if (!a.persist) break;
  // the next strip: dealt by arrival (a.dyn: one counter per launch) -- two workgroups share a CU and the one launched first wins every arbitration
  // between them, so a fixed deal leaves the other with a strip and a half to run alone at the end (profiles/r06_fused_persistent_static_trace.txt)
  if (tid == 0) ticket[0] = a.dyn ? ((HEAD || a.pre_n > 0) ? 0 : (int)gridDim.x) + atomicAdd(a.dyn, 1) : strip_next + (int)gridDim.x;
  if constexpr (HEAD) __builtin_amdgcn_s_waitcnt(0);   // the strip's samples are acknowledged before the barrier in front of its flag (as the A1 hand-over's)
  __syncthreads();   // (and the partial sums are read: the next strip's images may land on them)
  if constexpr (HEAD) {
    if (mode != 1 && tid == 0) __hip_atomic_store(a.head_flag + sidx, a.head_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  strip_next = __builtin_amdgcn_readfirstlane(ticket[0]);
  if (strip_next >= (HEAD ? first_limit : a.n_items)) break;
  }
  if (threadIdx.x == 0) {
    if (cu_word >= 0) atomicSub(ap->cu_slots + cu_word, 1);
    // the last workgroup to leave puts the counters back for the next launch
    if (ap->persist && ap->dyn && atomicAdd(ap->dyn + 1, 1) == (int)gridDim.x - 1) {
      ap->dyn[1] = 0;
      __threadfence();
      atomicExch(ap->dyn, 0);
    }
  }
}

using fused_plan::kShapes;
using fused_plan::Plan;
using fused_plan::Query;

// one launch of instance BTP (the base kernel's, or the patch-row form of the RBF sweep) of shape I of the table (fused_plan.h)
template <int I, int BTP, int HEAD = 0>
int launch_instance(dcgp_ctx* ctx, const ConvFusedArgs& a, const Plan& p) {
  constexpr int FN = kShapes[I].FN, NS = kShapes[I].NS, MAXF = kShapes[I].MAXF, NT = kShapes[I].NT;
  static bool attr_done[64] = {};   // (per instance)   // per device: a second ctx on another device of this process needs the opt-in too
  const int dv = ctx->device >= 0 && ctx->device < 64 ? ctx->device : 0;
  if (!attr_done[dv]) {   // more than 64 KB of dynamic LDS needs the opt-in
    hipFuncSetAttribute((const void*)conv_fused_kernel<FN, NS, MAXF, NT, BTP, 0, HEAD>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_done[dv] = true;
  }
  hipLaunchKernelGGL((conv_fused_kernel<FN, NS, MAXF, NT, BTP, 0, HEAD>), dim3((unsigned)p.grid), dim3(NT), (size_t)p.lds, ctx->stream, a);
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}
template <int I>
int launch_fused(dcgp_ctx* ctx, const ConvFusedArgs& a, const Plan& p) {
  if (a.head_n > 0 || a.tail_parts > 0) {   // head rows ride: the 64-column strip on 16 waves, RBF (plan_head_ride admits nothing else)
    if constexpr (I == 0) {
      if (!p.patch_rows && a.bk.type == 0) return a.tail_parts > 0 ? launch_instance<0, 0, 2>(ctx, a, p) : launch_instance<0, 0, 1>(ctx, a, p);
    }
    return ctx_fail(ctx, DCGP_ERR_ARG, "conv_fused: head rows on a launch that cannot carry them (shape %d)", I);
  }
  switch (p.patch_rows ? -1 : a.bk.type) {
    case 0: return launch_instance<I, 0>(ctx, a, p);
    case 1: return launch_instance<I, 1>(ctx, a, p);
    case 2: return launch_instance<I, 3>(ctx, a, p);
    case 3: return launch_instance<I, 4>(ctx, a, p);
    case -1:   // (the patch-row instance only where such layers run, the 64-column strip on 16 waves: the plan asks for it nowhere else)
      if constexpr (I == 0) return launch_instance<I, 2>(ctx, a, p);
      [[fallthrough]];
    default: return ctx_fail(ctx, DCGP_ERR_ARG, "conv_fused: unknown base kernel type %d", a.bk.type);
  }
}

// the question a layer launch asks the plan: filled here and nowhere else, for conv_fused_ok() and for conv_fused()
Query fused_query(const dcgp_ctx* ctx, const ConvFusedArgs& a) {
  const DcgpOptions& o = ctx->opt;
  Query q;
  q.Mp = a.Mp; q.M = a.M; q.R = a.R; q.Rp = a.Rp; q.Kc = a.Kc; q.P = a.P; q.HWC = a.HWC; q.L = a.L; q.Lp = a.Lp; q.Lz = a.Lz; q.f = a.f; q.C = a.C;
  q.n_mod = a.n_mod; q.rep = a.rep; q.base = a.bk.type;
  q.has_G = a.G != nullptr; q.keeps_state = a.Kuf_out || a.A1_out; q.has_trace = ctx->fused_trace != nullptr; q.n_cus = ctx->n_cus;
  q.fused_shape = o.fused_shape; q.fused_large = o.fused_large; q.fused_split = o.fused_split; q.fused_persist = o.fused_persist; q.fused_pre = o.fused_pre;
  q.fused_parts = o.fused_parts; q.fused_rep_share = o.fused_rep_share; q.fused_wgs = o.fused_wgs; q.fused_stagger = o.fused_stagger;
  q.sweep_no_rows = o.sweep_no_rows;
  return q;
}

// A workspace of the ctx that the kernel leaves zeroed behind every launch: cleared on the stream when it is new, has grown, or `clear` says so
template <class T>
int ws_zeroed(dcgp_ctx* ctx, const char* name, size_t bytes, T** out, bool clear = false, bool* cleared = nullptr) {
  const auto it = ctx->ws.find(name);
  clear = clear || it == ctx->ws.end() || it->second.second < bytes;
  *out = static_cast<T*>(ws_get(ctx, name, bytes));
  if (!*out) return DCGP_ERR_ALLOC;
  if (clear) HIP_TRY(ctx, hipMemsetAsync(*out, 0, ctx->ws[name].second, ctx->stream));
  if (cleared) *cleared = clear;
  return DCGP_OK;
}

}  // namespace

// debugging aid (tools/fused_trace.py): device buffer of 8 x 4 x 16 x 16 int64 ([sampled workgroup][strip of a persistent one][wave][stamp]) that the fused
// layer kernel stamps its phases into
extern "C" int dcgp_debug_set_fused_trace(dcgp_ctx* ctx, long long* buf_dev) {
  if (!ctx) return DCGP_ERR_ARG;
  ctx->fused_trace = buf_dev;   // per ctx: goes away with it (nullptr switches the stamps off)
  return DCGP_OK;
}

// debugging aid (tests): how the most recent layer-kernel launch of the ctx was dealt -- out4 = {persistent workgroups (0: one workgroup per strip), items the
// counter deals, hand-over slots, distinct strips D whose prologues the replicas share (0: not shared)}
extern "C" int dcgp_debug_fused_plan(dcgp_ctx* ctx, int* out4) {
  if (!ctx || !out4) return DCGP_ERR_ARG;
  const Plan& p = ctx->last_fused_plan;
  out4[0] = p.persist; out4[1] = p.n_items; out4[2] = p.pre_n; out4[3] = p.pre_D;
  return DCGP_OK;
}

// debugging aid (tests): {head rows the most recent layer-kernel launch of the ctx carried, launches of the ctx that carried any}
extern "C" int dcgp_debug_head_ride(dcgp_ctx* ctx, long long* out2) {
  if (!ctx || !out2) return DCGP_ERR_ARG;
  out2[0] = ctx->last_head_rows; out2[1] = ctx->head_ride_launches;
  return DCGP_OK;
}

// debugging aid (tests, no device needed): fused_plan::plan_head_ride for the launch plan_layer_launch gives the flat query, and where head row `row` sits in
// the deal: out[8] = {ok, why (fused_plan::RideWhy), head rows, item of row 0, item of `row`, first and last strip of `row`, the latest item that writes
// samples of `row`}
extern "C" int dcgp_debug_plan_head_ride(const long long* query, int n_query, const long long* ride, int n_ride, long long row, long long* out, int n_out) {
  if (!query || !ride || !out || n_query != Query::kFields || n_ride != fused_plan::RideQuery::kFields || n_out != 8) return DCGP_ERR_ARG;
  Query q;
  std::apply([&](auto&... f) { ((f = (long)*query++), ...); }, Query::fields(q));
  fused_plan::RideQuery r;
  r.next_is_head = ride[0]; r.head_form = ride[1]; r.head_HWC = ride[2]; r.head_lds = ride[3]; r.head_nfm = ride[4]; r.in_flight = ride[5]; r.chain_beside = ride[6];
  r.head_ride = ride[7];
  const Plan p = fused_plan::plan_layer_launch(q);
  const fused_plan::Ride rd = fused_plan::plan_head_ride(q, p, r);
  long lo = 0, hi = -1, last = -1;
  if (rd.ok && row >= 0 && row < rd.n_rows) {
    fused_plan::ride_row_strips(row, q.P, kShapes[p.shape].FN * 16, &lo, &hi);
    for (long st = lo; st <= hi; ++st) last = std::max(last, fused_plan::ride_sample_item(p, st));
  }
  const long long flat[8] = {rd.ok, rd.why, rd.n_rows, rd.first_item, rd.ok ? rd.first_item + row : -1, lo, hi, last};
  memcpy(out, flat, sizeof flat);
  return DCGP_OK;
}

// debugging aid (tests): {Kdiag items, sub-row items, sub-row items per row of the head's tail that the most recent layer-kernel launch of the ctx carried,
// head sweep launches the ctx has skipped because a layer launch had run the whole sweep}
extern "C" int dcgp_debug_head_tail(dcgp_ctx* ctx, long long* out4) {
  if (!ctx || !out4) return DCGP_ERR_ARG;
  out4[0] = ctx->last_tail_kd; out4[1] = ctx->last_tail_sub; out4[2] = ctx->last_tail_parts; out4[3] = ctx->head_sweeps_skipped;
  return DCGP_OK;
}

// debugging aid (tests, no device needed): fused_plan::plan_head_tail for the launch plan_layer_launch gives the flat query, and what tail item `item` (0: the
// first behind the whole rows) is: out[14] = {ok, why (fused_plan::TailWhy), whole rows, parts, units per part, item index of tail item 0, tail items, then of
// `item`: row, first unit, end unit, carries the row's Kdiag chunks, first and last strip of the row, the latest item that writes samples of the row}
extern "C" int dcgp_debug_plan_head_tail(const long long* query, int n_query, const long long* ride, int n_ride, const long long* tail, int n_tail, long long item,
                                         long long* out, int n_out) {
  if (!query || !ride || !tail || !out || n_query != Query::kFields || n_ride != fused_plan::RideQuery::kFields || n_tail != fused_plan::TailQuery::kFields || n_out != 14)
    return DCGP_ERR_ARG;
  Query q;
  std::apply([&](auto&... f) { ((f = (long)*query++), ...); }, Query::fields(q));
  fused_plan::RideQuery r;
  r.next_is_head = ride[0]; r.head_form = ride[1]; r.head_HWC = ride[2]; r.head_lds = ride[3]; r.head_nfm = ride[4]; r.in_flight = ride[5]; r.chain_beside = ride[6];
  r.head_ride = ride[7];
  fused_plan::TailQuery t;
  t.head_ride_tail = tail[0]; t.n_kd = tail[1];
  const Plan p = fused_plan::plan_layer_launch(q);
  const fused_plan::Tail tl = fused_plan::plan_head_tail(q, p, r, t);
  fused_plan::TailItem ti{-1, 0, 0, 0};
  long lo = 0, hi = -1, last = -1;
  if (tl.ok && item >= 0 && item < tl.n_items) {
    ti = fused_plan::tail_item(tl, r.head_nfm, item);
    fused_plan::ride_row_strips(ti.row, q.P, kShapes[p.shape].FN * 16, &lo, &hi);
    for (long st = lo; st <= hi; ++st) last = std::max(last, fused_plan::ride_sample_item(p, st));
  }
  const long long flat[14] = {tl.ok, tl.why, tl.n_rows, tl.parts, tl.upp, tl.first_item, tl.n_items, ti.row, ti.kz_lo, ti.kz_hi, ti.kd, lo, hi, last};
  memcpy(out, flat, sizeof flat);
  return DCGP_OK;
}

// debugging aid (tests, no device needed): the plan of a layer launch from a flat query; field orders in include/dcgp.h
extern "C" int dcgp_debug_plan_layer_launch(const long long* query, int n_query, long long* plan, int n_plan) {
  if (!query || !plan || n_query != Query::kFields || n_plan != Plan::kFields) return DCGP_ERR_ARG;
  Query q;
  auto fields = Query::fields(q);
  static_assert(std::tuple_size<decltype(fields)>::value == Query::kFields, "the flat query covers every field");
  std::apply([&](auto&... f) { ((f = (long)*query++), ...); }, fields);
  const Plan p = fused_plan::plan_layer_launch(q);
  long long units[3];
  const double u[3] = {p.units_plain, p.units_ahead, p.units_shared};
  memcpy(units, u, sizeof units);
  const long long flat[Plan::kFields] = {p.ok, p.shape, p.lds, p.lds_main, p.lds_img, p.grid, p.persist, p.n_strips, p.n_items, p.deal, p.split_first, p.split_q,
                                         p.pre_n, p.pre_first, p.pre_sq, p.pre_D, p.pre_whole, p.pre_stride, p.stagger, p.cu_slots, p.patch_rows,
                                         units[0], units[1], units[2]};
  memcpy(plan, flat, sizeof flat);
  return DCGP_OK;
}

bool conv_fused_ok(const dcgp_ctx* ctx, const ConvFusedArgs& a) {
  // no_fused_layer: A/B switch (tests flip it through dcgp_ctx_set_option): the unfused sweep + GEMM route
  return !ctx->opt.no_fused_layer && fused_plan::plan_layer_launch(fused_query(ctx, a)).ok;
}

int conv_fused_rides_head(const dcgp_ctx* ctx, const ConvFusedArgs& a, bool keeps_state, bool head_form, long head_HWC, long head_lds, long head_nfm, bool in_flight,
                           bool chain_beside) {
  if (ctx->opt.no_fused_layer) return 0;
  Query q = fused_query(ctx, a);
  q.keeps_state = keeps_state;
  fused_plan::RideQuery r;
  r.next_is_head = 1; r.head_form = head_form; r.head_HWC = head_HWC; r.head_lds = head_lds; r.head_nfm = head_nfm; r.in_flight = in_flight;
  r.chain_beside = chain_beside; r.head_ride = ctx->opt.head_ride;
  return fused_plan::plan_head_ride(q, fused_plan::plan_layer_launch(q), r).n_rows;
}

int conv_fused_head_tail(const dcgp_ctx* ctx, const ConvFusedArgs& a, bool keeps_state, bool head_form, long head_HWC, long head_lds, long head_nfm, long head_n_kd,
                         bool in_flight, bool chain_beside, int* n_rows) {
  *n_rows = 0;
  if (ctx->opt.no_fused_layer) return 0;
  Query q = fused_query(ctx, a);
  q.keeps_state = keeps_state;
  fused_plan::RideQuery r;
  r.next_is_head = 1; r.head_form = head_form; r.head_HWC = head_HWC; r.head_lds = head_lds; r.head_nfm = head_nfm; r.in_flight = in_flight;
  r.chain_beside = chain_beside; r.head_ride = ctx->opt.head_ride;
  fused_plan::TailQuery t;
  t.head_ride_tail = ctx->opt.head_ride_tail; t.n_kd = head_n_kd;
  const fused_plan::Tail tail = fused_plan::plan_head_tail_memo(q, r, t);
  if (!tail.ok) return 0;
  *n_rows = tail.n_rows;
  return tail.parts;
}

int conv_fused(dcgp_ctx* ctx, const ConvFusedArgs& a_in) {
  if (a_in.Kc <= 0) return DCGP_OK;
  const Plan p = fused_plan::plan_layer_launch(fused_query(ctx, a_in));
  if (!p.ok) return ctx_fail(ctx, DCGP_ERR_ARG, "conv_fused: layer shape not supported (M = %d, R = %d)", a_in.M, a_in.R);
  // The workspaces the plan asks for.  ONE counter pair, one hand-over area and one set of arrival counters per ctx: the code relies on a ctx's layer
  // launches being serialised on one main stream (a step on the other main stream starts behind the previous one's end, model.hip)
  ConvFusedArgs a = a_in;
  if (p.deal == fused_plan::kCounter) DCGP_TRY(ws_zeroed(ctx, "fused_dyn", 2 * sizeof(int), &a.dyn));
  if (p.pre_n > 0) {
    a.pre_buf = static_cast<double*>(ws_get(ctx, "fused_pre_buf", (size_t)p.pre_n * p.pre_stride * sizeof(double)));
    if (!a.pre_buf) return DCGP_ERR_ALLOC;
    bool cleared = false;   // flags compare equal to the launch's epoch: a fresh (or wrapped) area starts from zero
    DCGP_TRY(ws_zeroed(ctx, "fused_pre_flag", (size_t)p.pre_n * sizeof(unsigned), &a.pre_flag, ctx->fused_pre_epoch == 0xffffffffu, &cleared));
    if (cleared) ctx->fused_pre_epoch = 0;
    a.pre_epoch = ++ctx->fused_pre_epoch;
  }
  if (p.cu_slots) DCGP_TRY(ws_zeroed(ctx, "fused_cu_slots", 1024 * sizeof(int), &a.cu_slots));
  ctx->last_head_rows = 0;
  ctx->last_tail_kd = ctx->last_tail_sub = ctx->last_tail_parts = 0;
  a.tail_n = a.tail_upp = 0;
  if (a.tail_parts > 0) {
    // The head's whole sweep rides (fused_plan::plan_head_tail, asked again about the launch itself): `head` becomes segment 0 = the Kzx units and, behind it, the
    // Kdiag segments of the sweep launch's own plan -- a chunk has the boundaries and the slot it has there.
    fused_plan::RideQuery rq;
    rq.next_is_head = 1; rq.head_form = 1; rq.head_HWC = a.head.HWC; rq.head_lds = (long)head_units_lds(a.head); rq.head_nfm = a.head.nfm;
    rq.head_ride = ctx->opt.head_ride;
    fused_plan::TailQuery tq;
    tq.head_ride_tail = ctx->opt.head_ride_tail; tq.n_kd = a.head.n_kd;
    const fused_plan::Tail tail = fused_plan::plan_head_tail_memo(fused_query(ctx, a_in), rq, tq);
    if (!tail.ok || tail.n_rows != a.head_n || tail.parts != a.tail_parts || a.head.X != a.out_sample || a.head.N != a_in.Kc / a_in.P || a.head.n_mod < a.head.N ||
        a.head.n0 != 0 || !a.head.kzx || !a.head.kd || a.head.kuf || a.head.kfull || a.head.trace)
      return ctx_fail(ctx, DCGP_ERR_ARG, "conv_fused: the launch cannot carry the head's sweep (reason %d)", tail.why);
    HuSeg segs[6];
    int ns = 1, next_img = 0;
    for (int g = 0; g < a.head.nseg; ++g) {
      const HuSeg& s = a.head.seg[g];
      if (s.kind != 1) continue;
      if (ns >= 6 || s.img0 != next_img || s.upw != 1 || s.C < 1 || s.C > a.head.n_kd || s.T < 1)
        return ctx_fail(ctx, DCGP_ERR_ARG, "conv_fused: the head's Kdiag segments are not the plan the tail items were written for");
      segs[ns] = s;
      next_img = g + 1 < a.head.nseg ? a.head.seg[g + 1].img0 : a.head.N;   // (segments of one kind follow each other: the next one's first row ends this one)
      ++ns;
    }
    if (ns < 2) return ctx_fail(ctx, DCGP_ERR_ARG, "conv_fused: the head's sweep has no Kdiag chunks to carry");
    segs[0] = HuSeg{};
    a.head.nseg = ns;
    for (int g = 0; g < ns; ++g) a.head.seg[g] = segs[g];
    a.head.n_wgs = a.head_n + tail.n_items; a.head.upw = 1;
    a.tail_n = tail.n_items; a.tail_upp = tail.upp;
    bool cleared = false;
    DCGP_TRY(ws_zeroed(ctx, "fused_head_flag", (size_t)p.n_strips * sizeof(unsigned), &a.head_flag, ctx->fused_head_epoch == 0xffffffffu, &cleared));
    if (cleared) ctx->fused_head_epoch = 0;
    a.head_epoch = ++ctx->fused_head_epoch;
    ctx->last_head_rows = a.head_n;
    ctx->last_tail_kd = a.head_n; ctx->last_tail_sub = tail.n_items - a.head_n; ctx->last_tail_parts = tail.parts;
    ++ctx->head_ride_launches;
  } else if (a.head_n > 0) {
    // Head rows ride (decided by the step's plan through fused_plan::plan_head_ride; asked again here about the launch itself: a launch that cannot carry
    // them is refused, not run without them).  `head` becomes a launch plan of one workgroup per row that runs the row's Kzx units, one per wave.
    fused_plan::RideQuery rq;
    rq.next_is_head = 1; rq.head_form = 1; rq.head_HWC = a.head.HWC; rq.head_lds = (long)head_units_lds(a.head); rq.head_nfm = a.head.nfm;
    rq.head_ride = ctx->opt.head_ride;
    const fused_plan::Ride ride = fused_plan::plan_head_ride(fused_query(ctx, a_in), p, rq);
    if (!ride.ok || ride.n_rows != a.head_n || a.head.X != a.out_sample || a.head.N != a_in.Kc / a_in.P || a.head.n_mod < a.head.N || a.head.n0 != 0 || !a.head.kzx ||
        a.head.kuf || a.head.kfull || a.head.trace)
      return ctx_fail(ctx, DCGP_ERR_ARG, "conv_fused: the launch cannot carry the head's rows (reason %d)", ride.why);
    a.head.kd = nullptr; a.head.want_kd = 0;
    a.head.nseg = 1; a.head.seg[0] = HuSeg{}; a.head.n_wgs = a.head_n; a.head.upw = 1;
    bool cleared = false;
    DCGP_TRY(ws_zeroed(ctx, "fused_head_flag", (size_t)p.n_strips * sizeof(unsigned), &a.head_flag, ctx->fused_head_epoch == 0xffffffffu, &cleared));
    if (cleared) ctx->fused_head_epoch = 0;
    a.head_epoch = ++ctx->fused_head_epoch;
    ctx->last_head_rows = a.head_n;
    ++ctx->head_ride_launches;
  }
  // the plan into the argument block
  a.lds_main = p.lds_main; a.lds_img = p.lds_img;
  a.split_first = p.split_first; a.split_q = p.split_q;
  a.persist = p.persist; a.n_strips = p.n_strips; a.n_items = p.n_items; a.stagger = p.stagger;
  a.pre_n = p.pre_n; a.pre_first = p.pre_first; a.pre_sq = p.pre_sq; a.pre_stride = p.pre_stride; a.pre_D = p.pre_D; a.pre_whole = p.pre_whole;
  a.trace = ctx->fused_trace;
  a.no_rows = ctx->opt.sweep_no_rows ? 1 : 0;
  a.inv_HWC = 1.0f / (float)a.HWC; a.inv_nmod = 1.0f / (float)a.n_mod; a.inv_P = 1.0f / (float)a.P; a.inv_Wo = 1.0f / (float)a.Wo; a.inv_R = 1.0f / (float)a.R;
  ctx->last_fused_plan = p;
  ScopedTimer t(ctx, "conv_fused");
#ifdef DCGP_EXPERIMENTS
  const int abl = (int)ctx->opt.fused_abl;   // timing build only (make EXPERIMENTS=1): wrong results
  if (abl && p.shape == 0 && a.bk.type == 0) {
    const unsigned grid = (unsigned)((a.Kc + 63) / 64);
#define CF_ABL(X)                                                                                                                       \
  case X:                                                                                                                               \
    hipFuncSetAttribute((const void*)conv_fused_kernel<4, 2, 2, 1024, 0, X>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
    hipLaunchKernelGGL((conv_fused_kernel<4, 2, 2, 1024, 0, X>), dim3(grid), dim3(1024), (size_t)p.lds, ctx->stream, a);               \
    break;
    switch (abl) { CF_ABL(1) CF_ABL(2) CF_ABL(3) CF_ABL(4) default: return ctx_fail(ctx, DCGP_ERR_ARG, "conv_fused: unknown DCGP_FUSED_ABL value %d", abl); }
#undef CF_ABL
    LAUNCH_CHECK(ctx);
    return DCGP_OK;
  }
#endif
  static_assert(fused_plan::kNumShapes == 8, "one case per row of the shape table");
  switch (p.shape) {
    case 0: return launch_fused<0>(ctx, a, p);
    case 1: return launch_fused<1>(ctx, a, p);
    case 2: return launch_fused<2>(ctx, a, p);
    case 3: return launch_fused<3>(ctx, a, p);
    case 4: return launch_fused<4>(ctx, a, p);
    case 5: return launch_fused<5>(ctx, a, p);
    case 6: return launch_fused<6>(ctx, a, p);
    default: return launch_fused<7>(ctx, a, p);
  }
}

// head_units.hip -- ConvKernel.Kzx and ConvKernel.Kdiag of the head (conv_gp/kernels.py:106-133) in one launch,
// cut into equal WAVE-sized units.
//
// What bounds these sweeps on gfx950 (tools/pipe_mix.hip, profiles/r03_pipe_mix.txt): v_mfma_f64_16x16x4_f64 and every
// VALU instruction of a SIMD issue one after the other -- 64 cycles per MFMA, 4.4 per fp64 FMA, no overlap even across
// waves.  A 16 x 16 tile of kernel values at patch length L costs ceil((L+2)/4) MFMAs plus, per value, whatever the
// epilogue spends in the VALU, so the epilogue's instruction count is as much the kernel as the products are:
//   * both operands arrive scaled by sqrt(log2(e))/lengthscale, and the two free slots behind a patch (L = 25 or 250
//     pads to 28 / 252) carry (-|z|^2/2 + log2 variance, 1) against (1, -|x|^2/2): the MFMA accumulator IS the base-2
//     exponent of the kernel value, no norm / scale arithmetic per value;
//   * 2^t by a magic-number split (t + 1.5*2^52: integer part in the low mantissa word, no v_rndne / v_cvt), a
//     degree-11 minimax polynomial on [-1/2, 1/2] (11 FMAs with scalar coefficient operands; |error| 2e-17) and
//     v_ldexp_f64: 16 VALU instructions per value with the clamp, 17 with its weighted accumulation (the previous
//     epilogue: 29 and 8 hazard nops);
//   * chains of 8 values interleaved, so no dependent fp64 pair is adjacent (no s_nop).
// Work decomposition: per image, one unit per 16-row fragment of Z (its Kzx row sums over all patches) and one per
// PAIR of fragment rows (i, nf-1-i) of the symmetric patch Gram matrix (tiles on and right of the diagonal, off-diagonal
// tiles counted twice) -- nf or nf+1 tile products each.  A workgroup is 4 waves = 4 units of one image behind ONE
// image load and one pass of patch norms; waves never synchronise after that.  ~11 000 units at the headline size, so
// the tail of the launch is one unit (~10 us) whatever the image count is relative to 256 CUs.
#include "common.h"
#include <cmath>
#include <type_traits>

#include "head_units_dev.h"

namespace {

template <int NK4, int TL, int WMODE, int NT>
// (aligned(4096): the streamed forms are 40-50 KB of mostly straight-line code and their speed depends on where the code object puts them -- the same binary of the
// 5 x 5 x 10 head's sweep measured 70.7-71.9 us at one 256-byte-aligned address and 67.7-68.2 at another; page-aligned it is the latter wherever it lands)
__global__ __attribute__((aligned(4096))) __launch_bounds__(NT, WMODE == 2 ? 2 : ((WMODE == 1 || WMODE == 3) ? 3 : HU_WAVES)) void head_units_kernel(HeadUnitsArgs a_in) {
  head_units_dev::head_units_body<NK4, TL, WMODE, NT>(*(const __attribute__((address_space(4))) HeadUnitsArgs*)__builtin_amdgcn_kernarg_segment_ptr(), (int)blockIdx.x);
}

}  // namespace

size_t head_units_lds(const HeadUnitsArgs& a) {
  return (size_t)(((a.HWC + 1) & ~1) + 2 * a.nfp * 16 + ((a.H * (a.W - a.f + 1) + 1) & ~1)) * sizeof(double) +
         (size_t)(a.nfp * 16 + ((a.Lq + 1) & ~1)) * sizeof(int) +
         (((a.L == 25 || a.L == 16 || a.L == 48) && !a.stream_k) ? 256 * sizeof(double) : 0);   // the register-resident forms' table of 2^(j / 256)
}

bool head_units_ok(const HeadUnitsArgs& a) {
  if (a.kuf) {
    // the stores' 32-bit offsets: per lane (15 rows + 15 patches), per fragment + replica (scalar)
    const long lane_max = (15 * a.sM + 15 * a.sP) * 8, uni_max = ((long)(a.nfp + 1) * 16 * a.sP + (long)a.N * a.sN) * 8;
    if (lane_max >= (1L << 31) || uni_max >= (1L << 31)) return false;
  }
  if (a.kfull && (15 * a.kf_sM + 15) * 8 + (long)(a.nfp + 1) * 128 >= (1L << 31)) return false;
  return head_units_lds(a) <= 54 * 1024 && (long)a.Lq * a.Mp * 8 < (1L << 31);
}

// fills the derived fields of `a` (fragment counts, units per image)
void head_units_plan(HeadUnitsArgs* a) {
  a->HWC = a->H * a->W * a->C;
  a->nfm = a->Mp / 16;
  a->nfp = (a->P + 15) / 16;
  if (a->kzx_rows <= 0) a->kzx_rows = a->Mp;
  a->inv_C = 1.0f / (float)a->C; a->inv_f = 1.0f / (float)a->f; a->inv_Wo = 1.0f / (float)a->Wo; a->inv_Wr = 1.0f / (float)(a->W - a->f + 1);
  a->nseg = 0; a->n_wgs = 0; a->n_kd = 0; a->upw = 1; a->n_base = a->N;
  // waves per workgroup: 4 where the patch fits registers (one set-up for four long units); 2 for long patches on small views
  // (a 12 x 12 x 10 head input: units of 252 MFMAs, short beside the set-up they sit behind)
  a->wpg = (a->L == 25 || a->kuf || a->nfp > 8) ? 4 : 2;
  auto push = [&](int kind, int n_img, int wpi, int T, int C, int upw = 1) {
    if (n_img <= 0 || a->nseg >= 6) return;
    HuSeg& g = a->seg[a->nseg++];
    g.wg0 = (int)a->n_wgs; g.img0 = 0; g.wpi = wpi; g.kind = kind; g.T = T; g.C = C; g.upw = upw;
    a->n_wgs += (long)n_img * wpi;
  };
  // Occupancy shaping.  Workgroups are handed out as slots free up, so a launch of r = waves / resident slots rounds costs ceil(r)
  // rounds' worth of time when r is small: 6016 equal units on 4096 slots (4 waves per SIMD) are a full round and then a round at 47 %
  // occupancy that lasts almost as long (tools/sweep_trace.py: 74 us for 41 us of MFMA work).  Held to 3 waves per SIMD -- by claiming
  // enough LDS that only so many workgroups fit a CU -- the same launch is 1.96 rounds, both full.  `cap`: what the kernel's register
  // budget allows; the pipe reaches ~92 / 96 / 98 % of its rate from 2 / 3 / 4 waves per SIMD.
  auto shape_occupancy = [&](int cap) {
    // Round 5 looked at where the thin second round goes (tools/sweep_trace.py now records every wave's HW_ID; tools/r05_abl.sh): its waves
    // ARE spread evenly (896 SIMDs with two of them, 128 with one at the 12 x 12 x 10 head); a unit of 252 MFMAs = 7.2 us of issue takes a
    // wave 12.9 us alone on its SIMD and 17.9 us beside one other, and exactly as long with its A loads, its B gathers or both removed --
    // one wave issues an fp64 MFMA every ~96 cycles, not 64, so a SIMD needs three to four waves whatever they wait for.  Two plans that
    // keep the launch to ONE round (every image's units dealt evenly to the workgroups that fit the chip at once, two to three units per
    // wave behind one set-up; the Kdiag chunks as second units, or alone on a wave) measured 76 - 78 us against 70: a Kdiag chunk -- two row
    // passes, one of them a single tile wide -- takes a wave 50 - 67 us beside three others and is the launch's last wave either way.
    // MEASURED AND LEFT OFF (tools/head_ab.sh): every shape got slower held to fewer waves -- 79 -> 101 us at the 12 x 12 x 10 head, 110 ->
    // 134 us at the CIFAR head, 163 -> 176 us at the MNIST head.  A wave of these sweeps is bound by its own latencies (LDS gathers, the
    // A operand from L2), not by the pipe, so a SIMD with three waves does less than one with four whatever the round count says.
    a->occ = 0;
    if (a->occ_force <= 0) return;
    if (a->occ_force > 0) { a->occ = a->occ_force < cap ? a->occ_force : 0; return; }
    const double waves = (double)a->n_wgs * a->wpg;
    if (waves < 2048.0 || waves / (1024.0 * cap) >= 6.0) return;
    static const double eff[5] = {0.0, 0.75, 0.92, 0.96, 0.98};
    double best = 0.0;
    int best_s = cap;
    for (int s = cap; s >= 2; --s) {
      const double r = waves / (1024.0 * s);
      const double e = r / ceil(r) * eff[s];
      if (e > best + 0.02) { best = e; best_s = s; }
    }
    if (best_s < cap) a->occ = best_s;
  };
  if (a->kuf) {
    // ---- the storing form: row units only ----
    // rows n, n + n_mod, ... show the same image: evaluated once, stored to each (see the note at the kernel)
    if (!a->no_rep && a->n_mod > 0 && a->n_mod < a->N) a->n_base = a->n_mod;
    a->st_jb = (int)(16 * a->sP * 8);
    a->st_rb = (int)((long)a->n_mod * a->sN * 8);
    // few units (the distinct images of a tiled batch: 32 x 16 at the headline size): narrower workgroups, so that every CU has one
    // with replicas a unit is a row fragment x a range of <= 8 column fragments (one batch of row_pass_hold): more, shorter waves -- the
    // launch ends within a short unit's time of its slowest wave (identical waves finished 27 ... 53 us after their set-up at the CIFAR
    // first layer: the memory system does not serve them evenly) -- and the stores of a range start after <= 8 tiles, not after all
    a->st_split = 1; a->st_jn = a->nfp;
    a->st_hold = a->n_base < a->N && a->sP == 1 && (a->sN % 16) != 0;   // row segments of an image not 128-byte aligned: hold + replica-outer
    if (a->n_base < a->N && a->split_force != 0) {
      a->st_split = a->split_force > 0 ? a->split_force : (a->nfp + 7) / 8;
      if (a->st_split > a->nfp) a->st_split = a->nfp;
      a->st_jn = (a->nfp + a->st_split - 1) / a->st_split;
      a->st_split = (a->nfp + a->st_jn - 1) / a->st_jn;
    }
    const int nuw = a->nfm * a->st_split;   // units per image
    const long units = (long)a->n_base * nuw;
    if (units < 1024) a->wpg = units >= 256 ? 2 : 1;
    if (a->wpg_force == 1 || a->wpg_force == 2 || a->wpg_force == 4) a->wpg = a->wpg_force;
    // units per wave: the set-up of a workgroup (image, window sums, tables: ~2.5 us of latency) is as long as a short unit (a 16-row
    // fragment against the 9 patch fragments of a 12 x 12 view at L = 25: 63 MFMAs), so such launches put several units behind one
    // set-up -- as many as leave >= 512 workgroups (two per CU); units of a few hundred MFMAs (L = 250) stay one per wave
    if (a->upw_force > 0) a->upw = a->upw_force;
    else if (a->st_jn * (a->Lq / 4) < 200 && a->n_base == a->N)
      for (int k = 4; k > 1; k >>= 1) {
        const long nwg = (long)a->n_base * ((nuw + a->wpg * k - 1) / (a->wpg * k));
        if (a->nfp <= 16 && nwg >= 512 && nuw % (a->wpg * k) == 0) { a->upw = k; break; }
      }
    push(2, a->n_base, (nuw + a->wpg * a->upw - 1) / (a->wpg * a->upw), 0, 0, a->upw);
    shape_occupancy(a->st_hold ? 2 : 3);
    return;
  }
  // ---- the reducing form: the Kzx row units of every image first, then the Kdiag chunks, shrinking towards the end of the launch ----
  // A workgroup lives as long as its longest wave, and a wave that shares its SIMD with three others needs ~4 x its own issue time: a
  // unit of 37 tiles is ~50 us of a ~150 us launch, and workgroups that END at random moments of their last 50 us leave a third of the
  // chip idle for the final stretch (tools/sweep_trace.py: busy waves over time).  The dispatcher hands out workgroups in id order as
  // slots free up, so the order of the list is the schedule: long units first, and the last stretch made of chunks of 1/2, 1/4, 1/8 the
  // size -- each level about half a round of the resident slots -- ends within one short chunk.
  const int W = a->wpg;
  // row units of a few dozen MFMAs (a 5 x 5 view of long patches: two column fragments) are shorter than the set-up they sit behind:
  // two to four per wave
  int kz_upw = 1;
  {
    const int unit_mfma = a->nfp * (a->Lq / 4);
    if (unit_mfma < 200) {
      kz_upw = (250 + unit_mfma - 1) / unit_mfma;
      if (kz_upw > 4) kz_upw = 4;
      while (kz_upw > 1 && a->nfm % (W * kz_upw)) --kz_upw;
    }
    // long launches (M = 1024 on long patches: ~20 rounds of the resident slots) halve their set-ups the same way (817 -> 778 us); launches of
    // a round or two must not (the 12 x 12 x 10 head at M = 256: 74 -> 76 us with two units per wave, 90 with four)
    if (kz_upw == 1 && unit_mfma < 400 && (long)a->N * a->nfm / W >= 16 * 1024 && a->nfm % (W * 2) == 0) kz_upw = 2;
    if (a->upw_force > 0) kz_upw = a->upw_force;   // A/B (ctx option head_upw)
  }
  if (a->kzx) push(0, a->N, (a->nfm + W * kz_upw - 1) / (W * kz_upw), 0, 0, kz_upw);
  if (a->want_kd || a->kd) {
    const int ntot = a->nfp * (a->nfp + 1) / 2;
    // coarse chunks: about one Kzx-sized unit (nfp + 1 tiles) each, their count a multiple of the workgroup's waves where that is possible
    int C0 = ntot / (a->nfp + 1);
    if (C0 >= W) C0 = C0 / W * W;
    if (C0 < 1) C0 = 1;
    int T0 = (ntot + C0 - 1) / C0;
    C0 = (ntot + T0 - 1) / T0;
    int lvT[4] = {T0, 0, 0, 0}, lvC[4] = {C0, 0, 0, 0}, lvN[4] = {a->N, 0, 0, 0}, nlv = 1;
    const long slots = 1024;   // wave slots the chip holds of this kernel (4 per SIMD)
    // measured (tools/head_ab.sh): worth 4-5 % on launches of a few rounds of the slots (M = 32 head, the 12 x 12 x 10 heads); from ~10
    // rounds on (MNIST head at M = 256: 10.6) the extra workgroups' set-ups cost what the sharper end saves, so those keep equal chunks
    const long rounds = (long)a->N * ((a->kzx ? a->nfm : 0) + C0) / slots;
    if (a->tail_mode > 0 || (a->tail_mode < 0 && rounds < 8)) {
      int left = a->N;
      for (int lv = 1; lv < 4; ++lv) {
        const int T = (T0 + (1 << lv) - 1) >> lv;
        if (T < 3 || T == lvT[lv - 1]) break;
        const int C = (ntot + T - 1) / T;
        long n = slots / 2 / C;                     // half a round of the slots at this chunk size
        if (a->tail_mode > 0) n = n * a->tail_mode / 4;   // A/B: tail_mode / 4 of that
        if (n < 1) n = 1;
        if (n > left / 2) n = left / 2;             // never more than half of what is left: the coarse levels keep the bulk
        if (n <= 0) break;
        lvT[lv] = T; lvC[lv] = C; lvN[lv] = (int)n; left -= (int)n; nlv = lv + 1;
      }
      lvN[0] = left;
    }
    int img = 0;
    for (int lv = 0; lv < nlv; ++lv) {
      const int before = a->nseg;
      push(1, lvN[lv], (lvC[lv] + W - 1) / W, lvT[lv], lvC[lv]);
      if (a->nseg > before) { a->seg[before].img0 = img; img += lvN[lv]; }
      if (lvC[lv] > a->n_kd) a->n_kd = lvC[lv];
    }
  }
  shape_occupancy(4);
}

extern "C" int dcgp_debug_set_sweep_trace(dcgp_ctx* ctx, long long* buf_dev, long n_workgroups, const char* family) {
  if (!ctx) return DCGP_ERR_ARG;
  ctx->sweep_trace = buf_dev;   // [n_workgroups][waves per workgroup][8] int64; nullptr switches the stamps off
  ctx->sweep_trace_wgs = buf_dev ? n_workgroups : 0;
  ctx->sweep_trace_family = family ? family : "";
  return DCGP_OK;
}

int head_units(dcgp_ctx* ctx, const HeadUnitsArgs& a_in) {
  HeadUnitsArgs a = a_in;
  const char* family = a.timer ? a.timer : (a.kuf ? "kuf" : "head_sweep");
  if (ctx->sweep_trace && (ctx->sweep_trace_family.empty() || ctx->sweep_trace_family == family)) { a.trace = ctx->sweep_trace; a.trace_wgs = ctx->sweep_trace_wgs; }
  if (a.N <= 0) return DCGP_OK;
  a.exp_tab = exp2_table(ctx);
  if (!a.exp_tab) return DCGP_ERR_ALLOC;
  if (a.want_kd && !a.kd) return ctx_fail(ctx, DCGP_ERR_ARG, "head_units: Kdiag partial sums wanted but no buffer (allocate kd [N][n_kd] behind head_units_plan)");
  if (!head_units_ok(a) || a.n_mod <= 0 || a.Lq != round_up(a.L + 2, 4) || a.Mp % 16)
    return ctx_fail(ctx, DCGP_ERR_ARG, "head_units: unsupported shape (image %d doubles, L = %d, Mp = %d)", a.HWC, a.L, a.Mp);
  const long nwg = a.n_wgs;
  if (nwg <= 0) return DCGP_OK;
  if (nwg > 0x7fffffffL) return ctx_fail(ctx, DCGP_ERR_ARG, "head_units: too many workgroups");
  size_t lds = head_units_lds(a);
  // Beside the factorisation chain (a head-first model: the sweep needs Z only): a chain workgroup is one wave of 250 VGPRs per SIMD
  // and 50 KB of LDS, and would never find that much free at once on a CU this launch keeps refilling with four 128-register
  // workgroups.  Claiming 53 KB per workgroup holds the sweep to THREE per CU: whenever one of them ends -- somewhere on the chip
  // every ~0.1 us -- that CU has 53 KB and half of every SIMD's registers free, and the chain's high-priority stream takes the slot
  // before the sweep's backlog does.  (Round 3 claimed 54 KB = two per CU, so that every CU always had room: the sweep ran at two waves
  // per SIMD, 184 us instead of 171, and the chain no faster -- 157 against 134 us; head-only model 4100 -> 4300 steps/s.  52 KB and
  // below measured worse again, and with no claim at all the chain starves: 213 us.  ctx option share_kb.)
  const size_t share_claim = (size_t)(a.share_kb > 0 ? a.share_kb : 53) * 1024;
  if (a.share_cu && lds < share_claim) lds = share_claim;
  if (a.occ > 0) {   // occupancy shaping (head_units_plan): exactly 4 occ / wpg workgroups per CU
    const int per_cu = 4 * a.occ / a.wpg;
    const size_t claim = (size_t)(160 * 1024 / per_cu) & ~(size_t)255;
    if (claim <= 64 * 1024 && lds < claim) lds = claim;
  }
  // patch rows of 50 contiguous elements, an odd number of them (5 x 5 x 10): the patch-row form of the streamed loop (kernel: RW); ctx option sweep_no_rows: A/B
  const bool rw50 = a.f * a.C == 50 && (a.f & 1) && a.L == a.f * a.f * a.C && !ctx->opt.sweep_no_rows;
  ScopedTimer t(ctx, family);
  if (a.kuf) {
    // patch lengths of the first layers (5 x 5 x 1, 4 x 4 x 1, 4 x 4 x 3: MNIST / CIFAR conv0) with the row operand resident in registers
#define HU_STORE_W(NK4, TL, WM)                                                                                                          \
  do {                                                                                                                                     \
    if (a.wpg == 4) hipLaunchKernelGGL((head_units_kernel<NK4, TL, WM, 256>), dim3((unsigned)nwg), dim3(256), lds, ctx->stream, a);        \
    else if (a.wpg == 2) hipLaunchKernelGGL((head_units_kernel<NK4, TL, WM, 128>), dim3((unsigned)nwg), dim3(128), lds, ctx->stream, a);   \
    else hipLaunchKernelGGL((head_units_kernel<NK4, TL, WM, 64>), dim3((unsigned)nwg), dim3(64), lds, ctx->stream, a);                     \
  } while (0)
#define HU_STORE(NK4, TL)                     \
  do {                                        \
    if (a.st_hold) HU_STORE_W(NK4, TL, 2);    \
    else HU_STORE_W(NK4, TL, 1);              \
  } while (0)
    if (a.L == 25 && !a.stream_k) HU_STORE(7, 1);
    else if (a.L == 16 && !a.stream_k) HU_STORE(5, 0);
    else if (a.L == 48 && !a.stream_k) HU_STORE(13, 0);
    else if (rw50) HU_STORE(0, 50);
    else HU_STORE(0, 0);
#undef HU_STORE
#undef HU_STORE_W
  } else if (a.kfull) {   // a training step's head: the reducing form that also leaves every kernel value behind
    if (a.L == 25) hipLaunchKernelGGL((head_units_kernel<7, 1, 3, 256>), dim3((unsigned)nwg), dim3(256), lds, ctx->stream, a);
    else if (rw50 && a.wpg == 4) hipLaunchKernelGGL((head_units_kernel<0, 50, 3, 256>), dim3((unsigned)nwg), dim3(256), lds, ctx->stream, a);
    else if (rw50) hipLaunchKernelGGL((head_units_kernel<0, 50, 3, 128>), dim3((unsigned)nwg), dim3(128), lds, ctx->stream, a);
    else if (a.wpg == 4) hipLaunchKernelGGL((head_units_kernel<0, 0, 3, 256>), dim3((unsigned)nwg), dim3(256), lds, ctx->stream, a);
    else hipLaunchKernelGGL((head_units_kernel<0, 0, 3, 128>), dim3((unsigned)nwg), dim3(128), lds, ctx->stream, a);
  } else if (a.L == 25) {
    hipLaunchKernelGGL((head_units_kernel<7, 1, 0, 256>), dim3((unsigned)nwg), dim3(256), lds, ctx->stream, a);   // 5 x 5 x 1 patches
  } else if (rw50) {   // 5 x 5 x 10 patches (every long patch of the BASELINE configurations): the streamed form walking patch rows
    if (a.wpg == 4) hipLaunchKernelGGL((head_units_kernel<0, 50, 0, 256>), dim3((unsigned)nwg), dim3(256), lds, ctx->stream, a);
    else hipLaunchKernelGGL((head_units_kernel<0, 50, 0, 128>), dim3((unsigned)nwg), dim3(128), lds, ctx->stream, a);
  } else if (a.wpg == 4) {
    hipLaunchKernelGGL((head_units_kernel<0, 0, 0, 256>), dim3((unsigned)nwg), dim3(256), lds, ctx->stream, a);
  } else {
    hipLaunchKernelGGL((head_units_kernel<0, 0, 0, 128>), dim3((unsigned)nwg), dim3(128), lds, ctx->stream, a);
  }
  LAUNCH_CHECK(ctx);
  return DCGP_OK;
}

// How one launch of the one-launch conv layer kernel (conv_fused.hip) is dealt: strip shape, LDS split, grid, and which of the kernel's ways of handing strips
// to workgroups it takes.  Host-only and free of HIP, the ctx and device pointers: plan_layer_launch() maps a Query of plain integers to a Plan, conv_fused()
// executes the Plan, and the CPU suite reaches the same function through dcgp_debug_plan_layer_launch (tests/test_host_fused_plan.py).
#pragma once
#include <algorithm>
#include <functional>
#include <map>
#include <mutex>
#include <queue>
#include <tuple>
#include <vector>

namespace fused_plan {

// the instantiated shapes: <FN, NS, MAXF, NT> (the template switch of conv_fused() instantiates row i for shape i)
//   0: <4,2,2,1024>  Mp <= 256, 64-column strips, 16 waves in two teams       1: <4,1,2,512>  the same on 8 waves
//   2: <2,1,2,512>   Mp <= 256, 32-column strips (large images)               3: <1,1,2,512>  16-column strips
//   4: <2,1,2,768>   Mp <= 384 (12 waves)     5: <2,1,2,1024>  Mp <= 512      6: <1,1,4,1024>  Mp <= 1024
struct FusedShape { int FN, NS, MAXF, NT, max_nf; };
constexpr FusedShape kShapes[] = {{4, 2, 2, 1024, 16}, {4, 1, 2, 512, 16}, {2, 1, 2, 512, 16}, {1, 1, 2, 512, 16},
                                  {2, 1, 2, 768, 24},  {2, 1, 2, 1024, 32}, {1, 1, 4, 1024, 64},
                                  {2, 2, 2, 1024, 16}};   // 7: a 32-column strip on 16 waves, two teams splitting the outputs (few columns: a rank's shard)
constexpr int kNumShapes = sizeof(kShapes) / sizeof(kShapes[0]);
constexpr long kLdsBytes = 160 * 1024;   // LDS of a CU

// Everything the decision reads.  The order of the fields is the order of dcgp_debug_plan_layer_launch's flat query (include/dcgp.h).
struct Query {
  long Mp = 0, M = 0, R = 0, Rp = 0, Kc = 0, P = 0, HWC = 0, L = 0, Lp = 0, Lz = 0, f = 0, C = 0, n_mod = 0, rep = 1;
  long base = 0;          // base-kernel type (BaseKernel::type)
  long has_G = 0;         // the layer has a q_sqrt term
  long keeps_state = 0;   // the launch leaves K_uf / A1 for the reverse pass
  long has_trace = 0;     // phase stamps are on (dcgp_debug_set_fused_trace)
  long n_cus = 0;         // compute units of the device (<= 0: 256)
  long fused_shape = -1, fused_large = 0, fused_split = -1, fused_persist = -1, fused_pre = -1, fused_parts = -1, fused_rep_share = -1, fused_wgs = 0,
       fused_stagger = -1, sweep_no_rows = 0;   // the ctx options of the same names (common.h)
  static constexpr int kFields = 29;
  template <class Q>
  static auto fields(Q& q) {   // (the one list of the fields: the memo's key and the flat query are made from it)
    return std::tie(q.Mp, q.M, q.R, q.Rp, q.Kc, q.P, q.HWC, q.L, q.Lp, q.Lz, q.f, q.C, q.n_mod, q.rep, q.base, q.has_G, q.keeps_state, q.has_trace, q.n_cus,
                    q.fused_shape, q.fused_large, q.fused_split, q.fused_persist, q.fused_pre, q.fused_parts, q.fused_rep_share, q.fused_wgs, q.fused_stagger,
                    q.sweep_no_rows);
  }
  bool operator<(const Query& o) const { return fields(*this) < fields(o); }
};

enum Deal { kPerStrip = 0, kCounter = 1, kFixedStride = 2 };   // one workgroup per strip; persistent, strips off a device counter / blockIdx, blockIdx + grid, ...

// Everything conv_fused() needs to launch.  The integer fields, then the three makespans, are dcgp_debug_plan_layer_launch's flat plan in this order.
struct Plan {
  int ok = 0;              // 0: the kernel does not cover the layer (the sweep + GEMM route takes it); nothing else is set
  int shape = 0;           // row of kShapes
  long lds = 0;            // dynamic LDS of a workgroup, bytes
  int lds_main = 0, lds_img = 0;   // its split, in doubles: the strip / the images of the strip
  long grid = 0;           // workgroups
  int persist = 0;         // workgroups of a persistent launch (0: one workgroup per strip, strips of a shared last round several)
  int n_strips = 0, n_items = 0;   // persistent: strips, and items dealt (n_strips + pre_n * pre_sq; n_strips where replicas share a prologue)
  int deal = kPerStrip;
  int split_first = 1 << 30, split_q = 1;   // strips >= split_first are shared by split_q workgroups each
  // the hand-over of a persistent launch (ConvFusedArgs, layer.h): pre_n slots; prologues ahead for the strips from pre_first on, each taken up by pre_sq
  // parts; or (pre_D > 0) the strips below pre_D leave their A1 on the way, those below pre_whole run whole, every later strip i fetches slot i % pre_D
  int pre_n = 0, pre_first = 0, pre_sq = 1, pre_D = 0, pre_whole = 0;
  long pre_stride = 0;     // doubles per slot
  int stagger = 0;         // two workgroups per CU: 100 MHz ticks the second to arrive holds back
  int cu_slots = 0;        // ... and the launch needs the per-CU arrival counters
  int patch_rows = 0;      // the patch-row instance of the sweep (5 x 5 x 10 RBF patches on the 64-column strip of 16 waves)
  // the simulated deals that were compared, in outputs of the second product (0: not simulated): one item per strip (for parts: the launch without them);
  // the chosen prologues ahead (for parts: every strip ahead, its outputs as pre_sq parts); the replicas' shared prologues
  double units_plain = 0.0, units_ahead = 0.0, units_shared = 0.0;
  static constexpr int kFields = 24;
};

// Phase costs of a strip in outputs of the second product (profiles/r06_fused_phase_trace.txt at M = 256): sweep + first product, epilogue, and the hand-over
// of A1 through memory on either side
constexpr double kCostPrologue = 1.75, kCostEpilogue = 0.3, kCostHandOver = 0.2;
constexpr double kDealMargin = 0.98;    // a simulated deal must save 2 % to replace the plain one
constexpr double kShareMargin = 0.9;    // sharing a strip's outputs (a split last round, parts) must save a tenth
constexpr double kFront = 0.11;         // sweep + first product as a fraction of a strip: what every sharer of a split strip pays again
constexpr double kEps = 1e-9;

// The deal of a persistent launch, simulated: items go in list order to whichever of `slots` workgroups is free first.
//   kWhole         a strip from sweep to sample
//   kLeaving       the same, leaving its A1 in `slot` on the way (ready once prologue and hand-over are through)
//   kPrologueOnly  phases 0 - 2 only, A1 left in `slot`
//   kConsumer      fetches `slot` (waiting for it where the deal has it so) and runs `outputs` outputs of the second product and the epilogue: a strip whose
//                  prologue ran ahead or is shared (all R outputs), or a PART of a strip (its share of them)
enum Item { kWhole, kLeaving, kPrologueOnly, kConsumer };
class DealSim {
 public:
  DealSim(long slots, long R, long handovers) : R_((double)R), ready_((size_t)std::max<long>(handovers, 0), 0.0) {
    for (long i = 0; i < slots; ++i) free_at_.push(0.0);
  }
  void give(Item kind, long slot = 0, double outputs = 0.0) {
    const double F = kCostPrologue + R_ + kCostEpilogue;
    if (kind == kWhole) run(F, 0.0);
    else if (kind == kLeaving) ready_[(size_t)slot] = run(F + kCostHandOver, 0.0) - (R_ + kCostEpilogue);
    else if (kind == kPrologueOnly) ready_[(size_t)slot] = run(kCostPrologue + kCostHandOver, 0.0);
    else run(kCostHandOver + outputs + kCostEpilogue, ready_[(size_t)slot]);
  }
  void give_cost(double cost) { run(cost, 0.0); }   // an item of a given cost that waits for no hand-over (a head row, an item of the head's tail)
  double makespan() const { return end_; }
  std::vector<double> free_times() const {   // when each workgroup is done with its last item
    std::vector<double> out;
    for (auto q = free_at_; !q.empty(); q.pop()) out.push_back(q.top());
    return out;
  }

 private:
  double run(double cost, double not_before) {
    const double t = std::max(free_at_.top(), not_before) + cost;
    free_at_.pop();
    free_at_.push(t);
    end_ = std::max(end_, t);
    return t;
  }
  double R_, end_ = 0.0;
  std::vector<double> ready_;
  std::priority_queue<double, std::vector<double>, std::greater<double>> free_at_;
};

// Prologues ahead.  A partial round leaves workgroups idle for a whole strip time (720 strips on 256 CUs: 3 rounds for 2.81 of work).  Sharing a strip's
// OUTPUTS between workgroups re-pays its sweep and first product (4h.6: no split wins); sharing its PROLOGUE does not.  So the partial round goes first (`first`
// strips whole), its spare workgroups run phases 0 - 2 of n_pre later strips and leave A1 in memory (132 KB per strip, L2 / Infinity-Cache traffic), the other strips
// run whole, and the n_pre strips then start at the second product.
// SQ > 1 (few strips, a rank's shard of a strongly-scaled batch: first = 0, n_pre = strips): each of them as SQ parts, part q running the outputs r = q, q + SQ, ... --
// what sharing a strip between workgroups always wanted, without re-paying sweep and first product per part.  The NS teams of a part take its outputs in turn.
inline double ahead_units(long strips, long slots, long first, long n_pre, long R, long SQ = 1, int NS = 1) {
  DealSim d(slots, R, n_pre);
  for (long i = 0; i < first; ++i) d.give(kWhole);
  for (long i = 0; i < n_pre; ++i) d.give(kPrologueOnly, i);
  for (long i = 0; i < strips - first - n_pre; ++i) d.give(kWhole);
  for (long i = 0; i < n_pre; ++i)
    for (long q = 0; q < SQ; ++q) {
      const long nr = q < R ? (R - 1 - q) / SQ + 1 : 0;
      d.give(kConsumer, i, SQ == 1 ? (double)R : (double)(NS * ((nr + NS - 1) / NS)));   // (two teams: an output costs its team two units)
    }
  return d.makespan();
}
// Replicas share a prologue: strip i < D whole and leaving its A1, the rest of the first round (below `whole`) whole, every later strip fetching the A1 of strip i % D
inline double shared_units(long strips, long slots, long D, long whole, long R) {
  DealSim d(slots, R, D);
  for (long i = 0; i < strips; ++i) {
    if (i < D) d.give(kLeaving, i);
    else if (i < whole) d.give(kWhole);
    else d.give(kConsumer, i % D, (double)R);
  }
  return d.makespan();
}

// The partial last round of one workgroup per strip.  A 1024-thread strip owns its CU, so `strips` workgroups take ceil(strips / CUs) strip times and the
// last round leaves CUs idle.  Where they are enough, its strips are shared by Q workgroups each: every one of them runs the sweep and the first product
// (kFront of a strip) and the outputs r = q, q + Q, ... of the R-batched product, whose teams take them in turn -- a part costs
// kFront + (1 - kFront) * (outputs of its busiest team) / (outputs of a whole strip's busiest team).  Returns the last round's cost in strip times
// (1 unshared) and the Q to use.  Measured on shards of the headline batch (tools/shape_try.py): 90 strips of 64 columns 198 -> 118 us with Q = 2, 360
// strips of 32 columns on 16 waves 215 -> 174 us; the full batch (720 strips, 208 in the last round) has no CUs to share with.
inline double last_round(const Query& q, const FusedShape& sh, long strips, long slots, int* q_out) {
  *q_out = 1;
  const long want = q.fused_split, R = q.R;
  const long rem = strips % slots;
  if (rem == 0) return 0.0;
  if (want == 0 || want == 1 || sh.NT != 1024 || !q.has_G || R < 2) return 1.0;
  const long whole = (R + sh.NS - 1) / sh.NS;
  const long qmax = std::min(slots / rem, R);
  double best = kShareMargin;
  for (long s = 2; s <= qmax; ++s) {
    const long part = ((R + s - 1) / s + sh.NS - 1) / sh.NS;
    const double cost = kFront + (1.0 - kFront) * (double)part / (double)whole;
    if ((want > 1 && s <= want) || (want < 0 && cost < best - kEps)) { best = cost; *q_out = (int)s; }
  }
  return *q_out > 1 ? best : 1.0;
}

inline Plan plan_uncached(const Query& q) {
  Plan p;
  const long nf = q.Mp / 16;
  if (q.Rp != 16 || q.R > 16 || q.R < 1 || q.Mp > 1024 || q.Mp < 16 || q.Mp % 16 || q.P <= 0) return p;
  if (q.Kc >= (1 << 23) || q.HWC >= (1 << 23)) return p;   // the kernel's index arithmetic (fdiv) is exact below 2^23: larger layers take the sweep + GEMM route
  // M > 256: the 32- / 16-column strips LDS leaves room for re-fetch the A operands 2 - 4 x as often per MFMA and measure
  // 2 % (M = 384) to 16 % (M = 1024) behind the sweep + 128 x 128-tile GEMM route (87 % of the MFMA peak there); opt-in
  const long force = q.fused_shape;   // A/B experiments (-1: none)
  if (nf > 16 && force < 0 && !q.fused_large) return p;
  const long all_cus = q.n_cus > 0 ? q.n_cus : 256;

  // The shape.  Among those that fit, the one whose busiest CU carries the fewest columns: workgroups go round the CUs, a CU works through
  // ceil(strips / CUs) strips of BN columns at a rate that does not depend on BN (narrow strips share the CU), so few columns -- a shard of a
  // strongly-scaled batch -- are better cut into narrower strips (4 images x 10 samples x 144 patches: 90 strips of 64 keep 90 CUs busy for a full strip
  // time, 180 strips of 32 keep 180 busy for half of it).  The wider strip wins ties: fewer A-operand fetches per MFMA (measured 3 % / 6 % behind at
  // 32 / 16 columns on the full batch).
  double best = 0.0;
  int shape_q = 1;   // the sharing of the last round that the chosen shape was priced with
  for (int i = 0; i < kNumShapes; ++i) {
    const FusedShape& sh = kShapes[i];
    if (force >= 0 && i != force) continue;
    if (nf > sh.max_nf) continue;
    if (sh.max_nf > 16 && nf <= 16 && force < 0) continue;   // the many-wave shapes are for the large matrices
    if (i == 1 && force < 0) continue;                        // (the 8-wave form of shape 0: A/B experiments only)
    const long BN = sh.FN * 16, W = sh.NT / 64, TW = W / sh.NS, KG = W / sh.FN;
    const long nimg = (BN - 1) / q.P + 2;           // images a strip can touch
    const long main_d = std::max(q.Mp * BN, (TW * q.R + KG * 16) * BN);
    const long img_d = std::max((nimg * q.HWC + 1) & ~1L, TW * BN);
    const long bytes = (main_d + img_d + BN + 2) * 8 + std::max(q.Lz, q.Lp) * 4;
    if (bytes > kLdsBytes) continue;
    const long strips = q.Kc > 0 ? (q.Kc + BN - 1) / BN : 1;
    // shape 7 (32 columns on 16 waves, the outputs split over two teams): a strip's latency is what a launch of one round costs, and
    // the second team shortens it (a 4-image shard of the headline batch: 0.297 -> 0.290 ms per step); over several rounds the eight-wave
    // form's two strips per CU do better (8 images: 0.398 against 0.384)
    if (i == 7 && force < 0 && strips > 512) continue;
    int sq = 1;
    const double rounds = sh.NT == 1024 ? (double)(strips / all_cus) + last_round(q, sh, strips, all_cus, &sq) : (double)((strips + 255) / 256);
    const double cost = rounds * (double)BN * (i == 7 ? 0.97 : (sh.FN == 4 ? 1.0 : (sh.FN == 2 ? 1.03 : 1.12)));
    if (p.ok && cost >= best) continue;
    best = cost; shape_q = sq;
    p.ok = 1; p.shape = i; p.lds = bytes; p.lds_main = (int)main_d; p.lds_img = (int)img_d;
  }
  if (!p.ok) return p;

  const FusedShape& sh = kShapes[p.shape];
  const long BN = sh.FN * 16, TW = sh.NT / 64 / sh.NS, R = q.R;
  const long strips = (std::max<long>(q.Kc, 0) + BN - 1) / BN;
  const double whole_strip = kCostPrologue + (double)R + kCostEpilogue;
  p.grid = strips;
  p.patch_rows = p.shape == 0 && q.base == 0 && q.f * q.C == 50 && (q.f & 1) && q.L == q.f * q.f * q.C && q.Lz == ((q.L + 2 + 3) & ~3L) &&
                 !q.sweep_no_rows;
  const long slots = q.fused_wgs > 0 && q.fused_wgs < all_cus ? q.fused_wgs : all_cus;   // (fused_wgs: a small layer in several rounds, tests)
  // workgroups a CU holds: LDS and wave slots (the kernels are held to 128 registers: 16 waves of 64 per CU)
  const long per_cu = std::min<long>(kLdsBytes / p.lds, 1024 / sh.NT);
  // Persistent, chosen (-1): where a workgroup owns its CU and no strip of the last round is shared.  What it buys is the deal, not the persistence: strips
  // handed out by a device counter to whichever workgroup is free 572 us at cfg2, dealt by a fixed stride 576 -- as many as one workgroup per strip takes
  // (profiles/r06_fused_ab.txt)
  const long want = q.fused_persist;
  bool persist = strips > per_cu * slots && (want > 0 || (want < 0 && per_cu == 1 && shape_q == 1 && !q.keeps_state));
  // Few strips (< 1.5 rounds): all of them handed over, their outputs dealt as parts.  MEASURED (tools/parts_try.py, the 4 / 8 / 16-image shards of the headline batch):
  // correct and bit-identical, and SLOWER than the launches it would replace at every shard and every SQ -- 4 images 109 us (180 strips of 32 columns, one round) against
  // 120-148 us as parts, 8 images 169 against 185-259, 16 images 303-308 against 302-421.  A part pays its ticket, the flag, the fetch of the strip, the mean product, two
  // barriers of partial sums and the epilogue (~10 us) for 8-15 us of second product; the simulated deal prices that at 0.5 of an output.  So fused_parts = -1 is "off";
  // -2 leaves SQ to the simulated deal (A/B), q > 0 forces it (tests/test_gpu_ops.py).
  long parts = 0;
  const bool parts_wanted = q.fused_parts != 0 && q.fused_parts != -1 && want != 0 && want != 2;
  if (parts_wanted && !persist && per_cu == 1 && q.has_G && !q.keeps_state && R >= 2 && strips > 0 && 2 * strips <= 3 * slots) {
    int q_legacy = 1;
    const double last = last_round(q, sh, strips, all_cus, &q_legacy);
    const double legacy = ((double)(strips / slots) + (strips % slots ? last : 0.0)) * whole_strip;
    if (q.fused_parts > 0) parts = std::min(q.fused_parts, R);
    else {
      double best_t = legacy * kShareMargin;
      for (long s = 2; s <= R; ++s) {
        const double t = ahead_units(strips, slots, 0, strips, R, s, sh.NS);
        if (t < best_t - kEps) { best_t = t; parts = s; }
      }
    }
    if (parts > 1) {
      persist = true;
      p.units_plain = legacy;
      p.units_ahead = ahead_units(strips, slots, 0, strips, R, parts, sh.NS);
    }
  }

  if (!persist) {
    if (shape_q > 1 && !q.has_trace) {
      p.split_q = shape_q;
      p.split_first = (int)(strips - strips % slots);
      p.grid = p.split_first + (strips - p.split_first) * p.split_q;
    }
    return p;
  }
  p.persist = (int)(per_cu * slots);
  p.grid = p.persist;
  p.n_strips = p.n_items = (int)strips;
  p.deal = want != 2 ? kCounter : kFixedStride;   // (2: the fixed deal -- A/B)
  if (per_cu > 1) {
    p.stagger = (int)((q.fused_stagger >= 0 ? q.fused_stagger : 40) * 100);
    p.cu_slots = 1;
  }
  if (per_cu != 1 || p.deal != kCounter || !q.has_G) return p;

  // the hand-over: parts, or prologues ahead, or the replicas' shared prologues
  const long stride = q.Mp * BN + TW * BN;   // doubles of a slot: the strip's LDS image, then the partial sums of A1^2
  if (parts > 1) {
    p.pre_n = (int)strips; p.pre_sq = (int)parts; p.pre_stride = stride;
    p.n_items = (int)(strips + strips * parts);
    return p;
  }
  const long S = p.persist;
  p.units_plain = (double)((strips + S - 1) / S) * whole_strip;   // one item per strip: whole rounds
  // the number of prologues ahead: the best multiple of an eighth of the workgroups that a spare workgroup's strip time has room for (fused_pre = k > 0: k
  // per spare workgroup, and the best non-zero count whatever it saves)
  long n_pre = 0;
  const long rem = strips % S, rounds = strips / S, pre = q.fused_pre;
  if (pre != 0 && rem != 0 && rounds >= 1 && rounds <= 16 && R >= 2) {
    const long per = pre > 0 ? pre : (long)(whole_strip / (kCostPrologue + kCostHandOver));   // prologues a spare workgroup runs in one strip time
    const long most = std::min((S - rem) * per, strips - rem), step = std::max<long>(S / 8, 1);
    double best_t = p.units_plain * (pre > 0 ? 2.0 : kDealMargin);
    for (long n = step; n <= most; n += step) {
      const double t = ahead_units(strips, S, rem, n, R);
      if (t < best_t - kEps) { best_t = t; n_pre = n; p.units_ahead = t; }
    }
  }
  // Replicas share a prologue.  propagate() tiles the minibatch S times in front of the first layer, so row n shows image n % n_mod: where n_mod * P columns
  // are a whole number D of strips, strip i reads the images of strip i % D at the same patch positions and its K_uf, A1 and sum A1^2 are the same numbers,
  // bit for bit.  Nothing is shared across a strip that straddles two replicas (a period that is no whole number of strips), with `rep` in force (the outputs
  // are already laid out per replica), in the launch that keeps K_uf / A1 for the reverse pass, or with fused_pre >= 0 (0: no hand-over of any kind; k > 0:
  // that plan, forced).  The shared deal must beat the plain one and the prologues ahead by the margin those had to beat the plain one by.
  long D = 0;
  if (q.fused_rep_share != 0 && pre < 0 && q.n_mod > 0 && q.rep == 1 && q.Kc % q.P == 0 && !q.keeps_state) {
    const long rows = q.Kc / q.P, period = q.n_mod * q.P;
    if (rows % q.n_mod == 0 && rows / q.n_mod >= 2 && period % BN == 0) D = period / BN;
    if (D >= strips || D > 4 * S) D = 0;   // (the hand-over area: a strip's LDS image per slot)
  }
  if (D > 0) {
    p.pre_whole = (int)std::max(D, std::min(S, strips));
    p.units_shared = shared_units(strips, S, D, p.pre_whole, R);
    const double today = n_pre > 0 ? std::min(p.units_plain, p.units_ahead) : p.units_plain;
    if (!(p.units_shared < today * kDealMargin - kEps)) D = p.pre_whole = 0;
  }
  if (D > 0) {   // one slot per distinct strip, one item per strip
    p.pre_n = p.pre_D = (int)D;
    p.pre_stride = stride;
  } else if (n_pre > 0) {
    p.pre_n = (int)n_pre;
    p.pre_first = (int)rem;
    p.n_items = (int)(strips + n_pre);
    p.pre_stride = stride;
  }
  return p;
}

// One memo for the whole decision: a step asks the same few questions launch after launch, and the simulated deals cost up to a millisecond
inline Plan plan_layer_launch(const Query& q) {
  static std::mutex mu;
  static std::map<Query, Plan> memo;
  std::lock_guard<std::mutex> lock(mu);
  const auto it = memo.find(q);
  if (it != memo.end()) return it->second;
  if (memo.size() > 256) memo.clear();
  return memo[q] = plan_uncached(q);
}

// ---- Head rows riding the launch (conv_fused.hip: HEAD) --------------------------------------------------------------------------------------------------
// A persistent launch of 720 strips on 256 workgroups ends with 48 workgroups idle for a strip's time (the partial round that prologues ahead and shared
// prologues cannot fill: no strip work is left).  Where the next layer is the head, the rows of its patch sweep are dealt by the same counter behind the
// last strip item: row n waits for the strips that cover its columns [n P, n P + P) and runs the head's Kzx units of that row.  Whether a launch carries
// them is decided here and nowhere else (model.hip: plan_step); everywhere else the step is the one it was.
// HOW MANY rows ride: as many as the simulated deal's workgroups have room for before the launch's last strip ends (a row costs kCostHeadRow outputs of the second
// product).  Every row of the headline step in the launch (320 rows on 256 workgroups) measured 535 -> 574 us for the layer
// kernel: the 48 spare workgroups absorb ~240 rows, and the 80 left are a round of their own on 208 workgroups that end together -- 38 us for a sweep launch
// that had shrunk by 43.  The rows beyond the count stay in the head's sweep launch, whose one thin round costs about the same with or without them.
struct RideQuery {
  long next_is_head = 0;    // the layer's sample is the head's input, row for row
  long head_form = 0;       // the head's sweep is the reducing patch-row form of head_units_kernel (<0, 50, 0, *>: RBF ConvKernel head on 5 x 5 x 10 patches, nothing kept)
  long head_HWC = 0;        // doubles of a head row
  long head_lds = 0;        // LDS bytes of that sweep's workgroup
  long head_nfm = 0;        // its Z fragments (Mp / 16): one per wave
  long in_flight = 0;       // the step is enqueued beside others
  long chain_beside = 0;    // the parameter-only chain is not on the step's main stream (the head's prepared operands are not ordered in front of the launch)
  long head_ride = -1;      // the ctx option (0: never; k > 0: k rows, or all of them if there are fewer -- tests, A/B)
  static constexpr int kFields = 8;
};
enum RideWhy { kRides = 0, kRideOff, kRideNotHead, kRideForm, kRideLaunch, kRideState, kRideTrace, kRideInFlight, kRideGeometry, kRideNoRoom };
struct Ride {
  int ok = 0, why = kRideOff;
  int n_rows = 0;       // head items = rows 0 .. n_rows - 1 of the head, dealt behind the plan's n_items (which stay what they were)
  int first_item = 0;   // item of row 0
};
// a head row of 16 Kzx units, in outputs of the second product (15.4 us each): a round of rows measured 38 us (2.5), and a row also waits for its strips' flags.
// Counts tried at the headline: 144 rows (three per spare workgroup) 1420 steps/s, 192 (four: 2.4 a row) 1410, 224 1405, 240 1389, all 320 1387, none 1385
constexpr double kCostHeadRow = 3.0;
// rows that fit in front of the end of the launch's last strip, over the workgroups of the simulated deal (the deal of plan p, item by item)
// the items of plan p, in the order the counter deals them
inline void deal_plan_items(DealSim& d, const Query& q, const Plan& p) {
  const long strips = p.n_strips, R = q.R;
  if (p.pre_D > 0) {
    for (long i = 0; i < strips; ++i) {
      if (i < p.pre_D) d.give(kLeaving, i);
      else if (i < p.pre_whole) d.give(kWhole);
      else d.give(kConsumer, i % p.pre_D, (double)R);
    }
  } else if (p.pre_n > 0) {
    for (long i = 0; i < p.pre_first; ++i) d.give(kWhole);
    for (long i = 0; i < p.pre_n; ++i) d.give(kPrologueOnly, i);
    for (long i = 0; i < strips - p.pre_first - p.pre_n; ++i) d.give(kWhole);
    for (long i = 0; i < p.pre_n; ++i) d.give(kConsumer, i, (double)R);
  } else {
    for (long i = 0; i < strips; ++i) d.give(kWhole);
  }
}
inline long ride_room(const Query& q, const Plan& p) {
  DealSim d(p.persist, q.R, p.pre_n);
  deal_plan_items(d, q, p);
  long room = 0;
  for (double t : d.free_times()) room += (long)((d.makespan() - t + kEps) / kCostHeadRow);
  return room;
}
inline Ride plan_head_ride(const Query& q, const Plan& p, const RideQuery& r) {
  Ride out;
  auto no = [&](int why) { out.ok = 0; out.why = why; return out; };
  if (r.head_ride == 0) return no(kRideOff);
  if (!r.next_is_head) return no(kRideNotHead);
  if (!r.head_form) return no(kRideForm);
  // persistent on the counter deal, one workgroup per CU, the RBF instance of the 64-column strip on 16 waves, no strip shared between workgroups
  if (!p.ok || p.shape != 0 || p.persist <= 0 || p.deal != kCounter || p.grid != p.persist || p.cu_slots || p.patch_rows || q.base != 0 || q.rep != 1 ||
      p.pre_sq != 1 || p.split_q != 1)
    return no(kRideLaunch);
  if (q.keeps_state) return no(kRideState);
  if (q.has_trace) return no(kRideTrace);
  if (r.in_flight || r.chain_beside) return no(kRideInFlight);
  if (q.P <= 0 || q.Kc <= 0 || q.Kc % q.P || q.P * q.R != r.head_HWC || r.head_nfm < 1 || r.head_nfm > kShapes[0].NT / 64 || r.head_lds > (long)p.lds_main * 8)
    return no(kRideGeometry);
  const long rows = q.Kc / q.P;
  const long n = r.head_ride > 0 ? std::min(r.head_ride, rows) : std::min(ride_room(q, p), rows);
  if (n <= 0) return no(kRideNoRoom);
  out.ok = 1; out.why = kRides;
  out.n_rows = (int)n;
  out.first_item = p.n_items;
  return out;
}
// the strips whose samples are head row `row`
inline void ride_row_strips(long row, long P, long BN, long* lo, long* hi) { *lo = row * P / BN; *hi = (row * P + P - 1) / BN; }
// the item that writes a strip's samples (and sets its flag): the strip's own, or the consumer of a prologue that ran ahead
inline long ride_sample_item(const Plan& p, long strip) {
  if (p.pre_n > 0 && p.pre_D == 0 && strip >= p.pre_first && strip < p.pre_first + p.pre_n) return p.n_strips + (strip - p.pre_first) * p.pre_sq;
  return strip;
}

// ---- The head's whole sweep in the launch (conv_fused.hip: HEAD, tail items) ------------------------------------------------------------------------------
// Behind the whole rows of plan_head_ride the counter deals the REST of the head's sweep, so that no sweep launch follows the layer kernel:
//   * `parts` sub-row items per row that did not ride whole: part q runs the Z-fragment units [q upp, q upp + upp) of the row, one per wave, and the last part the
//     row's Kdiag chunks on the waves behind its units -- a round of such items puts two to three waves on a SIMD where a round of whole rows puts four on
//     a third of the chip;
//   * then one Kdiag item per row that rode whole: the row's Kdiag chunks, one per wave (the chunks of the stand-alone launch's plan, same boundaries, same slots).
//     They wait for strips that are long done and are short, so they go LAST and fill the workgroups up behind the sub-row items, whose rows' strips end with the
//     launch's last round (dealt first they measured 0.703 - 0.726 ms per headline step over the whole-row counts, last 0.6990 - 0.6998: profiles/head_tail_ab.txt).
// Every tail item sits behind every strip item and behind the whole rows, and waits for the strips of its row exactly as a whole row does: a strip it
// waits for is an earlier item, held by a running workgroup that waits for nothing a head item produces.
struct TailQuery {
  long head_ride_tail = -1;   // the ctx option of the same name: -1 chosen, 0 never, 1 always where eligible, k = 2 / 4 the same with k parts per row (A/B)
  long n_kd = 0;         // Kdiag slots per row of the head's sweep plan (head_units_plan): the most chunks a row has; 0: the sweep has no Kdiag chunks
  static constexpr int kFields = 2;
};
enum TailWhy { kTailRides = 0, kTailOff, kTailNoRide, kTailGeometry, kTailFewWorkgroups, kTailNoGain };
struct Tail {
  int ok = 0, why = kTailOff;
  int n_rows = 0;       // whole rows in front (items first_item - n_rows .. first_item - 1): Ride::n_rows of the launch that carries the tail
  int parts = 1, upp = 0;   // sub-row items per row that did not ride whole, Z-fragment units of each
  int first_item = 0;   // item of the first tail item
  int n_items = 0;      // tail items: (rows - n_rows) * parts sub-row items, row by row, then n_rows Kdiag items
  double units_sweep = 0.0, units_tail = 0.0;   // the simulated launch + sweep launch, and the launch that carries the tail (0: not simulated)
};
struct TailItem { int row, kz_lo, kz_hi, kd; };   // the Z-fragment units [kz_lo, kz_hi) of `row`, and (kd) the row's Kdiag chunks
inline TailItem tail_item(const Tail& t, long nfm, long i) {
  const long n_sub = t.n_items - t.n_rows;
  if (i >= n_sub) return TailItem{(int)(i - n_sub), 0, 0, 1};
  const long row = t.n_rows + i / t.parts, part = i % t.parts;
  return TailItem{(int)row, (int)(part * t.upp), (int)std::min<long>(nfm, (part + 1) * t.upp), part == t.parts - 1 ? 1 : 0};
}
// Prices in outputs of the second product (15.4 us), fitted to the layer kernel's measured length at the headline (profiles/head_tail_ab.txt, kernel stats: the
// launch with 144 whole rows 535.4 us = this simulation's 33.25; + the tail as halves 573.3, as quarters 583.8, 320 whole rows 582.5, + their 320 Kdiag items
// 585.1): a Kdiag item (set-up of the row's image and one chunk per wave on two to four waves: they fill gaps), a sub-row item of half / a quarter of a
// 16-fragment row, and what the tail replaces -- the sweep launch and its boundary, with Kzx rows left in it (44.4 us + ~6 between the launches: the step gains
// 13.3 us where the kernels' sum gains 7.2) / with Kdiag chunks only (24.3 + 6)
constexpr double kCostTailKd = 0.9, kCostTailHalf = 1.4, kCostTailQuarter = 0.95;
constexpr double kCostSweepKzx = 3.3, kCostSweepKd = 2.0;
constexpr double kTailMargin = 0.5;   // the tail must save half an output (~8 us) to be chosen
inline bool tail_parts_ok(long parts, long nfm, long n_kd, long waves) {
  if (parts < 1 || parts > nfm) return false;
  const long upp = (nfm + parts - 1) / parts;
  return (parts - 1) * upp < nfm && (nfm - (parts - 1) * upp) + n_kd <= waves;   // no empty part; the last part's units and the Kdiag chunks are one wave each
}
inline double tail_units(const Query& q, const Plan& p, long rows, long n_rows, long parts) {
  DealSim d(p.persist, q.R, p.pre_n);
  deal_plan_items(d, q, p);
  for (long i = 0; i < n_rows; ++i) d.give_cost(kCostHeadRow);
  if (parts <= 0) return d.makespan();
  const double part = parts >= 4 ? kCostTailQuarter : (parts >= 2 ? kCostTailHalf : kCostHeadRow);
  for (long i = 0; i < (rows - n_rows) * parts; ++i) d.give_cost(part);
  for (long i = 0; i < n_rows; ++i) d.give_cost(kCostTailKd);
  return d.makespan();
}
inline Tail plan_head_tail(const Query& q, const Plan& p, const RideQuery& r, const TailQuery& t) {
  Tail out;
  auto no = [&](int why) { out.ok = 0; out.why = why; return out; };
  if (t.head_ride_tail == 0) return no(kTailOff);
  // eligible where plan_head_ride is: a launch whose deal merely has no room for a whole row can still carry the tail
  const Ride ride = plan_head_ride(q, p, r);
  if (!ride.ok && ride.why != kRideNoRoom) return no(kTailNoRide);
  const long waves = kShapes[0].NT / 64, nfm = r.head_nfm, rows = q.Kc / q.P;
  if (t.n_kd < 1 || t.n_kd > waves) return no(kTailGeometry);
  const bool chosen = t.head_ride_tail < 0;
  // (the prices were measured with one workgroup on every CU of the device: nothing else is chosen)
  if (chosen && p.persist != (q.n_cus > 0 ? q.n_cus : 256)) return no(kTailFewWorkgroups);
  long parts = 0;
  if (t.head_ride_tail > 1) {
    if (!tail_parts_ok(t.head_ride_tail, nfm, t.n_kd, waves)) return no(kTailGeometry);
    parts = t.head_ride_tail;
  }
  // the whole rows in front are plan_head_ride's: the spare workgroup time is best spent on whole rows (four waves a SIMD), and with the Kdiag items last the
  // step measured the same from 144 to 208 of them (0.6990 - 0.6998 ms; 96: 0.7032, 224: 0.6992 - 0.7026, all 320: 0.7056)
  const long n_rows = ride.ok ? ride.n_rows : 0;
  if (chosen) {
    out.units_sweep = tail_units(q, p, rows, n_rows, 0) + (n_rows < rows ? kCostSweepKzx : kCostSweepKd);
    double best = out.units_sweep - kTailMargin;
    long best_parts = 0;
    for (long s : {2L, 4L, 1L}) {
      if (!tail_parts_ok(s, nfm, t.n_kd, waves)) continue;
      const double u = tail_units(q, p, rows, n_rows, s);
      if (u < best - kEps) { best = u; best_parts = s; }
    }
    if (!best_parts) return no(kTailNoGain);
    parts = best_parts;
    out.units_tail = best;
  } else if (!parts) {
    for (long s : {1L, 4L, 2L})
      if (tail_parts_ok(s, nfm, t.n_kd, waves)) parts = s;   // (two parts where the row has them)
    if (!parts) return no(kTailGeometry);
  }
  out.ok = 1; out.why = kTailRides;
  out.n_rows = (int)n_rows;
  out.parts = (int)parts; out.upp = (int)((nfm + parts - 1) / parts);
  out.first_item = p.n_items + (int)n_rows;
  out.n_items = (int)(n_rows + (rows - n_rows) * parts);
  return out;
}
// ... for the plan of q itself (p = plan_layer_launch(q)), remembered: a step asks twice, launch after launch, and the simulated deals above are ~1500 items
// each -- tens of microseconds of host time in front of a step's first launch
inline Tail plan_head_tail_memo(const Query& q, const RideQuery& r, const TailQuery& t) {
  if (t.head_ride_tail == 0) return Tail{};
  static std::mutex mu;
  static std::map<std::tuple<Query, std::tuple<long, long, long, long, long, long, long, long, long, long>>, Tail> memo;
  const auto key = std::make_tuple(q, std::make_tuple(r.next_is_head, r.head_form, r.head_HWC, r.head_lds, r.head_nfm, r.in_flight, r.chain_beside, r.head_ride,
                                                      t.head_ride_tail, t.n_kd));
  {
    std::lock_guard<std::mutex> lock(mu);
    const auto it = memo.find(key);
    if (it != memo.end()) return it->second;
  }
  const Tail out = plan_head_tail(q, plan_layer_launch(q), r, t);
  std::lock_guard<std::mutex> lock(mu);
  if (memo.size() > 256) memo.clear();
  return memo[key] = out;
}

}  // namespace fused_plan

// How one call of the strided fp64 GEMM (gemm_gen.hip) is launched: which kernel serves it (the general kernel's tile, its layout / load instantiation, its
// split along k, its grid) or whether the symmetric long contraction's own kernel does.  Host-only and free of HIP, the ctx and device pointers: plan_gemm()
// maps a Query of plain integers to a Plan, gemm_gen() executes the Plan, and the CPU suite reaches the same function through dcgp_debug_plan_gemm
// (tests/test_host_gemm_plan.py).  A test can therefore say which configuration served it, and a change of the dispatch shows up there.
#pragma once
#include <tuple>

namespace gemm_plan {

constexpr int kGK = 16;                                           // k tile of the general kernel
constexpr int kSyRows = 256, kSyKC = 32, kSyLD = kSyKC + 1, kSyNT = 768;   // syrk_kscale_kernel: rows it covers, k chunk, LDS row stride, threads
constexpr long kBigFill = 512, kSmallWgs = 256;                   // thresholds of the tile choice (below)

// Everything the decision reads.  The order of the fields is the order of dcgp_debug_plan_gemm's flat query (include/dcgp.h).
struct Query {
  long M = 0, N = 0, K = 0, batch = 1;
  long a_rs = 0, a_cs = 0, a_bs = 0, b_rs = 0, b_cs = 0, b_bs = 0;   // element strides of GenGemm
  long accumulate = 0, colscale = 0, kscale = 0, sub = 0, lower_only = 0, mirror = 0, phi = 0;   // the epilogue switches (for the pointers: given or not)
  long a_aligned = 0, b_aligned = 0;   // the A / B pointer is a multiple of 16 bytes
  long same_ab = 0;                    // A and B are the same pointer
  long null_ptr = 0;                   // A, B or C is missing
  long gemm_tile = 0, no_syrk = 0;     // the ctx options of the same names (common.h)
  long n_cus = 0;                      // compute units of the device (<= 0: 256)
  static constexpr int kFields = 24;
  template <class Q>
  static auto fields(Q& q) {
    return std::tie(q.M, q.N, q.K, q.batch, q.a_rs, q.a_cs, q.a_bs, q.b_rs, q.b_cs, q.b_bs, q.accumulate, q.colscale, q.kscale, q.sub, q.lower_only, q.mirror,
                    q.phi, q.a_aligned, q.b_aligned, q.same_ab, q.null_ptr, q.gemm_tile, q.no_syrk, q.n_cus);
  }
};

enum Route { kNothing = 0, kGeneral = 1, kSyrk = 2 };   // nothing to do (an empty result); gemm_gen_kernel; syrk_kscale_kernel
enum Error { kOk = 0, kBadArguments = 1, kBatchSplit = 2, kLowerNotSquare = 3 };

// Everything gemm_gen() needs to launch; dcgp_debug_plan_gemm's flat plan in this order.
struct Plan {
  int route = kNothing, error = kOk;   // with an error nothing is launched (the fields decided before it was found stay set)
  int tile = 0, threads = 0, wave_tile = 0;   // gemm_gen_kernel<tile, threads, wave_tile, ...>; syrk: 256 rows on 768 threads, 32 x 32 per wave
  int ksplit = 1, kchunk = 0;          // ranges of the contraction (1: direct store, no partial buffer) and the columns of a range
  int lower_compact = 0;               // the grid enumerates the tiles on / below the diagonal only
  int akf = 0, bkf = 0, vec = 0;       // the kernel's AKF / BKF / VEC
  long grid_x = 0, grid_y = 0, grid_z = 0;
  long part_doubles = 0;               // the partial buffer (0: none)
  long reduce_blocks = 0;              // workgroups of splitk_reduce_kernel behind it (256 threads each; 0: none)
  long lds = 0;                        // dynamic LDS of a workgroup, bytes (syrk only)
  static constexpr int kFields = 17;
};

inline long round_up_to(long x, long m) { return (x + m - 1) / m * m; }

// The one table of the general kernel's configurations: gemm_gen_kernel<GT, threads_of(GT), wave_tile_of(GT), ...>.  plan_general reports from it and
// gemm_gen_launch<GT> instantiates from it, so the plan's threads / wave_tile are the launch's.
constexpr int threads_of(int GT) { return GT == 128 ? 1024 : 256; }
constexpr int wave_tile_of(int GT) { return GT == 32 ? 16 : 32; }

// the symmetric long contraction of the reverse pass on its own kernel (syrk_kscale_kernel): A diag(kscale) A^T, k contiguous, 129 .. 256 rows
inline bool syrk_applies(const Query& q) {
  return !q.no_syrk && q.same_ab && q.a_bs == q.b_bs && q.a_cs == 1 && q.b_rs == 1 && q.a_rs == q.b_cs && q.M == q.N && q.M <= kSyRows && q.M > 128 &&
         q.K >= 8192 && q.lower_only && q.mirror && q.kscale && !q.colscale && !q.sub && !q.phi && (q.a_rs & 1) == 0 && (q.a_bs & 1) == 0 && q.a_aligned &&
         q.batch <= 64 && q.M * q.a_rs * 8 < 0x7fffffffL;
}

// the general kernel on a GT x GT tile: split, grid, instantiation
inline void plan_general(const Query& q, Plan& p, int GT) {
  p.route = kGeneral;
  p.tile = GT; p.threads = threads_of(GT); p.wave_tile = wave_tile_of(GT);
  // 256 CUs; 4 co-resident 32- / 64-tile workgroups per CU (40 KB LDS each), 2 of the 128-tile ones (72 KB, 1024 threads)
  const long slots_per_round = GT == 128 ? 512 : 1024;
  const long nt_m = (q.M + GT - 1) / GT, nt_n = (q.N + GT - 1) / GT;
  long tiles = nt_m * nt_n * q.batch;
  if (q.lower_only) {                 // tiles above the diagonal exit at once
    long live = 0;
    for (long bi = 0; bi < nt_m; ++bi) live += (bi + 1 < nt_n ? bi + 1 : nt_n);
    tiles = live * q.batch;
  }
  // split long contractions so that the launch fills the chip: a whole number of rounds of co-resident workgroups
  // (the 32-tile configuration serves launches that cannot fill the chip: it splits earlier and finer)
  const long split_min_k = GT == 32 ? 1024 : 2048, split_chunk = GT == 32 ? 128 : 512;
  long ksplit = 1;
  if (q.K >= split_min_k && tiles < slots_per_round) {
    ksplit = (slots_per_round + tiles - 1) / tiles;
    if (tiles * ksplit > slots_per_round && ksplit > 1) --ksplit;   // stay within one round rather than spill a few workgroups into a second
    const long max_split = q.K / split_chunk;
    if (ksplit > max_split) ksplit = max_split;
    if (ksplit < 1) ksplit = 1;
  }
  long kchunk = q.K;
  if (ksplit > 1) {
    kchunk = round_up_to((q.K + ksplit - 1) / ksplit, kGK);
    ksplit = (q.K + kchunk - 1) / kchunk;
    p.part_doubles = ksplit * q.batch * q.M * q.N;
    p.reduce_blocks = (q.M * q.N * q.batch + 255) / 256;
  }
  p.ksplit = (int)ksplit; p.kchunk = (int)kchunk;
  if (q.batch * ksplit > 65535) { p.error = kBatchSplit; return; }
  p.grid_x = nt_n; p.grid_y = nt_m; p.grid_z = q.batch * ksplit;
  if (q.lower_only && (ksplit > 1 || q.accumulate)) {   // nothing has to be written above the diagonal: visit the live tiles only
    if (q.M != q.N) { p.error = kLowerNotSquare; return; }
    p.lower_compact = 1;
    p.grid_x = tiles / q.batch; p.grid_y = 1;
  }
  p.akf = q.a_cs == 1; p.bkf = q.b_rs == 1;
  // 16-byte loads: the contiguous stride is 1 and every other stride, the base and the k origin of a split keep 16-byte alignment
  auto even = [](long x) { return (x & 1) == 0; };
  const bool a_vec = (p.akf ? even(q.a_rs) : (q.a_rs == 1 && even(q.a_cs))) && even(q.a_bs) && q.a_aligned;
  const bool b_vec = (p.bkf ? even(q.b_cs) : (q.b_cs == 1 && even(q.b_rs))) && even(q.b_bs) && q.b_aligned;
  p.vec = a_vec && b_vec;
}

// one range of columns per workgroup and output, the launch one workgroup per CU with no second round
inline void plan_syrk(const Query& q, Plan& p) {
  p.route = kSyrk;
  p.tile = kSyRows; p.threads = kSyNT; p.wave_tile = 32;
  const long cus = q.n_cus > 0 ? q.n_cus : 256;
  long ksplit = cus / q.batch;
  if (ksplit < 1) ksplit = 1;
  if (ksplit > q.K / 256) ksplit = q.K / 256;
  const long kchunk = round_up_to((q.K + ksplit - 1) / ksplit, kSyKC);
  ksplit = (q.K + kchunk - 1) / kchunk;
  p.ksplit = (int)ksplit; p.kchunk = (int)kchunk;
  p.akf = p.bkf = p.vec = 1;
  p.grid_x = ksplit; p.grid_y = q.batch; p.grid_z = 1;
  p.part_doubles = ksplit * q.batch * q.M * q.N;
  p.reduce_blocks = (q.M * q.N * q.batch + 255) / 256;
  p.lds = (long)(2 * kSyRows * kSyLD + 2 * kSyKC) * 8;
}

// big_fill / small_wgs: the thresholds of the tile choice (arguments for the timing-only builds that read them from the environment)
inline Plan plan_gemm(const Query& q, long big_fill = kBigFill, long small_wgs = kSmallWgs) {
  Plan p;
  if (q.M <= 0 || q.N <= 0 || q.batch <= 0) return p;
  if (q.null_ptr || q.K < 0) { p.error = kBadArguments; return p; }
  if (syrk_applies(q)) { plan_syrk(q, p); return p; }
  if (q.gemm_tile == 32 || q.gemm_tile == 64 || q.gemm_tile == 128) { plan_general(q, p, (int)q.gemm_tile); return p; }   // A/B switch
  // the 1024-thread 128-tile (twice the flop per operand byte) pays off where it can fill its 512 slots, split included:
  // the tiled batch's contractions (K = 46080 columns at the headline size), M = 1024.  With a few thousand columns and
  // M = 256 (de-duplicated first layer) its ~270 workgroups lose to ~900 64-tiles (training step 2.05 -> 1.93 ms)
  const long tiles128 = ((q.M + 127) / 128) * ((q.N + 127) / 128) * q.batch / (q.lower_only ? 2 : 1);
  if (q.M >= 128 && q.N >= 128 && q.K >= 4096 && tiles128 * (q.K / 512) >= big_fill) { plan_general(q, p, 128); return p; }
  // the M x M x M products of the Cholesky / KL adjoint chains would launch a few dozen 64-tile workgroups on 256 CUs and
  // take as long as one wave needs for its 32 x 32 x K block (K x 64 cycles of fp64 MFMA); 32-tiles with a 16 x 16 block per
  // wave put four times as many CUs to work on a quarter of that each.  Likewise the long contractions with a narrow
  // output (d alpha = A1 gm: M x R): a handful of tiles, split into 128-deep chunks instead of 512-deep ones
  const long wgs = ((q.M + 63) / 64) * ((q.N + 63) / 64) * q.batch / (q.lower_only ? 2 : 1);
  const long max_wgs = wgs * (q.K >= 2048 ? q.K / 512 : 1);   // what the 64-tile configuration could launch, split included
  plan_general(q, p, max_wgs <= small_wgs ? 32 : 64);
  return p;
}

}  // namespace gemm_plan

// How one panel launch of the factorisation chain (chol_fused.hip: factor_inverse_batched, chol_rl_kernel) is laid out: its trailing and inverse tiles, the
// look-ahead workgroup, the right-hand sides riding one panel behind, the grid -- and how a workgroup of that grid finds its work.  Free of HIP, the ctx and
// device pointers: plan_launch() maps a Query of plain integers to a Launch, factor_inverse_batched() launches from it, and the two decodes below are the
// ones the kernel itself calls (host and device).  The CPU suite reaches all three through dcgp_debug_plan_chain (tests/test_host_chain_plan.py), so a test
// can say which configuration served it and a change of the launch arithmetic shows up there.
#pragma once

#if defined(__HIPCC__)
#define CHAIN_PLAN_HD __host__ __device__
#else
#define CHAIN_PLAN_HD
#endif

namespace chain_plan {

constexpr int kNB = 32;             // panel width (chol_dev::NB)
constexpr long kRhsOneTileWgs = 400;   // right-hand-side workgroups of a launch up to which each takes one 64-row tile (beyond: two)

// Everything the layout of launch jp reads.  The order of the fields is the order of dcgp_debug_plan_chain's flat query (include/dcgp.h).
struct Query {
  int Mp = 0, batch = 0, jp = 0;
  int has_inv = 0;    // inv(L) is formed (d_Linv != nullptr)
  int rides = 0;      // right-hand sides ride the chain (d_rhs != nullptr)
  int max_R = 0;      // the largest R among the matrices of the batch
  int alone = 0;      // ChainMode::alone
  int no_iso = 0;     // the ctx option chain_no_iso
  static constexpr int kFields = 8;
};

// Everything factor_inverse_batched() needs to fill RlArgs and launch; dcgp_debug_plan_chain's flat plan in this order.
struct Launch {
  int np = 0, j = 0;                      // panels of the matrix, first column of this launch's panel
  int nt = 0, nT = 0, nct = 0;            // 64-row tiles below the panel, trailing tiles (lower triangle of nt x nt), 64-column tiles of the inverse
  int la_idx = -1;                        // the look-ahead workgroup (-1: none)
  int has_xla = 0, has_xin = 0, has_xnext = 0, has_xself = 0;   // the diagonal blocks' hand-over buffer exists; this launch reads / writes / publishes block 0 into it
  int has_rhs = 0;                        // this launch carries right-hand-side items
  int rhs_p = -1, rhs_last = 0, rhs_nt = 0, rhs_tpw = 1, rhs_ng = 1, rhs_nq = 0, rhs_base = 0;
  int gx = 0;                             // workgroups per matrix (0: the last panel of a plain factor -- one workgroup is launched all the same)
  int iso_per = 0;                        // > 0: the XCD-isolated 1-D grid, this many workgroups per matrix beside the look-ahead one
  int grid_x = 1, grid_y = 1;
  static constexpr int kFields = 24;
};

CHAIN_PLAN_HD inline int panels(int Mp) { return (Mp + kNB - 1) / kNB; }
// row groups of the right-hand sides: rhs_nt 64-row tiles below the lagged panel, tpw of them per workgroup (at least one group: it forms the final rows)
CHAIN_PLAN_HD inline int rhs_groups(int rhs_nt, int tpw) { return rhs_nt > 0 ? (rhs_nt + tpw - 1) / tpw : 1; }
// the first 64-row tile below the lagged panel that row group g updates (it takes tpw consecutive ones: rows 32 (p + 1) + 64 tile ...)
CHAIN_PLAN_HD inline int rhs_first_tile(int g, int tpw) { return tpw * g; }

inline Launch plan_launch(const Query& q) {
  Launch l;
  const int Mp = q.Mp, NB = kNB, jp = q.jp, j = jp * NB;
  l.np = panels(Mp); l.j = j;
  const bool xla = q.has_inv && l.np > 1;   // factor and inverse of every diagonal block, handed from launch to launch
  l.has_xla = xla;
  const int below = Mp - (j + NB);
  l.nt = below > 0 ? (below + 63) / 64 : 0;
  l.nT = l.nt * (l.nt + 1) / 2;
  l.nct = q.has_inv ? ((j + NB < Mp ? j + NB : Mp) + 63) / 64 : 0;
  const int nY = q.has_inv ? (1 + l.nt) * l.nct : 0;
  int gx = l.nT + nY;
  if (xla) {
    if (jp > 0) l.has_xin = 1;
    if (jp + 1 < l.np) { l.has_xnext = 1; l.la_idx = gx; ++gx; }
  }
  if (q.rides) {   // the right-hand sides: panel jp - 1 here, and the last panel too in the last launch
    const bool last = jp == l.np - 1;
    if (jp == 0 && xla) l.has_xself = 1;
    if (jp > 0 || last) {
      l.has_rhs = 1; l.rhs_p = jp - 1; l.rhs_last = last ? 1 : 0;
      const int below_p = jp > 0 ? Mp - NB * jp : 0;                 // rows below the lagged panel
      l.rhs_nt = below_p > 0 ? (below_p + 63) / 64 : 0;
      // one 64-row tile per workgroup while the launch stays inside the resident slots (~400 beside the chain's own tiles), else two
      const long w1 = (long)q.batch * (q.max_R * jp + 1) * (l.rhs_nt > 0 ? l.rhs_nt : 1);
      l.rhs_tpw = w1 > kRhsOneTileWgs ? 2 : 1;
      l.rhs_ng = rhs_groups(l.rhs_nt, l.rhs_tpw);
      l.rhs_nq = jp * l.rhs_ng + (last ? 1 : 0);                     // items per Lq_q: (column tile <= jp - 1, group), + the last panel's diagonal tile
      l.rhs_base = gx > 0 ? gx : 1;
      gx = l.rhs_base + q.max_R * l.rhs_nq + (jp > 0 ? l.rhs_ng : 1);   // ... + alpha's
    }
  }
  l.gx = gx;
  const int per = gx > 0 ? gx : 1;
  if (xla && !q.no_iso && q.alone) {   // the look-ahead workgroups alone on one XCD (RlArgs::iso_per)
    l.iso_per = per - (l.la_idx >= 0 ? 1 : 0);
    const int items = q.batch * l.iso_per, slots = (items + 6) / 7;
    l.grid_x = 8 * (slots > q.batch ? slots : q.batch); l.grid_y = 1;
  } else {
    l.grid_x = per; l.grid_y = q.batch;
  }
  return l;
}

// ---- the isolated 1-D grid -> (matrix b, workgroup bx of its 2-D row) ----
// Workgroup lin of a launch runs on XCD lin % 8.  The slots with (lin + 1) & 7 == 0 hold the look-ahead workgroups, one matrix each; the seven others of
// every eight take the remaining items in order: the right-hand sides of all matrices first (the longest), then the trailing / inverse tiles.
struct Wg { int b, bx; bool live; };
CHAIN_PLAN_HD inline Wg decode_iso(int lin, int batch, int iso_per, int la_idx, bool has_rhs, int rhs_base) {
  Wg w{0, 0, false};
  const int slot = lin >> 3;
  const int xcd = (lin + 1) & 7;   // (XCD 7 reads as 0: see RlArgs::iso_per)
  if (xcd == 0) {
    if (slot >= batch || la_idx < 0) return w;
    w.b = slot; w.bx = la_idx; w.live = true;
    return w;
  }
  const int item = slot * 7 + xcd - 1, nla = la_idx >= 0 ? 1 : 0;
  const int rhs_per = has_rhs ? iso_per + nla - rhs_base : 0, chain_per = iso_per - rhs_per;
  if (item < batch * rhs_per) { w.b = item / rhs_per; w.bx = rhs_base + item % rhs_per; w.live = true; return w; }
  const int it = item - batch * rhs_per;
  if (it >= batch * chain_per) return w;
  w.b = it / chain_per; w.bx = it % chain_per;
  if (nla && w.bx >= la_idx) ++w.bx;
  w.live = true;
  return w;
}

// ---- right-hand-side item idx of a matrix with R right-hand sides Lq_q -> (q, column tile ct, row group g) ----
// R blocks of rhs_nq items (Lq_q: (ct <= p, g), then in the last launch the last panel's diagonal tile, which is final_only), then alpha's ng (q == R).
// The slots of a batch are sized by its largest R: live == false where a matrix of smaller R has no item.
struct RhsItem { int q, ct, g; bool final_only, live; };
CHAIN_PLAN_HD inline RhsItem decode_rhs(int idx, int R, int rhs_nq, int p, int rhs_last, int ng) {
  RhsItem it{0, 0, 0, false, true};
  if (idx < R * rhs_nq) {
    it.q = idx / rhs_nq;
    const int rem = idx % rhs_nq;
    if (p >= 0 && rem < (p + 1) * ng) { it.ct = rem / ng; it.g = rem % ng; }
    else { it.ct = p + 1; it.g = 0; it.final_only = true; }   // (only enumerated in the last launch)
  } else {
    const int rem = idx - R * rhs_nq;
    it.q = R; it.ct = 0; it.g = rem;
    if (p < 0) { if (rem != 0 || !rhs_last) it.live = false; it.final_only = true; }   // a one-panel matrix: this launch factors it
    else if (rem >= ng) it.live = false;
  }
  return it;
}

}  // namespace chain_plan

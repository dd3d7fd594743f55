// The decision to carry the head's WHOLE sweep in the layer kernel's persistent launch, on its own: includes nothing of the project but csrc/fused_plan.h and
// walks the grid of tests/head_ride_grid.cc (head rows x patches per row x strip shape x workgroups x what the step is) under the tail options, and the
// headline query.  One line per query: the 29 query fields, '|', the 8 ride-query fields, '|', the 2 tail-query fields, '|', ok, why, whole rows, parts, units
// per part, first item, items.  For every query that carries the tail the properties of the item list are checked here:
//   * every Z-fragment unit of every row that did not ride whole is in exactly one tail item, and no unit of a row that did;
//   * every row's Kdiag chunks are in exactly one tail item (the chunks of a row are run together, one per wave, by the item that carries them);
//   * an item's units and chunks fit the workgroup's waves;
//   * every tail item sits behind the last strip item and behind the whole rows, and each strip of its row has its samples written by an earlier item;
//   * the whole rows in front of the tail are plan_head_ride's count.
// A query that plan_head_ride does not admit for another reason than room carries no tail.  A violated property ends the run with status 1.
#include <cstdio>
#include <tuple>
#include <vector>

#include "fused_plan.h"

using fused_plan::Plan;
using fused_plan::Query;
using fused_plan::Ride;
using fused_plan::RideQuery;
using fused_plan::Tail;
using fused_plan::TailItem;
using fused_plan::TailQuery;

static int fail(const char* what, long a, long b) {
  fprintf(stderr, "%s (%ld, %ld)\n", what, a, b);
  return 1;
}

// the properties of one planned tail; 0 if they hold
static int check(const Query& q, const Plan& p, const RideQuery& r, const TailQuery& t, const Tail& tl) {
  const long rows = q.Kc / q.P, nfm = r.head_nfm, BN = fused_plan::kShapes[p.shape].FN * 16, waves = fused_plan::kShapes[p.shape].NT / 64;
  const Ride rd = fused_plan::plan_head_ride(q, p, r);
  if (!rd.ok && rd.why != fused_plan::kRideNoRoom) return fail("a tail on a launch plan_head_ride does not admit", rd.why, tl.why);
  if (tl.n_rows != (rd.ok ? rd.n_rows : 0)) return fail("the whole rows in front of a tail are plan_head_ride's", tl.n_rows, rd.n_rows);
  if (tl.first_item != p.n_items + tl.n_rows) return fail("the tail sits behind the strip items and the whole rows", tl.first_item, p.n_items);
  if (tl.n_items != tl.n_rows + (rows - tl.n_rows) * tl.parts) return fail("one Kdiag item per whole row, parts items per other row", tl.n_items, tl.parts);
  if (tl.parts < 1 || tl.upp < 1 || tl.upp * tl.parts < nfm) return fail("the parts cover a row's units", tl.parts, tl.upp);
  std::vector<int> unit((size_t)(rows * nfm), 0), kd((size_t)rows, 0);
  for (long i = 0; i < tl.n_items; ++i) {
    const TailItem it = fused_plan::tail_item(tl, nfm, i);
    const long item = tl.first_item + i;
    if (it.row < 0 || it.row >= rows) return fail("a tail item's row", it.row, rows);
    if (it.kz_lo < 0 || it.kz_hi > nfm || it.kz_lo > it.kz_hi) return fail("a tail item's units", it.kz_lo, it.kz_hi);
    if (it.kz_hi == it.kz_lo && !it.kd) return fail("an empty tail item", i, it.row);
    if ((it.kz_hi - it.kz_lo) + (it.kd ? t.n_kd : 0) > waves) return fail("units and chunks are one wave each", it.kz_hi - it.kz_lo, t.n_kd);
    if (it.row < tl.n_rows && it.kz_hi > it.kz_lo) return fail("a row that rode whole has its units run again", it.row, it.kz_lo);
    for (long u = it.kz_lo; u < it.kz_hi; ++u) ++unit[(size_t)(it.row * nfm + u)];
    kd[(size_t)it.row] += it.kd ? 1 : 0;
    if (item < p.n_items) return fail("a tail item in front of a strip item", item, p.n_items);
    long lo, hi;
    fused_plan::ride_row_strips(it.row, q.P, BN, &lo, &hi);
    if (lo < 0 || hi >= p.n_strips || lo > hi) return fail("a row's strips lie inside the launch", lo, hi);
    for (long st = lo; st <= hi; ++st) {
      const long w = fused_plan::ride_sample_item(p, st);
      if (w < 0 || w >= p.n_items || w >= item) return fail("a strip's samples are written by an earlier item", w, item);
    }
  }
  for (long row = 0; row < rows; ++row) {
    if (kd[(size_t)row] != 1) return fail("every row's Kdiag chunks are run once", row, kd[(size_t)row]);
    for (long u = 0; u < nfm; ++u)
      if (unit[(size_t)(row * nfm + u)] != (row < tl.n_rows ? 0 : 1)) return fail("every unit of a row that did not ride whole is run once", row, u);
  }
  return 0;
}

static void print(const Query& q, const RideQuery& r, const TailQuery& t, const Tail& tl) {
  std::apply([&](const auto&... f) { (printf("%ld ", (long)f), ...); }, Query::fields(q));
  printf("| %ld %ld %ld %ld %ld %ld %ld %ld | %ld %ld | %d %d %d %d %d %d %d\n", r.next_is_head, r.head_form, r.head_HWC, r.head_lds, r.head_nfm, r.in_flight,
         r.chain_beside, r.head_ride, t.head_ride_tail, t.n_kd, tl.ok, tl.why, tl.n_rows, tl.parts, tl.upp, tl.first_item, tl.n_items);
}

int main() {
  long n = 0, riding = 0;
  const long shapes[] = {0, 2, 6};
  const long sides[] = {8, 12, 16, 28};
  const long nfms[] = {1, 2, 3, 16};
  for (long rows = 1; rows <= 12; ++rows)
    for (long side : sides)
      for (long stride = 1; stride <= 2; ++stride)
        for (long shape : shapes)
          for (long wgs = 1; wgs <= 6; ++wgs)
            for (int variant = 0; variant < 12; ++variant) {   // 0, 8 - 11: the tail forced; 1 - 7: something keeps the head off the launch (head_ride_grid.cc)
              const long o = (side - 5) / stride + 1, P = o * o;
              Query q;
              q.M = 32; q.Mp = 32; q.R = 10; q.Rp = 16; q.P = P; q.Kc = rows * P; q.HWC = side * side; q.L = 25; q.Lp = 28; q.Lz = 28; q.f = 5; q.C = 1;
              q.n_mod = rows; q.has_G = 1; q.n_cus = 256;
              q.fused_shape = shape; q.fused_persist = variant == 7 ? 2 : 1; q.fused_wgs = wgs;
              RideQuery r;
              r.next_is_head = variant != 1; r.head_form = variant != 2; r.head_HWC = P * q.R; r.head_lds = 16 * 1024; r.head_nfm = nfms[(rows + variant) % 4];
              r.in_flight = variant == 3; r.head_ride = variant == 4 ? 0 : (variant == 8 ? rows : (variant == 9 ? (rows + 1) / 2 : -1));
              q.keeps_state = variant == 5; q.has_trace = variant == 6;
              TailQuery t;
              t.head_ride_tail = variant == 10 ? 2 : (variant == 11 ? 4 : 1);
              t.n_kd = 2 + (rows + side) % 3;
              const Plan p = fused_plan::plan_layer_launch(q);
              const Tail tl = fused_plan::plan_head_tail(q, p, r, t);
              print(q, r, t, tl);
              ++n;
              TailQuery off = t;
              off.head_ride_tail = 0;
              if (fused_plan::plan_head_tail(q, p, r, off).ok) return fail("head_ride_tail = 0 carries no tail", n, 0);
              TailQuery chosen = t;
              chosen.head_ride_tail = -1;   // (fused_wgs < the CUs: the prices were not measured there)
              if (fused_plan::plan_head_tail(q, p, r, chosen).ok) return fail("a launch of few workgroups is not chosen", n, wgs);
              if (!tl.ok) {
                if (tl.why == fused_plan::kTailRides || tl.n_rows != 0 || tl.n_items != 0) return fail("a query that carries no tail must say why", tl.why, tl.n_items);
                const Ride rd = fused_plan::plan_head_ride(q, p, r);
                const bool parts_fit = t.head_ride_tail == 1 || fused_plan::tail_parts_ok(t.head_ride_tail, r.head_nfm, t.n_kd, 16);
                if ((rd.ok || rd.why == fused_plan::kRideNoRoom) && parts_fit) return fail("a forced tail on an eligible launch", tl.why, rd.why);
                continue;
              }
              ++riding;
              if (variant != 0 && variant < 8) return fail("only the plain synchronous forward step carries the tail", variant, tl.why);
              if (check(q, p, r, t, tl)) return 1;
            }
  // the headline: cfg2's conv layer at stride 2 (320 rows of 144 patches, 720 strips on 256 workgroups), the head on 12 x 12 x 10 at M = 256
  {
    Query q;
    q.M = 256; q.Mp = 256; q.R = 10; q.Rp = 16; q.P = 144; q.Kc = 320 * 144; q.HWC = 784; q.L = 25; q.Lp = 28; q.Lz = 28; q.f = 5; q.C = 1;
    q.n_mod = 32; q.has_G = 1; q.n_cus = 256;
    RideQuery r;
    r.next_is_head = 1; r.head_form = 1; r.head_HWC = 1440; r.head_lds = 16 * 1024; r.head_nfm = 16;
    const Plan p = fused_plan::plan_layer_launch(q);
    for (long how : {-1L, 1L, 2L, 4L})
      for (long ride : {-1L, 96L, 320L}) {
        TailQuery t;
        t.head_ride_tail = how; t.n_kd = 4;
        r.head_ride = ride;
        const Tail tl = fused_plan::plan_head_tail(q, p, r, t);
        print(q, r, t, tl);
        ++n;
        if (how > 0 && !tl.ok) return fail("the headline launch carries a forced tail", how, tl.why);
        if (how > 0 && tl.n_rows != (ride < 0 ? 144 : ride)) return fail("the headline's whole rows", tl.n_rows, ride);
        if (how > 1 && tl.parts != how) return fail("forced parts", tl.parts, how);
        if (how < 0 && !tl.ok && tl.why != fused_plan::kTailNoGain) return fail("the headline is decided by the simulated deal", tl.why, 0);
        if (how < 0 && tl.ok && !(tl.units_tail < tl.units_sweep)) return fail("a chosen tail is the shorter simulated deal", (long)tl.units_tail, (long)tl.units_sweep);
        if (tl.ok && check(q, p, r, t, tl)) return 1;
        riding += tl.ok;
      }
    r.head_ride = -1;
    if (fused_plan::plan_head_ride(q, p, r).n_rows != 144) return fail("plan_head_ride's headline count", fused_plan::plan_head_ride(q, p, r).n_rows, 144);
  }
  fprintf(stderr, "%ld queries, %ld carry the tail\n", n, riding);
  return riding > 0 ? 0 : 1;
}

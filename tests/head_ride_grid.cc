// The decision to carry the head's rows in the layer kernel's persistent launch, on its own: includes nothing of the project but csrc/fused_plan.h and walks
// the grid of tests/test_host_head_ride.py (head rows x patches per row x strip shape x workgroups x what the step is).  One line per query: the 29 query
// fields, '|', the 8 ride-query fields, '|', ok, why, rows, first item.  For every query that rides, the properties of the item order are checked here:
// every riding row (the first n of the head's) is one item behind every strip item, the strips of a row lie inside the launch, and each of them has its samples written by an earlier item.
// A violated property ends the run with status 1.
#include <cstdio>
#include <tuple>
#include <vector>

#include "fused_plan.h"

using fused_plan::Plan;
using fused_plan::Query;
using fused_plan::Ride;
using fused_plan::RideQuery;

static int fail(const char* what, long a, long b) {
  fprintf(stderr, "%s (%ld, %ld)\n", what, a, b);
  return 1;
}

int main() {
  long n = 0, riding = 0;
  const long shapes[] = {0, 2, 6};        // 64-column strips on 16 waves; 32 columns on 8 (two per CU); 16 columns
  const long sides[] = {8, 12, 16, 28};   // image side of the conv layer (5 x 5 patches, stride 2 or 1)
  for (long rows = 1; rows <= 12; ++rows)
    for (long side : sides)
      for (long stride = 1; stride <= 2; ++stride)
        for (long shape : shapes)
          for (long wgs = 1; wgs <= 6; ++wgs)
            for (int variant = 0; variant < 10; ++variant) {   // 0: as chosen; 8, 9: forced counts; the others: something keeps the rows off the launch
              const long o = (side - 5) / stride + 1, P = o * o;
              Query q;
              q.M = 32; q.Mp = 32; q.R = 10; q.Rp = 16; q.P = P; q.Kc = rows * P; q.HWC = side * side; q.L = 25; q.Lp = 28; q.Lz = 28; q.f = 5; q.C = 1;
              q.n_mod = rows; q.has_G = 1; q.n_cus = 256;
              q.fused_shape = shape; q.fused_persist = variant == 7 ? 2 : 1; q.fused_wgs = wgs;
              RideQuery r;
              r.next_is_head = variant != 1; r.head_form = variant != 2; r.head_HWC = P * q.R; r.head_lds = 16 * 1024; r.head_nfm = 2;
              r.in_flight = variant == 3; r.head_ride = variant == 4 ? 0 : (variant == 8 ? rows : (variant == 9 ? (rows + 1) / 2 : -1));
              q.keeps_state = variant == 5; q.has_trace = variant == 6;
              const Plan p = fused_plan::plan_layer_launch(q);
              const Ride rd = fused_plan::plan_head_ride(q, p, r);
              std::apply([&](const auto&... f) { (printf("%ld ", (long)f), ...); }, Query::fields(q));
              printf("| %ld %ld %ld %ld %ld %ld %ld %ld | %d %d %d %d\n", r.next_is_head, r.head_form, r.head_HWC, r.head_lds, r.head_nfm, r.in_flight, r.chain_beside,
                     r.head_ride, rd.ok, rd.why, rd.n_rows, rd.first_item);
              ++n;
              if (!rd.ok) {
                if (rd.why == fused_plan::kRides || rd.n_rows != 0) return fail("a query that does not ride must say why", rd.why, rd.n_rows);
                continue;
              }
              ++riding;
              if (variant != 0 && variant < 8) return fail("only the plain synchronous forward step rides", variant, rd.why);
              const long BN = fused_plan::kShapes[p.shape].FN * 16;
              if (rd.n_rows < 1 || rd.n_rows > rows || rd.first_item != p.n_items) return fail("one item per riding row, behind the plan's items", rd.n_rows, rd.first_item);
              if (variant == 8 && rd.n_rows != rows) return fail("a forced count of all rows", rd.n_rows, rows);
              if (variant == 9 && rd.n_rows != (rows + 1) / 2) return fail("a forced count", rd.n_rows, rows);
              if (variant == 0 && rd.n_rows != std::min(fused_plan::ride_room(q, p), rows)) return fail("the chosen count is the deal's room", rd.n_rows, rows);
              std::vector<int> seen((size_t)rows, 0);
              for (long item = rd.first_item; item < rd.first_item + rd.n_rows; ++item) {
                const long row = item - rd.first_item;
                ++seen[(size_t)row];
                long lo, hi;
                fused_plan::ride_row_strips(row, P, BN, &lo, &hi);
                if (lo < 0 || hi >= p.n_strips || lo > hi) return fail("a row's strips lie inside the launch", lo, hi);
                if (lo * BN > row * P || (hi + 1) * BN < (row + 1) * P) return fail("a row's strips cover its columns", lo, hi);
                for (long st = lo; st <= hi; ++st) {
                  const long w = fused_plan::ride_sample_item(p, st);
                  if (w < 0 || w >= p.n_items || w >= item) return fail("a strip's samples are written by an earlier item", w, item);
                }
              }
              for (long row = 0; row < rows; ++row)   // (the rows beyond the count stay in the head's own launch)
                if (seen[(size_t)row] != (row < rd.n_rows ? 1 : 0)) return fail("every riding row is run once, no other", row, seen[(size_t)row]);
            }
  fprintf(stderr, "%ld queries, %ld ride\n", n, riding);
  return riding > 0 ? 0 : 1;
}

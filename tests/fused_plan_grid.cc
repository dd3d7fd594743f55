// The layer kernel's launch planner on its own: includes nothing of the project but csrc/fused_plan.h, walks the grid of tests/test_host_fused_plan.py
// (strips 1..40 x workgroups 1..8 x R in {1, 2, 3, 10} x every tiling of the rows x three settings of the deal) and prints one line per
// query: the 29 query fields, '|', the 21 integer plan fields and the three makespans.  The test compiles it with the host compiler and compares every line
// with what the library answers; each query is planned twice, and a second answer that differs from the first ends the run with status 1.
#include <cstdio>
#include <cstring>
#include <tuple>

#include "fused_plan.h"

using fused_plan::Plan;
using fused_plan::Query;

static void format_plan(char* out, size_t cap, const Query& q, const Plan& p) {
  size_t at = 0;
  std::apply([&](const auto&... f) { ((at += snprintf(out + at, cap - at, "%ld ", (long)f)), ...); }, Query::fields(q));
  snprintf(out + at, cap - at, "| %d %d %ld %d %d %ld %d %d %d %d %d %d %d %d %d %d %d %ld %d %d %d %.17g %.17g %.17g", p.ok, p.shape, p.lds, p.lds_main, p.lds_img,
           p.grid, p.persist, p.n_strips, p.n_items, p.deal, p.split_first, p.split_q, p.pre_n, p.pre_first, p.pre_sq, p.pre_D, p.pre_whole, p.pre_stride,
           p.stagger, p.cu_slots, p.patch_rows, p.units_plain, p.units_ahead, p.units_shared);
}

int main() {
  const long Rs[] = {1, 2, 3, 10};
  long n = 0;
  for (long strips = 1; strips <= 40; ++strips)
    for (long wgs = 1; wgs <= 8; ++wgs)
      for (long R : Rs)
        for (long n_mod = 1; n_mod <= strips; ++n_mod) {   // n_mod == strips: untiled rows
          if (strips % n_mod) continue;
          for (int variant = 0; variant < 3; ++variant) {   // the deal forced persistent; as chosen; as chosen, with parts
            Query q;   // 12 x 12 x 1 images, 5 x 5 patches at stride 2: 16 patches, one 16-column strip (shape 6) per image
            q.M = 32; q.Mp = 32; q.R = R; q.Rp = 16; q.P = 16; q.Kc = strips * q.P; q.HWC = 144; q.L = 25; q.Lp = 28; q.Lz = 28; q.f = 5; q.C = 1;
            q.n_mod = n_mod; q.has_G = 1; q.n_cus = 256;
            q.fused_shape = 6; q.fused_persist = variant == 0 ? 1 : -1; q.fused_parts = variant == 2 ? 3 : -1; q.fused_wgs = wgs;
            char first[1024], again[1024];
            format_plan(first, sizeof first, q, fused_plan::plan_layer_launch(q));
            format_plan(again, sizeof again, q, fused_plan::plan_layer_launch(q));
            if (strcmp(first, again)) { fprintf(stderr, "the memo answers differently\n"); return 1; }
            puts(first);
            ++n;
          }
        }
  fprintf(stderr, "%ld queries\n", n);
  return 0;
}

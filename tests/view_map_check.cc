// view_map_check.cc -- walks the index arithmetic of the view gather (deepcgp_amd/csrc/augment.hip: view_images_kernel) on the host, with the
// functions of deepcgp_amd/csrc/augment_map.h it is made of: view_row (destination row -> view and source image), view_draw (the table row) and,
// row by row as augment_image does, augment_source_in_row.  tests/test_host_tta.py compares the output with deepcgp_amd/augment.py's
// apply_views.  Includes the header and nothing else of the project.
//   view_map_check map n H W C dy dx flip [dy dx flip ...]    one line per destination row r of the view-major batch [V n]: the index into the
//                                                              source batch [n][H][W][C] (or -1 for fill) of every destination value, in order.
//                                                              Exit 3 if an index leaves the source batch or a row's (view, image) its ranges.
//   view_map_check table per_axis H W dy dx flip [dy dx flip ...]   prints "ok" or what view_table_error says (per_axis: 0 or 1)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "augment_map.h"

int main(int argc, char** argv) {
  if (argc >= 9 && (argc - 6) % 3 == 0 && !strcmp(argv[1], "map")) {
    const int n = atoi(argv[2]), H = atoi(argv[3]), W = atoi(argv[4]), C = atoi(argv[5]), V = (argc - 6) / 3;
    std::vector<int32_t> views;
    for (int a = 6; a < argc; ++a) views.push_back(atoi(argv[a]));
    const int WC = W * C;
    const long len = (long)H * WC;
    for (long r = 0; r < (long)V * n; ++r) {
      const ViewRow q = view_row(r, n);
      if (q.v < 0 || q.v >= V || q.i < 0 || q.i >= n || (long)q.v * n + q.i != r) return 3;
      const AugmentDraw d = view_draw(views.data(), q.v);
      for (int y = 0; y < H; ++y) {
        const int sy = y - d.dy;
        for (int j = 0; j < WC; ++j) {
          long s = -1;
          if (sy >= 0 && sy < H) {
            const int sj = augment_source_in_row(j, W, C, d.dx, d.flip);
            if (sj >= WC) return 3;
            if (sj >= 0) s = (long)q.i * len + (long)sy * WC + sj;
          }
          if (s >= (long)n * len) return 3;
          printf(y == 0 && j == 0 ? "%ld" : " %ld", s);
        }
      }
      printf("\n");
    }
    return 0;
  }
  if (argc >= 8 && (argc - 5) % 3 == 0 && !strcmp(argv[1], "table")) {
    const int per_axis = atoi(argv[2]), H = atoi(argv[3]), W = atoi(argv[4]), V = (argc - 5) / 3;
    std::vector<int32_t> views;
    for (int a = 5; a < argc; ++a) views.push_back(atoi(argv[a]));
    const char* why = view_table_error(views.data(), V, H, W, per_axis != 0);
    printf("%s\n", why ? why : "ok");
    return 0;
  }
  return 2;
}

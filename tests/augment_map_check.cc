// augment_map_check.cc -- prints the index map and the draws of deepcgp_amd/csrc/augment_map.h; tests/test_host_augment.py compares them with an
// np.flip / np.pad / slice formulation and with deepcgp_amd/augment.py.  Includes the header and nothing else of the project.
//   augment_map_check map H W C t          one line per (dy, dx, flip), dy and dx over [-t, t], flip over {0, 1}:
//                                          "dy dx flip" and then the source index (or -1) of every destination index, in order
//   augment_map_check draw t hflip n seed...   one line per seed (decimal, up to 2^64 - 1): "dy dx flip" of positions 0 .. n - 1
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "augment_map.h"

int main(int argc, char** argv) {
  if (argc == 6 && !strcmp(argv[1], "map")) {
    const int H = atoi(argv[2]), W = atoi(argv[3]), C = atoi(argv[4]), t = atoi(argv[5]);
    const long len = (long)H * W * C;
    for (int dy = -t; dy <= t; ++dy)
      for (int dx = -t; dx <= t; ++dx)
        for (int flip = 0; flip < 2; ++flip) {
          printf("%d %d %d", dy, dx, flip);
          for (long i = 0; i < len; ++i) printf(" %ld", augment_source_index(i, H, W, C, dy, dx, flip));
          printf("\n");
        }
    return 0;
  }
  if (argc >= 6 && !strcmp(argv[1], "draw")) {
    const int t = atoi(argv[2]), hflip = atoi(argv[3]), n = atoi(argv[4]);
    for (int a = 5; a < argc; ++a) {
      const uint64_t seed = strtoull(argv[a], nullptr, 10);
      for (int b = 0; b < n; ++b) {
        const AugmentDraw d = augment_draw(seed, (uint64_t)b, t, hflip);
        printf("%d %d %d ", d.dy, d.dx, d.flip);
      }
      printf("\n");
    }
    return 0;
  }
  return 2;
}

// pad_map_check.cc -- prints the index map of deepcgp_amd/csrc/pad_map.h for one shape; tests/test_host_padding.py compares it with np.pad.
// Includes the header and nothing else of the project.  usage: pad_map_check rows H W C p
//   line 1: the source index (or -1) of every padded index, in order;  line 2: the padded index of every source index, in order
#include <cstdio>
#include <cstdlib>

#include "pad_map.h"

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int rows = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]), C = atoi(argv[4]), p = atoi(argv[5]);
  const long n_pad = (long)rows * (H + 2 * p) * (W + 2 * p) * C, n_src = (long)rows * H * W * C;
  for (long i = 0; i < n_pad; ++i) printf("%ld ", pad_source_index(i, H, W, C, p));
  printf("\n");
  for (long j = 0; j < n_src; ++j) printf("%ld ", pad_padded_index(j, H, W, C, p));
  printf("\n");
  return 0;
}

// dilate_map_check.cc -- prints the index map of deepcgp_amd/csrc/dilate_map.h for one shape; tests/test_host_dilation.py compares it with
// NumPy slicing x[:, a::d, b::d].  Includes the header and nothing else of the project.  usage: dilate_map_check rows H W C d
//   line 1: the image index (or -1 on the fill) of every phase index, in order;  line 2: the phase index of every image index, in order
#include <cstdio>
#include <cstdlib>

#include "dilate_map.h"

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int rows = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]), C = atoi(argv[4]), d = atoi(argv[5]);
  const long n_img = (long)rows * H * W * C;
  const long n_ph = (long)rows * d * d * dilate_ceil_div(H, d) * dilate_ceil_div(W, d) * C;
  for (long i = 0; i < n_ph; ++i) printf("%ld ", s2b_source_index(i, H, W, C, d));
  printf("\n");
  for (long j = 0; j < n_img; ++j) printf("%ld ", s2b_phase_index(j, H, W, C, d));
  printf("\n");
  return 0;
}

// csrc/mesh_simplify_math.h built by a host compiler into a program of its own: tests/test_mesh_simplify_host.py runs
// it, so that the cell arithmetic of csrc/mesh_simplify.hip is checked against numpy's float64 floor without a GPU.
//
//   mesh_simplify_host_check H ORIGIN BITS...     H, ORIGIN: doubles as strtod reads them (C99 hexadecimal floats are
//                                                 exact); BITS: the bit patterns of float32 coordinates, in decimal
// prints one line per coordinate: its cell index, or -2 (not finite) or -4 (out of range); then, for every three
// coordinates in turn, "key K" with the cell key of that point about the origin (ORIGIN, ORIGIN, ORIGIN), or "key -S"
// with the status bits S.
#include "mesh_simplify_math.h"
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const double h = strtod(argv[1], nullptr), o = strtod(argv[2], nullptr);
  const int n = argc - 3;
  float* x = (float*)malloc(sizeof(float) * (size_t)(n > 0 ? n : 1));
  for (int i = 0; i < n; ++i) {
    const uint32_t bits = (uint32_t)strtoul(argv[3 + i], nullptr, 10);
    memcpy(&x[i], &bits, sizeof bits);
    int64_t index = 0;
    const int bad = gsr::simplify_cell_index(x[i], o, h, &index);
    printf("%" PRId64 "\n", bad ? -(int64_t)bad : index);
  }
  const double origin[3] = {o, o, o};
  for (int i = 0; i + 2 < n; i += 3) {
    int64_t key = 0;
    const int bad = gsr::simplify_cell_key(x + i, origin, h, &key);
    printf("key %" PRId64 "\n", bad ? -(int64_t)bad : key);
  }
  free(x);
  return 0;
}

// csrc/icp_math.h -- the bodies of icp_transform_kernel and of the pair loop of icp_accumulate_kernel -- built by the host
// compiler with the kernel's -ffp-contract=off and run over pairs that tests/test_icp_host.py writes: the transformed
// coordinates and the 17 terms of every pair must be those of the numpy restatement (tests/icp_restate.py) bit for bit.
// Stand-alone: it may be built with -fsanitize=address,undefined and run directly.
//
//   icp_host_check <file>  ->  per pair one line: accepted (0 / 1), 3 hex words (the float32 bits of M p) and 17 hex
//                              words (the float64 bits of the terms of the pair (M p, r))
//
// The file, little endian: double[12] the 3x4 matrix, double[6] the pivots c_q, c_r, float thr2, int32 R, int32 n, then n
// records of float[3] p, float[3] r, float dist2, int32 nearest.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "icp_math.h"

namespace {

template <typename T>
bool get(FILE* f, T* out, size_t n) {
  return fread(out, sizeof(T), n, f) == n;
}

struct Record {
  float p[3], r[3], dist2;
  int32_t nearest;
};
static_assert(sizeof(Record) == 32, "packed as the test writes it");

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  gsr::IcpMatrix M;
  gsr::IcpPivots c;
  float thr2;
  int32_t Rn[2];
  if (!get(f, M.m, 12) || !get(f, c.cq, 3) || !get(f, c.cr, 3) || !get(f, &thr2, 1) || !get(f, Rn, 2) || Rn[1] < 0) return 4;
  std::vector<Record> records((size_t)Rn[1]);
  if (!get(f, records.data(), records.size())) return 5;
  fclose(f);
  for (const Record& rec : records) {
    float q[3];
    gsr::icp_transform_point(M, rec.p, q);
    double t[gsr::ICP_SUMS];
    gsr::icp_pair_terms(q, rec.r, rec.dist2, c, t);
    printf("%d", gsr::icp_pair_accepted(rec.dist2, thr2, rec.nearest, Rn[0]) ? 1 : 0);
    for (int a = 0; a < 3; ++a) {
      uint32_t bits;
      memcpy(&bits, &q[a], 4);
      printf(" %08" PRIx32, bits);
    }
    for (int k = 0; k < gsr::ICP_SUMS; ++k) {
      uint64_t bits;
      memcpy(&bits, &t[k], 8);
      printf(" %016" PRIx64, bits);
    }
    printf("\n");
  }
  return 0;
}

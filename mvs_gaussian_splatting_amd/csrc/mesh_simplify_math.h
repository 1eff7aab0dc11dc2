// The cell of a vertex on the clustering grid of csrc/mesh_simplify.hip (mesh.simplify_mesh), written
// once for device and host: tests/mesh_simplify_host_check.cpp builds it with the host compiler, so the floor and the
// half-open cell are checked against numpy's float64 without a GPU.
//
// With h the cell size and o the origin, both doubles: i = floor(((double)x - o) / h) per axis, one IEEE subtraction,
// one IEEE division and one floor, so numpy's float64 gives the same integer.  A cell holds o + i h <= x < o + (i + 1) h
// up to the rounding of that quotient.  Every index must lie in 0 .. 2^21 - 1; key = ix << 42 | iy << 21 | iz.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GSR_HD __host__ __device__ inline
#else
#define GSR_HD inline
#endif

namespace gsr {

constexpr int SIMPLIFY_CELL_BITS = 21;
constexpr int64_t SIMPLIFY_NO_CELL = INT64_MAX;   // the key of a vertex that takes no part: sorts behind every cell

// bits of the status word (include/gsr.h: GSR_SIMPLIFY_*)
constexpr int SIMPLIFY_BAD_INDEX = 1, SIMPLIFY_NOT_FINITE = 2, SIMPLIFY_OUT_OF_RANGE = 4;

// -> 0 and *index, or the status bit that refuses the coordinate (*index is not written then)
GSR_HD int simplify_cell_index(float x, double o, double h, int64_t* index) {
  if (!(fabsf(x) <= FLT_MAX)) return SIMPLIFY_NOT_FINITE;
  const double t = floor(((double)x - o) / h);
  // compared as doubles: a quotient beyond int64 (or a NaN from an origin that is not finite) is never converted
  if (!(t >= 0.0 && t < (double)((int64_t)1 << SIMPLIFY_CELL_BITS))) return SIMPLIFY_OUT_OF_RANGE;
  *index = (int64_t)t;
  return 0;
}

// -> 0 and *key, or the status bits of the coordinates that were refused (*key = SIMPLIFY_NO_CELL then)
GSR_HD int simplify_cell_key(const float p[3], const double o[3], double h, int64_t* key) {
  int64_t i[3] = {0, 0, 0};
  int bad = 0;
  for (int a = 0; a < 3; ++a) bad |= simplify_cell_index(p[a], o[a], h, &i[a]);
  *key = bad ? SIMPLIFY_NO_CELL : (i[0] << (2 * SIMPLIFY_CELL_BITS)) | (i[1] << SIMPLIFY_CELL_BITS) | i[2];
  return bad;
}

}  // namespace gsr

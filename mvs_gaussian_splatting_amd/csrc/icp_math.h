// The per-point arithmetic of csrc/icp.hip (geometry_eval.icp_step / icp_registration), written once for
// device and host: tests/icp_host_check.cpp builds it with the host compiler and the kernel's -ffp-contract=off, so the
// transformed bits and the per-pair terms are checked against numpy's float64 (tests/icp_restate.py) without a GPU.
//
// Transform.  m is the upper 3x4 of a similarity, row-major doubles (s R | t).  Per output axis, with the float32
// coordinates widened exactly: fl(fl(fl(fl(m0 x) + fl(m1 y)) + fl(m2 z)) + m3) in float64, every operation rounded on
// its own (no fused multiply-add), then ONE rounding to float32.
//
// Pair terms.  For an accepted pair (q, r) and the float64 pivots c_q, c_r: a = (double)q - c_q, b = (double)r - c_r
// (one subtraction each), and the 17 terms in the order of ICP_SUMS below: a (3), b (3), a_i b_j row-major (9, one
// multiplication each), fl(fl(a0 a0 + a1 a1) + a2 a2) (1), (double)dist2 (1).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GSR_HD __host__ __device__ inline
#else
#define GSR_HD inline
#endif

namespace gsr {

constexpr int ICP_SUMS = 17;            // doubles behind the int64 count: Σa, Σb, Σ a bᵀ, Σ|a|², Σ dist2
constexpr int ICP_WORDS = 1 + ICP_SUMS;  // 8-byte words of a result and of a partial

struct IcpMatrix {
  double m[12];
};
struct IcpPivots {
  double cq[3], cr[3];
};

GSR_HD float icp_transform_axis(const double* row, float x, float y, float z) {
  const double v = ((row[0] * (double)x + row[1] * (double)y) + row[2] * (double)z) + row[3];
  return (float)v;
}

GSR_HD void icp_transform_point(const IcpMatrix& M, const float p[3], float out[3]) {
  for (int a = 0; a < 3; ++a) out[a] = icp_transform_axis(M.m + 4 * a, p[0], p[1], p[2]);
}

// the pair test: dist2 <= thr2 (inclusive; a NaN is never accepted) and a neighbour that exists (-1: an empty target)
GSR_HD bool icp_pair_accepted(float dist2, float thr2, int32_t nearest, int32_t R) {
  return dist2 <= thr2 && (uint32_t)nearest < (uint32_t)R;
}

GSR_HD void icp_pair_terms(const float q[3], const float r[3], float dist2, const IcpPivots& c, double t[ICP_SUMS]) {
  double a[3], b[3];
  for (int i = 0; i < 3; ++i) {
    a[i] = (double)q[i] - c.cq[i];
    b[i] = (double)r[i] - c.cr[i];
  }
  for (int i = 0; i < 3; ++i) {
    t[i] = a[i];
    t[3 + i] = b[i];
    for (int j = 0; j < 3; ++j) t[6 + 3 * i + j] = a[i] * b[j];
  }
  t[15] = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
  t[16] = (double)dist2;
}

}  // namespace gsr

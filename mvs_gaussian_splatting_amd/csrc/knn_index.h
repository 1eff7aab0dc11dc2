// The Morton-box index over a point cloud that knn.hip builds and that knn.hip (distCUDA2) and nearest.hip (cross-set
// nearest point) query: the layout of the caller-owned buffer and the small helpers both sides need.
#pragma once
#include "gsr_common.h"
#include "gsr_launch.h"

namespace gsr {

constexpr int KNN_INDEX_BOX = 128;     // points per box (knn.hip: KNN_BOX)
constexpr int KNN_INDEX_SUPER = 64;    // boxes per super-box (knn.hip: KNN_SUPER)
constexpr int KNN_KEY_BITS = 30;    // 10 bits per axis

__device__ inline unsigned f2ord(float f) {   // order-preserving float -> uint
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float ord2f(unsigned o) {
  const unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float f; memcpy(&f, &u, 4); return f;
#endif
}

__device__ inline uint32_t spread10(uint32_t v) {   // 10 bits -> every third bit
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// 30-bit Morton code of a point in the frame of the encoded bounding box `mm` (3 min words, 3 max words), every axis
// clamped to 0..1023: points outside the box, and NaN (fmaxf / fminf return their other operand), get a code in range.
// A division and a multiplication, nothing a compiler can contract: the same bits in every translation unit.
__device__ inline uint32_t morton30(const float* __restrict__ p, const unsigned* __restrict__ mm) {
  uint32_t code = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = ord2f(mm[a]), hi = ord2f(mm[3 + a]);
    const float t = (p[a] - lo) / fmaxf(hi - lo, 1e-30f);
    const uint32_t q = (uint32_t)fminf(1023.0f, fmaxf(0.0f, t * 1023.0f));
    code |= spread10(q) << a;
  }
  return code;
}

// The index of N points.  mm, the sorted keys, spts, box_* and sup_* are what a query reads; the other key / value buffer
// and `sort` are the build's scratch, kept inside the index so that a build needs no second buffer.
struct KnnLayout {
  size_t mm, ka, kb, va, vb, spts, box_lo, box_hi, sup_lo, sup_hi, sort, bytes;
  int nboxes, nsuper;
  explicit KnnLayout(int N) {
    const size_t n = N > 0 ? (size_t)N : 1;
    nboxes = (int)((n + KNN_INDEX_BOX - 1) / KNN_INDEX_BOX);
    nsuper = (nboxes + KNN_INDEX_SUPER - 1) / KNN_INDEX_SUPER;
    size_t o = 0;
    mm = o;     o = align_up(o + 64, 256);
    ka = o;     o = align_up(o + 4 * n, 256);
    kb = o;     o = align_up(o + 4 * n, 256);
    va = o;     o = align_up(o + 4 * n, 256);
    vb = o;     o = align_up(o + 4 * n, 256);
    spts = o;   o = align_up(o + 16 * n, 256);
    box_lo = o; o = align_up(o + 12 * (size_t)nboxes, 256);
    box_hi = o; o = align_up(o + 12 * (size_t)nboxes, 256);
    sup_lo = o; o = align_up(o + 12 * (size_t)nsuper, 256);
    sup_hi = o; o = align_up(o + 12 * (size_t)nsuper, 256);
    sort = o;   o = align_up(o + SortLayout((uint32_t)n).bytes, 256);
    bytes = o;
  }
  // where the pair sort of KNN_KEY_BITS bits leaves the sorted keys: it ping-pongs once per pass
  size_t sorted_keys() const { return (sort_passes(KNN_KEY_BITS) & 1) ? kb : ka; }
};

// knn.hip: bounding box, Morton codes, sort, boxes and super-boxes of pts[N,3] into `index` (KnnLayout(N).bytes); N > 0
void launch_knn_build(const float* pts, int N, void* index, hipStream_t s);

}  // namespace gsr

// Cross-set nearest point: for every query point the exact nearest point of a REFERENCE cloud, the
// primitive under the Chamfer distance and the precision / recall / F-score of geometry_eval.py.  The reference is
// indexed by knn.hip's build (knn_index.h: Morton order, boxes of 128 sorted points, super-boxes of 64 boxes, each with
// its bounding box); this file holds the query.
//
// Definition.  d2(q, r) = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), dx = fl(q.x - r.x) and likewise dy, dz: float32,
// round to nearest, no fused multiply-add (this file is compiled with -ffp-contract=off).  The result is the minimum of
// d2 over the reference and, among the points that attain it, the smallest ORIGINAL index.  A float32 numpy brute force
// gives the same bits and the same index (tests/nearest_restate.py).
//
// Pruning.  A box is skipped only when its box distance bd is GREATER than the current best.  bd is formed with the same
// operations from ex = max(lo.x - q.x, q.x - hi.x, 0) and likewise ey, ez.  For a point r inside the box lo.x <= r.x <=
// hi.x, so the exact |q.x - r.x| is at least the exact value of whichever of lo.x - q.x, q.x - hi.x, 0 is largest;
// rounding to nearest is monotone and symmetric in sign, so |fl(q.x - r.x)| >= ex, then fl(dx dx) >= fl(ex ex), and both
// sums keep the order: bd <= d2(q, r) for every r of the box.  A skipped box therefore holds only points with d2 > best:
// none that improves the minimum and none that ties it.  Equality must open the box, or a tie with a smaller index
// inside it would be lost.  Within a box every point is visited, and (d2, index) is a total order, so the scan order and
// the order in which boxes are opened do not matter: the result depends on the two clouds alone.
//
// Order and starting bound.  Queries are not members of the reference, so each gets the 30-bit Morton code of its
// position in the reference's bounding-box frame (clamped to 0..1023 per axis: a query far outside gets the code of the
// nearest face cell), the queries are sorted by that code with the rasterizer's pair sort so that neighbouring lanes
// open the same boxes, and each query binary-searches its code in the reference's sorted keys and scans the box it
// lands in first.  Then it walks super-boxes and boxes as knn_query_kernel does, one lane per query, every lane reading
// the boxes it opens through L2.  Results are scattered by the query's original index.
//
// Safety.  Every loop is bounded at launch: 32 search steps, nsuper, KNN_INDEX_SUPER, KNN_INDEX_BOX.  No lane waits
// on another lane, wave or workgroup.  A query index read from the sorted values is checked against Q before use;
// the search position is clamped to 0..R-1; box and point indices are formed from loop counters clamped to nboxes
// and R.  R and Q are at most GSR_NN_MAX_POINTS = 2^31 - 256 (the entry points below refuse more), so first + KNN_INDEX_BOX
// and the index of the last workgroup's last lane stay inside int.  NaN / Inf coordinates give an unspecified value
// (a NaN distance compares false and is never kept) and change no bound.
#include <float.h>

#include "gsr_common.h"
#include "gsr_entry.h"
#include "gsr_launch.h"
#include "knn_index.h"

namespace gsr {

struct NnQueryLayout {
  size_t ka, kb, va, vb, sort, bytes;
  explicit NnQueryLayout(int Q) {
    const size_t n = Q > 0 ? (size_t)Q : 1;
    size_t o = 0;
    ka = o;   o = align_up(o + 4 * n, 256);
    kb = o;   o = align_up(o + 4 * n, 256);
    va = o;   o = align_up(o + 4 * n, 256);
    vb = o;   o = align_up(o + 4 * n, 256);
    sort = o; o = align_up(o + SortLayout((uint32_t)n).bytes, 256);
    bytes = o;
  }
};

__global__ __launch_bounds__(256) void nn_morton_kernel(const float* __restrict__ query, int Q,
                                                        const unsigned* __restrict__ mm, uint32_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Q) return;
  keys[i] = morton30(query + 3 * (size_t)i, mm);
  vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void nn_empty_kernel(int Q, float* __restrict__ dist2, int32_t* __restrict__ nearest) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Q) return;
  dist2[i] = __uint_as_float(0x7f800000u);
  nearest[i] = -1;
}

__device__ inline float nn_box_dist2(const float* __restrict__ lo, const float* __restrict__ hi, float px, float py, float pz) {
  const float ex = fmaxf(fmaxf(lo[0] - px, px - hi[0]), 0.0f);
  const float ey = fmaxf(fmaxf(lo[1] - py, py - hi[1]), 0.0f);
  const float ez = fmaxf(fmaxf(lo[2] - pz, pz - hi[2]), 0.0f);
  return ex * ex + ey * ey + ez * ez;
}

__global__ __launch_bounds__(256) void nn_query_kernel(int R, int Q, int nboxes, int nsuper,
                                                       const uint32_t* __restrict__ rkeys, const float4* __restrict__ spts,
                                                       const float* __restrict__ box_lo, const float* __restrict__ box_hi,
                                                       const float* __restrict__ sup_lo, const float* __restrict__ sup_hi,
                                                       const float* __restrict__ query, const uint32_t* __restrict__ qkeys,
                                                       const uint32_t* __restrict__ qidx, float* __restrict__ dist2,
                                                       int32_t* __restrict__ nearest) {
  const int s = blockIdx.x * 256 + threadIdx.x;   // queries in Morton order: neighbouring lanes open the same boxes
  if (s >= Q) return;
  const uint32_t qi = qidx[s];
  if (qi >= (uint32_t)Q) return;                  // never true after the sort; a scribbled workspace must not scatter
  const uint32_t code = qkeys[s];
  const float px = query[3 * (size_t)qi], py = query[3 * (size_t)qi + 1], pz = query[3 * (size_t)qi + 2];
  float best = __uint_as_float(0x7f800000u);
  uint32_t bi = 0xffffffffu;                      // -1: nothing found
  auto scan_box = [&](int b) {
    const int first = b * KNN_INDEX_BOX, last = min(R, first + KNN_INDEX_BOX);
    for (int j = first; j < last; ++j) {
      const float4 r = spts[j];
      const float dx = px - r.x, dy = py - r.y, dz = pz - r.z;
      const float d = dx * dx + dy * dy + dz * dz;
      const uint32_t i = __float_as_uint(r.w);
      if (d < best || (d == best && i < bi)) { best = d; bi = i; }
    }
  };
  // first sorted reference point whose key is not below the query's: at most 32 halvings of 0..R
  int lo = 0, hi = R;
  for (int step = 0; step < 32; ++step) {
    if (lo >= hi) break;
    const int mid = lo + (hi - lo) / 2;
    if (rkeys[mid] < code) lo = mid + 1; else hi = mid;
  }
  const int own = min(max(lo, 0), R - 1) / KNN_INDEX_BOX;
  scan_box(own);                                   // a bound before any pruning test
  for (int S = 0; S < nsuper; ++S) {
    if (!(nn_box_dist2(sup_lo + 3 * (size_t)S, sup_hi + 3 * (size_t)S, px, py, pz) <= best)) continue;
    const int b0 = S * KNN_INDEX_SUPER, b1 = min(nboxes, b0 + KNN_INDEX_SUPER);
    for (int b = b0; b < b1; ++b) {
      if (b == own) continue;
      if (nn_box_dist2(box_lo + 3 * (size_t)b, box_hi + 3 * (size_t)b, px, py, pz) <= best) scan_box(b);
    }
  }
  dist2[qi] = best;
  nearest[qi] = (int32_t)bi;
}

static void launch_nn_query(const void* index, int R, const float* query, int Q, float* dist2, int32_t* nearest, void* ws,
                            hipStream_t s) {
  const int nb = (Q + 255) / 256;
  if (R <= 0) {
    hipLaunchKernelGGL(nn_empty_kernel, dim3(nb), dim3(256), 0, s, Q, dist2, nearest);
    return;
  }
  const KnnLayout L(R);
  const NnQueryLayout W(Q);
  const char* b = static_cast<const char*>(index);
  char* w = static_cast<char*>(ws);
  uint32_t* ka = reinterpret_cast<uint32_t*>(w + W.ka);
  uint32_t* kb = reinterpret_cast<uint32_t*>(w + W.kb);
  uint32_t* va = reinterpret_cast<uint32_t*>(w + W.va);
  uint32_t* vb = reinterpret_cast<uint32_t*>(w + W.vb);
  hipLaunchKernelGGL(nn_morton_kernel, dim3(nb), dim3(256), 0, s, query, Q, reinterpret_cast<const unsigned*>(b + L.mm), ka, va);
  const bool in_b = launch_sort_pairs_u32(ka, va, kb, vb, (uint32_t)Q, KNN_KEY_BITS, w + W.sort, s);
  hipLaunchKernelGGL(nn_query_kernel, dim3(nb), dim3(256), 0, s, R, Q, L.nboxes, L.nsuper,
                     reinterpret_cast<const uint32_t*>(b + L.sorted_keys()), reinterpret_cast<const float4*>(b + L.spts),
                     reinterpret_cast<const float*>(b + L.box_lo), reinterpret_cast<const float*>(b + L.box_hi),
                     reinterpret_cast<const float*>(b + L.sup_lo), reinterpret_cast<const float*>(b + L.sup_hi), query,
                     in_b ? kb : ka, in_b ? vb : va, dist2, nearest);
}

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_nn_index_bytes(int32_t R) { return KnnLayout(R).bytes; }
size_t gsr_nn_query_workspace_bytes(int32_t Q) { return NnQueryLayout(Q).bytes; }
int gsr_nn_build(const float* ref, int32_t R, void* index, size_t index_bytes, void* stream) {
  if (R < 0 || R > GSR_NN_MAX_POINTS) return fail(GSR_E_BADARG, "R must lie in 0..2^31-256");
  if (R == 0) return 0;
  if (!ref || !index) return fail(GSR_E_BADARG, "NULL argument");
  if (index_bytes < KnnLayout(R).bytes) return fail(GSR_E_CAPACITY, "nn index too small");
  if (!aligned({index}, 255u)) return fail(GSR_E_ALIGN, "index must be 256-byte aligned");
  if (!aligned({ref}, 3u)) return fail(GSR_E_ALIGN, "ref must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_knn_build(ref, R, index, s);
  return check(false, s, "nn_build");
}
int gsr_nn_query(const void* index, size_t index_bytes, int32_t R, const float* query, int32_t Q, float* dist2,
                 int32_t* nearest, void* workspace, size_t workspace_bytes, void* stream) {
  if (R < 0 || Q < 0 || R > GSR_NN_MAX_POINTS || Q > GSR_NN_MAX_POINTS)
    return fail(GSR_E_BADARG, "R and Q must lie in 0..2^31-256");
  if (Q == 0) return 0;
  if (!query || !dist2 || !nearest) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({query, dist2, nearest}, 3u)) return fail(GSR_E_ALIGN, "query / dist2 / nearest must be 4-byte aligned");
  if (R > 0) {
    if (!index || !workspace) return fail(GSR_E_BADARG, "NULL index / workspace");
    if (index_bytes < KnnLayout(R).bytes) return fail(GSR_E_CAPACITY, "nn index too small");
    if (workspace_bytes < NnQueryLayout(Q).bytes) return fail(GSR_E_CAPACITY, "nn query workspace too small");
    if (!aligned({index, workspace}, 255u)) return fail(GSR_E_ALIGN, "index / workspace must be 256-byte aligned");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_nn_query(index, R, query, Q, dist2, nearest, workspace, s);
  return check(false, s, "nn_query");
}

}  // extern "C"

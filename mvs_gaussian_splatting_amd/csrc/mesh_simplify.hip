// Mesh simplification by vertex clustering on a uniform grid (Rossignac-Borrel; Open3D's simplify_vertex_clustering
// with the averaging contraction): the kernels around the caller's sorts and scans (include/gsr.h, ABI v39;
// mesh.simplify_mesh).
//
// Launch shape of every kernel here but one: 256-lane workgroups, one lane per vertex / sorted slot / cluster / face, a
// one-dimensional grid of ceil(n / 256) workgroups, no grid-stride loop and no persistence, no LDS.  The one is
// simplify_lowest_kernel, a grid-stride minimum over at most 1024 workgroups with 48 bytes of LDS.  No float atomics
// anywhere: the atomics are the integer OR that sets a bit of the status word and the integer minimum of the default
// origin, both independent of the order they land in.  Nothing waits on another lane (the one barrier is reached by
// every lane of its workgroup).  The other loop is the walk of a run in simplify_reduce_kernel, bounded by the run's end.
//
//   * simplify_lowest_kernel      the default origin: the per-axis minimum of the finite coordinates of the marked
//                                 vertices, as an integer atomicMin on float bits mapped to integers of the same order
//                                 (one per workgroup and axis); simplify_origin_kernel turns it into
//                                 origin = (double)min - h / 2.  (torch's where + amin over [V,3] took a third of the
//                                 whole call.)
//   * simplify_cell_keys_kernel   key[v] = the cell of vertex v (mesh_simplify_math.h) where vertex_mark[v], else
//                                 SIMPLIFY_NO_CELL, which sorts last.  A marked vertex with a coordinate that is not finite
//                                 or a cell index outside 0 .. 2^21 - 1 sets its status bit and gets SIMPLIFY_NO_CELL too.
//   (the caller sorts the keys, stably: the members of a cell stay in ascending vertex index)
//   * simplify_run_heads_kernel   head[i] = 1 where sorted slot i holds a cell that slot i - 1 does not.
//   (the caller scans the heads: ends[i] - 1 is the cluster of slot i, ends[V - 1] = K)
//   * simplify_starts_kernel      start[c] = the first slot of cluster c, start[K] = the first slot with no cell (or V);
//                                 cluster_of_vertex[order[i]] = the cluster of slot i, -1 for a slot with no cell.
//   * simplify_reduce_kernel      one lane per cluster walks start[c] .. start[c + 1]: gathers the members' rows through
//                                 `order`, sums them in float64 from the first member on (not from 0, so a run of one is a
//                                 bit-copy, -0.0 included) and writes sum / n rounded to float32 once.  Neighbouring lanes
//                                 own neighbouring runs, so their `order` reads share cache lines; the rows themselves
//                                 are a gather of 12-byte rows that neighbouring vertices of a TSDF mesh mostly share
//                                 lines for.  The order of the sum is the run's, a fixed function of the input.
//   * simplify_face_keys_kernel   tri[f] = the clusters of face f's corners in corner order; keep[f] = no two are equal;
//                                 the triple rotated so that its smallest index comes first (the winding stays) as two
//                                 sort keys, first << 32 | second and third, or the largest keys for a dropped face.
//   (the caller sorts by the third index, then stably by the first two: equal triples become neighbours, smallest face
//    first)
//   * simplify_face_unique_kernel a slot whose rotated triple equals its predecessor's clears its face's keep flag.
//   * simplify_vertex_map_kernel  vertex_cluster[v] = the compacted index of v's cluster, or -1.
//
// No index read from memory is used unchecked: an order[], start[] or cluster value outside its range sets
// SIMPLIFY_BAD_INDEX and is skipped.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "mesh_simplify_math.h"

namespace gsr {

namespace {

constexpr int SIMPLIFY_BLOCK = 256;
constexpr int64_t FACE_KEY_DROPPED = INT64_MAX;

static_assert(SIMPLIFY_BAD_INDEX == GSR_SIMPLIFY_BAD_INDEX && SIMPLIFY_NOT_FINITE == GSR_SIMPLIFY_NOT_FINITE &&
                  SIMPLIFY_OUT_OF_RANGE == GSR_SIMPLIFY_OUT_OF_RANGE, "status bits of include/gsr.h");

constexpr int LOWEST_MAX_BLOCKS = 1024;

// float bits -> an int32 that orders as the floats do (finite values; -0.0 below +0.0), and back
__device__ __forceinline__ int32_t float_order(int32_t bits) { return bits >= 0 ? bits : bits ^ 0x7fffffff; }

__global__ void simplify_lowest_init_kernel(int32_t* lowest) {
  if (threadIdx.x < 3) lowest[threadIdx.x] = INT32_MAX;
}

__global__ void __launch_bounds__(SIMPLIFY_BLOCK) simplify_lowest_kernel(const float* vertices, const uint8_t* vertex_mark,
                                                                         int64_t V, int32_t* lowest) {
  __shared__ int32_t part[SIMPLIFY_BLOCK / WAVE][3];
  int32_t m[3] = {INT32_MAX, INT32_MAX, INT32_MAX};
  const int64_t stride = (int64_t)gridDim.x * SIMPLIFY_BLOCK;
  for (int64_t v = (int64_t)blockIdx.x * SIMPLIFY_BLOCK + threadIdx.x; v < V; v += stride) {
    if (!vertex_mark[v]) continue;
    for (int a = 0; a < 3; ++a) {
      const float x = vertices[3 * v + a];
      // a coordinate that is not finite has no place in the minimum; the key kernel refuses its vertex
      if (fabsf(x) <= FLT_MAX) m[a] = min(m[a], float_order(__float_as_int(x)));
    }
  }
  for (int a = 0; a < 3; ++a)
    for (int d = WAVE / 2; d > 0; d >>= 1) m[a] = min(m[a], __shfl_xor(m[a], d, WAVE));
  if ((threadIdx.x & (WAVE - 1)) == 0)
    for (int a = 0; a < 3; ++a) part[threadIdx.x / WAVE][a] = m[a];
  __syncthreads();                                    // every lane of the workgroup arrives: no return above
  if (threadIdx.x < 3) {
    int32_t r = part[0][threadIdx.x];
    for (int w = 1; w < SIMPLIFY_BLOCK / WAVE; ++w) r = min(r, part[w][threadIdx.x]);
    if (r != INT32_MAX) atomicMin(lowest + threadIdx.x, r);
  }
}

__global__ void simplify_origin_kernel(const int32_t* lowest, double h, double* origin) {
  // no finite marked coordinate at all: INT32_MAX are the bits of a NaN, and the key kernel refuses every vertex
  if (threadIdx.x < 3) origin[threadIdx.x] = (double)__int_as_float(float_order(lowest[threadIdx.x])) - h / 2.0;
}

__global__ void __launch_bounds__(SIMPLIFY_BLOCK) simplify_cell_keys_kernel(const float* vertices,
                                                                            const uint8_t* vertex_mark, int64_t V,
                                                                            const double* origin, double h, int64_t* keys,
                                                                            int32_t* status) {
  const int64_t v = (int64_t)blockIdx.x * SIMPLIFY_BLOCK + threadIdx.x;
  if (v >= V) return;
  int64_t key = SIMPLIFY_NO_CELL;
  if (vertex_mark[v]) {
    const float p[3] = {vertices[3 * v], vertices[3 * v + 1], vertices[3 * v + 2]};
    const double o[3] = {origin[0], origin[1], origin[2]};
    const int bad = simplify_cell_key(p, o, h, &key);
    if (bad) atomicOr(status, bad);
  }
  keys[v] = key;
}

__global__ void __launch_bounds__(SIMPLIFY_BLOCK) simplify_run_heads_kernel(const int64_t* keys_sorted, int64_t V,
                                                                            uint8_t* head) {
  const int64_t i = (int64_t)blockIdx.x * SIMPLIFY_BLOCK + threadIdx.x;
  if (i >= V) return;
  const int64_t k = keys_sorted[i];
  head[i] = k != SIMPLIFY_NO_CELL && (i == 0 || keys_sorted[i - 1] != k);
}

__global__ void __launch_bounds__(SIMPLIFY_BLOCK) simplify_starts_kernel(const int64_t* keys_sorted, const int64_t* order,
                                                                         const int64_t* ends, int64_t V, int64_t K,
                                                                         int32_t* start, int32_t* cluster_of_vertex,
                                                                         int32_t* status) {
  const int64_t i = (int64_t)blockIdx.x * SIMPLIFY_BLOCK + threadIdx.x;
  if (i >= V) return;
  const int64_t k = keys_sorted[i];
  const bool live = k != SIMPLIFY_NO_CELL;
  const bool first = i == 0 || keys_sorted[i - 1] != k;
  const int64_t c = ends[i] - 1;
  const int64_t v = order[i];
  if ((uint64_t)v >= (uint64_t)V || (live && (uint64_t)c >= (uint64_t)K)) {
    atomicOr(status, SIMPLIFY_BAD_INDEX);
    return;
  }
  cluster_of_vertex[v] = live ? (int32_t)c : -1;
  if (live && first) start[c] = (int32_t)i;
  if (!live && first) start[K] = (int32_t)i;          // the one slot where the cells end
  if (live && i == V - 1) start[K] = (int32_t)V;      // or every vertex has a cell
}

__global__ void __launch_bounds__(SIMPLIFY_BLOCK) simplify_reduce_kernel(const float* vertices, const float* colors,
                                                                         const int64_t* order, const int32_t* start,
                                                                         int64_t V, int64_t K, float* out_vertices,
                                                                         float* out_colors, int32_t* status) {
  const int64_t c = (int64_t)blockIdx.x * SIMPLIFY_BLOCK + threadIdx.x;
  if (c >= K) return;
  const int64_t lo = start[c], hi = start[c + 1];
  if (lo < 0 || hi <= lo || hi > V) {
    atomicOr(status, SIMPLIFY_BAD_INDEX);
    return;
  }
  double sp[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0};
  for (int64_t i = lo; i < hi; ++i) {                 // hi - lo steps: the members of cell c in ascending vertex index
    const int64_t v = order[i];
    if ((uint64_t)v >= (uint64_t)V) {
      atomicOr(status, SIMPLIFY_BAD_INDEX);
      return;
    }
    for (int a = 0; a < 3; ++a) {
      const double x = (double)vertices[3 * v + a];
      sp[a] = i == lo ? x : sp[a] + x;
    }
    if (colors)
      for (int a = 0; a < 3; ++a) {
        const double x = (double)colors[3 * v + a];
        sc[a] = i == lo ? x : sc[a] + x;
      }
  }
  const double n = (double)(hi - lo);
  for (int a = 0; a < 3; ++a) out_vertices[3 * c + a] = (float)(sp[a] / n);
  if (colors)
    for (int a = 0; a < 3; ++a) out_colors[3 * c + a] = (float)(sc[a] / n);
}

__global__ void __launch_bounds__(SIMPLIFY_BLOCK) simplify_face_keys_kernel(const int32_t* faces,
                                                                            const int32_t* cluster_of_vertex, int64_t F,
                                                                            uint32_t V, uint32_t K, int32_t* tri,
                                                                            uint8_t* keep, int64_t* key_first,
                                                                            int32_t* key_third, int32_t* status) {
  const int64_t f = (int64_t)blockIdx.x * SIMPLIFY_BLOCK + threadIdx.x;
  if (f >= F) return;
  int32_t c[3] = {0, 0, 0};
  bool ok = true;
  for (int a = 0; a < 3; ++a) {
    const int32_t v = faces[3 * f + a];
    ok = ok && (uint32_t)v < V;
    if (ok) {
      c[a] = cluster_of_vertex[v];
      ok = (uint32_t)c[a] < K;
    }
  }
  if (!ok) {                                          // a corner outside 0..V-1 or without a cluster: refused, dropped
    atomicOr(status, SIMPLIFY_BAD_INDEX);
    c[0] = c[1] = c[2] = 0;
  }
  for (int a = 0; a < 3; ++a) tri[3 * f + a] = c[a];
  const bool alive = c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
  keep[f] = alive;
  // three different indices: the smallest is one of them alone
  const int r = c[0] < c[1] ? (c[0] < c[2] ? 0 : 2) : (c[1] < c[2] ? 1 : 2);
  const int32_t r0 = c[r], r1 = c[r == 2 ? 0 : r + 1], r2 = c[r == 0 ? 2 : r - 1];
  key_first[f] = alive ? (int64_t)(((uint64_t)(uint32_t)r0 << 32) | (uint64_t)(uint32_t)r1) : FACE_KEY_DROPPED;
  key_third[f] = alive ? r2 : INT32_MAX;
}

__global__ void __launch_bounds__(SIMPLIFY_BLOCK) simplify_face_unique_kernel(const int64_t* first_sorted,
                                                                              const int64_t* perm,
                                                                              const int32_t* key_third, int64_t F,
                                                                              uint8_t* keep, int32_t* status) {
  const int64_t i = (int64_t)blockIdx.x * SIMPLIFY_BLOCK + threadIdx.x + 1;
  if (i >= F) return;
  const int64_t k = first_sorted[i];
  if (k == FACE_KEY_DROPPED || first_sorted[i - 1] != k) return;
  const int64_t fa = perm[i - 1], fb = perm[i];
  if ((uint64_t)fa >= (uint64_t)F || (uint64_t)fb >= (uint64_t)F) {
    atomicOr(status, SIMPLIFY_BAD_INDEX);
    return;
  }
  // the sorts are stable: fb is not the smallest face of its triple.  Only slot i writes keep[fb].
  if (key_third[fa] == key_third[fb]) keep[fb] = 0;
}

__global__ void __launch_bounds__(SIMPLIFY_BLOCK) simplify_vertex_map_kernel(const int32_t* cluster_of_vertex,
                                                                             const uint8_t* cluster_mark,
                                                                             const int64_t* cluster_offs, int64_t V,
                                                                             uint32_t K, int32_t* vertex_cluster) {
  const int64_t v = (int64_t)blockIdx.x * SIMPLIFY_BLOCK + threadIdx.x;
  if (v >= V) return;
  const int32_t c = cluster_of_vertex[v];
  vertex_cluster[v] = ((uint32_t)c < K && cluster_mark[c]) ? (int32_t)cluster_offs[c] : -1;
}

inline dim3 simplify_grid(int64_t n) { return dim3((unsigned)((n + SIMPLIFY_BLOCK - 1) / SIMPLIFY_BLOCK)); }
inline bool simplify_size_ok(int64_t n) { return n >= 1 && n <= (int64_t)INT32_MAX; }

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h): every size is checked to lie in 1 .. 2^31 - 1, every pointer for NULL and alignment
using namespace gsr;

extern "C" {

int gsr_simplify_default_origin(const float* vertices, const uint8_t* vertex_mark, int64_t V, double voxel_size,
                                int32_t* lowest, double* origin, void* stream) {
  if (!simplify_size_ok(V)) return fail(GSR_E_BADARG, "V must lie in 1..2^31-1");
  if (!vertices || !vertex_mark || !lowest || !origin) return fail(GSR_E_BADARG, "NULL argument");
  if (!(voxel_size > 0.0 && voxel_size <= DBL_MAX)) return fail(GSR_E_BADARG, "voxel_size must be finite and positive");
  if (!aligned({vertices, lowest}, 3u)) return fail(GSR_E_ALIGN, "vertices / lowest must be 4-byte aligned");
  if (!aligned({origin}, 7u)) return fail(GSR_E_ALIGN, "origin must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t blocks = (V + SIMPLIFY_BLOCK - 1) / SIMPLIFY_BLOCK;
  hipLaunchKernelGGL(simplify_lowest_init_kernel, dim3(1), dim3(WAVE), 0, s, lowest);
  hipLaunchKernelGGL(simplify_lowest_kernel, dim3((unsigned)(blocks < LOWEST_MAX_BLOCKS ? blocks : LOWEST_MAX_BLOCKS)),
                     dim3(SIMPLIFY_BLOCK), 0, s, vertices, vertex_mark, V, lowest);
  hipLaunchKernelGGL(simplify_origin_kernel, dim3(1), dim3(WAVE), 0, s, lowest, voxel_size, origin);
  return check(false, s, "simplify_default_origin");
}
int gsr_simplify_cell_keys(const float* vertices, const uint8_t* vertex_mark, int64_t V, const double* origin,
                           double voxel_size, int64_t* keys, int32_t* status, void* stream) {
  if (!simplify_size_ok(V)) return fail(GSR_E_BADARG, "V must lie in 1..2^31-1");
  if (!vertices || !vertex_mark || !origin || !keys || !status) return fail(GSR_E_BADARG, "NULL argument");
  if (!(voxel_size > 0.0 && voxel_size <= DBL_MAX)) return fail(GSR_E_BADARG, "voxel_size must be finite and positive");
  if (!aligned({vertices, status}, 3u)) return fail(GSR_E_ALIGN, "vertices / status must be 4-byte aligned");
  if (!aligned({origin, keys}, 7u)) return fail(GSR_E_ALIGN, "origin / keys must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(simplify_cell_keys_kernel, simplify_grid(V), dim3(SIMPLIFY_BLOCK), 0, s, vertices, vertex_mark, V,
                     origin, voxel_size, keys, status);
  return check(false, s, "simplify_cell_keys");
}
int gsr_simplify_run_heads(const int64_t* keys_sorted, int64_t V, uint8_t* head, void* stream) {
  if (!simplify_size_ok(V)) return fail(GSR_E_BADARG, "V must lie in 1..2^31-1");
  if (!keys_sorted || !head) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({keys_sorted}, 7u)) return fail(GSR_E_ALIGN, "keys must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(simplify_run_heads_kernel, simplify_grid(V), dim3(SIMPLIFY_BLOCK), 0, s, keys_sorted, V, head);
  return check(false, s, "simplify_run_heads");
}
int gsr_simplify_reduce(const float* vertices, const float* colors, const int64_t* keys_sorted, const int64_t* order,
                        const int64_t* ends, int64_t V, int64_t K, int32_t* start, float* out_vertices, float* out_colors,
                        int32_t* cluster_of_vertex, int32_t* status, void* stream) {
  if (!simplify_size_ok(V) || K < 1 || K > V) return fail(GSR_E_BADARG, "V must lie in 1..2^31-1 and K in 1..V");
  if (!vertices || !keys_sorted || !order || !ends || !start || !out_vertices || !cluster_of_vertex || !status)
    return fail(GSR_E_BADARG, "NULL argument");
  if ((colors != nullptr) != (out_colors != nullptr)) return fail(GSR_E_BADARG, "give colors and out_colors together or neither");
  if (!aligned({vertices, colors, start, out_vertices, out_colors, cluster_of_vertex, status}, 3u))
    return fail(GSR_E_ALIGN, "float and int32 arrays must be 4-byte aligned");
  if (!aligned({keys_sorted, order, ends}, 7u)) return fail(GSR_E_ALIGN, "keys / order / ends must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(simplify_starts_kernel, simplify_grid(V), dim3(SIMPLIFY_BLOCK), 0, s, keys_sorted, order, ends, V, K,
                     start, cluster_of_vertex, status);
  hipLaunchKernelGGL(simplify_reduce_kernel, simplify_grid(K), dim3(SIMPLIFY_BLOCK), 0, s, vertices, colors, order, start,
                     V, K, out_vertices, out_colors, status);
  return check(false, s, "simplify_reduce");
}
int gsr_simplify_face_keys(const int32_t* faces, const int32_t* cluster_of_vertex, int64_t F, int64_t V, int64_t K,
                           int32_t* tri, uint8_t* keep, int64_t* key_first, int32_t* key_third, int32_t* status,
                           void* stream) {
  if (!simplify_size_ok(F) || !simplify_size_ok(V) || K < 1 || K > V)
    return fail(GSR_E_BADARG, "F and V must lie in 1..2^31-1 and K in 1..V");
  if (!faces || !cluster_of_vertex || !tri || !keep || !key_first || !key_third || !status)
    return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({faces, cluster_of_vertex, tri, key_third, status}, 3u))
    return fail(GSR_E_ALIGN, "int32 arrays must be 4-byte aligned");
  if (!aligned({key_first}, 7u)) return fail(GSR_E_ALIGN, "key_first must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(simplify_face_keys_kernel, simplify_grid(F), dim3(SIMPLIFY_BLOCK), 0, s, faces, cluster_of_vertex, F,
                     (uint32_t)V, (uint32_t)K, tri, keep, key_first, key_third, status);
  return check(false, s, "simplify_face_keys");
}
int gsr_simplify_face_unique(const int64_t* first_sorted, const int64_t* perm, const int32_t* key_third, int64_t F,
                             uint8_t* keep, int32_t* status, void* stream) {
  if (!simplify_size_ok(F)) return fail(GSR_E_BADARG, "F must lie in 1..2^31-1");
  if (!first_sorted || !perm || !key_third || !keep || !status) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({key_third, status}, 3u)) return fail(GSR_E_ALIGN, "key_third / status must be 4-byte aligned");
  if (!aligned({first_sorted, perm}, 7u)) return fail(GSR_E_ALIGN, "first_sorted / perm must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (F >= 2)       // one lane per pair of neighbouring slots
    hipLaunchKernelGGL(simplify_face_unique_kernel, simplify_grid(F - 1), dim3(SIMPLIFY_BLOCK), 0, s, first_sorted, perm,
                       key_third, F, keep, status);
  return check(false, s, "simplify_face_unique");
}
int gsr_simplify_vertex_map(const int32_t* cluster_of_vertex, const uint8_t* cluster_mark, const int64_t* cluster_offs,
                            int64_t V, int64_t K, int32_t* vertex_cluster, void* stream) {
  if (!simplify_size_ok(V) || K < 1 || K > V) return fail(GSR_E_BADARG, "V must lie in 1..2^31-1 and K in 1..V");
  if (!cluster_of_vertex || !cluster_mark || !cluster_offs || !vertex_cluster) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({cluster_of_vertex, vertex_cluster}, 3u)) return fail(GSR_E_ALIGN, "int32 arrays must be 4-byte aligned");
  if (!aligned({cluster_offs}, 7u)) return fail(GSR_E_ALIGN, "cluster_offs must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(simplify_vertex_map_kernel, simplify_grid(V), dim3(SIMPLIFY_BLOCK), 0, s, cluster_of_vertex,
                     cluster_mark, cluster_offs, V, (uint32_t)K, vertex_cluster);
  return check(false, s, "simplify_vertex_map");
}

}  // extern "C"

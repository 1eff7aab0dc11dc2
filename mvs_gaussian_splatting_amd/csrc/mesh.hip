// Mesh cleaning on an indexed triangle mesh: connected components of the faces, their sizes, and the compaction that
// keeps a subset of the faces and the vertices they refer to (include/gsr.h, ABI v31; mesh.py).
//
// Launch shape of every kernel here: 256-lane workgroups, one lane per node / face / key / vertex, a one-dimensional
// grid of ceil(n / 256) workgroups, no grid-stride loop and no persistence.  No LDS.  Nothing waits on another lane,
// wave or workgroup: the only loops are the two of the union-find below, and each of their steps strictly lowers an
// index.
//
// Labelling: a lock-free union-find over n nodes, int32 parent[n].
//   * mesh_init_kernel      parent[i] = i (and, for the vertex connectivity, first[i] = INT32_MAX).
//   * mesh_hook_*_kernel    for each pair (a, b): find both roots, link the larger root under the smaller with a 32-bit
//                           atomicMin on parent[larger]; if the atomic returns something other than `larger`, that node
//                           had a parent already: go on with the pair (value returned, smaller).
//   * mesh_flatten_kernel   a launch of its own behind the hooks: parent[i] = root of i.
// Invariant: parent[x] <= x at every instant (init writes x; the only other writer in the hooks is atomicMin(parent[hi],
// lo) with lo < hi; flatten writes a root, which a chain of such links reaches, so it is <= x too).
// Connectivity: the links (x, parent[x]) together with the pairs that lanes still hold connect exactly what the pairs
// seen so far connect.  An atomicMin that finds old != hi replaces the link (hi, old) by (hi, min(old, lo)); the lane
// goes on holding (old, lo), so nothing that was connected comes apart, and only nodes of one component are ever linked.
// Components therefore only grow, and a value that parent[x] held at any earlier time -- all a stale load can return --
// is still a node of x's component with an index <= x: a stale read costs iterations, never correctness.  The loads of
// parent in the hooks are relaxed agent-scope atomic loads all the same (a plain load may be served from this CU's L1,
// which no other CU's atomic refreshes, or be kept in a register), and parent is never passed const __restrict__.
// Result: when the hooks have drained, every component is one tree whose links all point to smaller indices, so its
// root is its smallest node whatever order the atomics landed in, and after flatten parent[] holds the same bits from
// run to run.
//
// Two ways to form the pairs.  Vertex connectivity: nodes are vertices, face (v0, v1, v2) gives (v0, v1) and (v0, v2)
// straight from `faces`.  Edge connectivity: nodes are faces; mesh_edge_keys_kernel writes for each of the 3 F directed
// edges (a, b) of the faces the key (min(a, b) << 32) | max(a, b) and the owning face, the caller sorts the keys, and
// mesh_hook_runs_kernel unions the owners of equal neighbouring keys (so an edge of three or more faces joins all of
// them, and a degenerate face's repeated edge joins the face to itself: nothing).
//
// Numbering: face f is marked when it is the smallest face of its component.  Edge connectivity: parent[f] == f.
// Vertex connectivity: one atomicMin of the face index into first[root of v0] (one per wave and root: the lanes of a wave
// that share a root are served by the lowest, whose face index is the smallest), then first[root of v0] == f.  The
// caller scans the marks; mesh_label_kernel writes face_component[f] = scan[smallest face of f's component] and counts
// the faces per component with integer atomics (one per wave and component), exact and order-free.
//
// Compaction: mesh_mark_vertices_kernel stores 1 at every vertex a kept face refers to; the caller scans the vertex
// marks and the keep flags; mesh_compact_kernel copies the kept vertex / colour rows and writes the kept faces
// re-indexed, both in their original order, at slots the scans fix.
//
// A face index outside 0..V-1 is never used as an index: the face is skipped and *status is set to 1.
#include "gsr_common.h"
#include "gsr_entry.h"

namespace gsr {

namespace {

constexpr int MESH_BLOCK = 256;

__device__ __forceinline__ int32_t load_parent(int32_t* parent, int32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x, or a node of x's component that was its root at some earlier time.
__device__ __forceinline__ int32_t find_root(int32_t* parent, int32_t x, unsigned& steps) {
  // Terminates: a step replaces x by a value p with 0 <= p < x (anything else ends the loop), so at most x steps.  It
  // waits for nobody: a stale p is an earlier parent of x, which is smaller than x as well.
  for (;;) {
    const int32_t p = load_parent(parent, x);
    if ((uint32_t)p >= (uint32_t)x) return x;   // p == x: a root.  p > x or p < 0 (a parent[] that init did not write): stop
    x = p;
    ++steps;
  }
}

__device__ __forceinline__ void unite(int32_t* parent, int32_t a, int32_t b, unsigned& steps, unsigned& retries) {
  // Terminates: a retry goes on with (old, lo), both smaller than hi, and the finds only lower them further, so the
  // larger root of the pair strictly falls from one iteration to the next; it is bounded below by 0.  No iteration
  // waits for another lane's store: whatever the atomic returns, this lane either is done or holds a smaller pair.
  for (;;) {
    a = find_root(parent, a, steps);
    b = find_root(parent, b, steps);
    if (a == b) return;
    const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
    const int32_t old = atomicMin(parent + hi, lo);
    // old == hi: hi was a root at the instant of the atomic and hangs under lo now.  (old > hi or old < 0 cannot happen
    // behind init; the same test ends the loop then instead of following a value that is no node.)
    if ((uint32_t)old >= (uint32_t)hi) return;
    // hi had the parent old < hi already, and has min(old, lo) now: (old, lo) is still to be joined
    a = old;
    b = lo;
    ++retries;
  }
}

__device__ __forceinline__ void add_stats(unsigned long long* stats, unsigned steps, unsigned retries) {
  if (!stats) return;
  if (steps) atomicAdd(stats, (unsigned long long)steps);
  if (retries) atomicAdd(stats + 1, (unsigned long long)retries);
}

__device__ __forceinline__ bool face_ok(const int32_t* faces, int64_t f, uint32_t V, int32_t v[3]) {
  v[0] = faces[3 * f];
  v[1] = faces[3 * f + 1];
  v[2] = faces[3 * f + 2];
  return (uint32_t)v[0] < V && (uint32_t)v[1] < V && (uint32_t)v[2] < V;
}

__global__ void __launch_bounds__(MESH_BLOCK) mesh_init_kernel(int64_t n, int32_t* parent, int32_t* first) {
  const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (i >= n) return;
  parent[i] = (int32_t)i;
  if (first) first[i] = INT32_MAX;
}

__global__ void __launch_bounds__(MESH_BLOCK) mesh_hook_faces_kernel(const int32_t* faces, int64_t F, uint32_t V,
                                                                     int32_t* parent, int32_t* status,
                                                                     unsigned long long* stats) {
  const int64_t f = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (f >= F) return;
  int32_t v[3];
  if (!face_ok(faces, f, V, v)) {
    *status = 1;
    return;
  }
  unsigned steps = 0, retries = 0;
  unite(parent, v[0], v[1], steps, retries);
  unite(parent, v[0], v[2], steps, retries);
  add_stats(stats, steps, retries);
}

__global__ void __launch_bounds__(MESH_BLOCK) mesh_edge_keys_kernel(const int32_t* faces, int64_t F, uint32_t V,
                                                                    int64_t* keys, int32_t* owner, int32_t* status) {
  const int64_t f = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (f >= F) return;
  int32_t v[3];
  const bool ok = face_ok(faces, f, V, v);
  if (!ok) *status = 1;
  for (int e = 0; e < 3; ++e) {
    const int32_t a = v[e], b = v[e == 2 ? 0 : e + 1];
    const int64_t lo = a < b ? a : b, hi = a < b ? b : a;
    // a refused face gets three keys of its own (negative, so no edge's): it joins nothing
    keys[3 * f + e] = ok ? (int64_t)(((uint64_t)lo << 32) | (uint64_t)hi) : -(3 * f + e) - 1;
    owner[3 * f + e] = (int32_t)f;
  }
}

__global__ void __launch_bounds__(MESH_BLOCK) mesh_hook_runs_kernel(const int64_t* keys, const int64_t* order,
                                                                    const int32_t* owner, int64_t m, uint32_t n,
                                                                    int32_t* parent, int32_t* status,
                                                                    unsigned long long* stats) {
  const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x + 1;
  if (i >= m) return;
  if (keys[i] != keys[i - 1]) return;
  const int64_t oa = order[i - 1], ob = order[i];
  if ((uint64_t)oa >= (uint64_t)m || (uint64_t)ob >= (uint64_t)m) {
    *status = 1;
    return;
  }
  const int32_t a = owner[oa], b = owner[ob];
  if ((uint32_t)a >= n || (uint32_t)b >= n) {
    *status = 1;
    return;
  }
  unsigned steps = 0, retries = 0;
  unite(parent, a, b, steps, retries);
  add_stats(stats, steps, retries);
}

__global__ void __launch_bounds__(MESH_BLOCK) mesh_flatten_kernel(int64_t n, int32_t* parent) {
  const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (i >= n) return;
  unsigned steps = 0;
  // other lanes of this launch store roots too: a node read here holds its old parent or its root, both on the way to
  // the same root
  const int32_t r = find_root(parent, (int32_t)i, steps);
  __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One operation per group of lanes of a wave that hold the same key, issued by the group's lowest lane.  Every lane of
// the wave must call it (those with nothing to add with live = false); true for the issuing lanes, whose *group is the
// mask of the lanes they issue for.
__device__ __forceinline__ bool wave_group(bool live, int32_t key, int lane, unsigned long long* group) {
  bool lead = false;
  for (;;) {                                           // at most 64 rounds: every round retires its leader's group
    const unsigned long long pending = __ballot(live);
    if (!pending) break;
    const int leader = __ffsll((long long)pending) - 1;
    const int32_t k = __shfl(key, leader);
    const bool mine = live && key == k;
    const unsigned long long same = __ballot(mine);
    if (mine) {
      lead = lane == leader;
      *group = same;
      live = false;
    }
  }
  return lead;
}

__global__ void __launch_bounds__(MESH_BLOCK) mesh_face_min_kernel(const int32_t* faces, int64_t F, uint32_t V,
                                                                   const int32_t* parent, int32_t* first) {
  const int64_t f = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  int32_t v[3], r = -1;
  bool live = f < F && face_ok(faces, f, V, v);
  if (live) {
    r = parent[v[0]];
    live = (uint32_t)r < V;
  }
  unsigned long long group = 0;
  // lanes ascend with f: the group's lowest lane holds its smallest face
  if (wave_group(live, r, threadIdx.x & 63, &group)) atomicMin(first + r, (int32_t)f);
}

template <bool VERTEX>
__global__ void __launch_bounds__(MESH_BLOCK) mesh_mark_kernel(const int32_t* faces, int64_t F, uint32_t V,
                                                               const int32_t* parent, const int32_t* first,
                                                               int32_t* face_root, uint8_t* mark) {
  const int64_t f = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (f >= F) return;
  if (!VERTEX) {
    mark[f] = parent[f] == (int32_t)f;
    return;
  }
  int32_t v[3], root = (int32_t)f;                     // a refused face stands alone
  if (face_ok(faces, f, V, v)) {
    const int32_t r = parent[v[0]];
    if ((uint32_t)r < V) root = first[r];
  }
  face_root[f] = root;
  mark[f] = root == (int32_t)f;
}

__global__ void __launch_bounds__(MESH_BLOCK) mesh_label_kernel(const int32_t* face_root, const int64_t* ids, int64_t F,
                                                                int64_t K, int32_t* face_component,
                                                                unsigned long long* component_faces) {
  const int64_t f = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  bool live = f < F;
  int32_t c = -1;
  if (live) {
    const int32_t r = face_root[f];
    live = (uint32_t)r < (uint64_t)F;
    if (live) {
      const int64_t id = ids[r];
      live = id >= 0 && id < K;
      c = (int32_t)id;
    }
    if (live) face_component[f] = c;
  }
  unsigned long long group = 0;
  if (wave_group(live, c, threadIdx.x & 63, &group)) atomicAdd(component_faces + c, (unsigned long long)__popcll(group));
}

__global__ void __launch_bounds__(MESH_BLOCK) mesh_mark_vertices_kernel(const int32_t* faces, const uint8_t* keep,
                                                                        int64_t F, uint32_t V, uint8_t* vertex_mark,
                                                                        int32_t* status) {
  const int64_t f = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (f >= F || !keep[f]) return;
  int32_t v[3];
  if (!face_ok(faces, f, V, v)) {
    *status = 1;
    return;
  }
  vertex_mark[v[0]] = 1;
  vertex_mark[v[1]] = 1;
  vertex_mark[v[2]] = 1;
}

__global__ void __launch_bounds__(MESH_BLOCK) mesh_compact_kernel(const float* vertices, const float* colors,
                                                                  const int32_t* faces, const uint8_t* keep,
                                                                  const uint8_t* vertex_mark, const int64_t* vert_offs,
                                                                  const int64_t* face_offs, int64_t V, int64_t F,
                                                                  int64_t Vk, int64_t Fk, float* out_vertices,
                                                                  float* out_colors, int32_t* out_faces,
                                                                  int32_t* status) {
  const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (i < V && vertex_mark[i]) {
    const int64_t o = vert_offs[i];
    if (o >= 0 && o < Vk) {
      for (int a = 0; a < 3; ++a) out_vertices[3 * o + a] = vertices[3 * i + a];
      if (colors)
        for (int a = 0; a < 3; ++a) out_colors[3 * o + a] = colors[3 * i + a];
    }
  }
  if (i < F && keep[i]) {
    const int64_t o = face_offs[i];
    int32_t v[3];
    if (!face_ok(faces, i, (uint32_t)V, v)) {
      *status = 1;
      return;
    }
    if (o >= 0 && o < Fk)
      for (int a = 0; a < 3; ++a) out_faces[3 * o + a] = (int32_t)vert_offs[v[a]];
  }
}

inline dim3 mesh_grid(int64_t n) { return dim3((unsigned)((n + MESH_BLOCK - 1) / MESH_BLOCK)); }
inline bool mesh_size_ok(int64_t n) { return n >= 1 && n <= (int64_t)INT32_MAX; }

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h): every size is checked to lie in 1 .. 2^31 - 1, every pointer for NULL and alignment
using namespace gsr;

extern "C" {

int gsr_mesh_cc_init(int64_t n, int32_t* parent, int32_t* first, void* stream) {
  if (!mesh_size_ok(n)) return fail(GSR_E_BADARG, "n must lie in 1..2^31-1");
  if (!parent) return fail(GSR_E_BADARG, "parent is NULL");
  if (!aligned({parent, first}, 3u)) return fail(GSR_E_ALIGN, "parent / first must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mesh_init_kernel, mesh_grid(n), dim3(MESH_BLOCK), 0, s, n, parent, first);
  return check(false, s, "mesh_cc_init");
}
int gsr_mesh_cc_hook_faces(const int32_t* faces, int64_t F, int64_t V, int32_t* parent, int32_t* status, uint64_t* stats,
                           void* stream) {
  if (!mesh_size_ok(F) || !mesh_size_ok(V)) return fail(GSR_E_BADARG, "F and V must lie in 1..2^31-1");
  if (!faces || !parent || !status) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({faces, parent, status}, 3u)) return fail(GSR_E_ALIGN, "faces / parent / status must be 4-byte aligned");
  if (!aligned({stats}, 7u)) return fail(GSR_E_ALIGN, "stats must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mesh_hook_faces_kernel, mesh_grid(F), dim3(MESH_BLOCK), 0, s, faces, F, (uint32_t)V, parent, status,
                     reinterpret_cast<unsigned long long*>(stats));
  return check(false, s, "mesh_cc_hook_faces");
}
int gsr_mesh_edge_keys(const int32_t* faces, int64_t F, int64_t V, int64_t* keys, int32_t* owner, int32_t* status,
                       void* stream) {
  if (!mesh_size_ok(F) || !mesh_size_ok(V)) return fail(GSR_E_BADARG, "F and V must lie in 1..2^31-1");
  if (!faces || !keys || !owner || !status) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({faces, owner, status}, 3u)) return fail(GSR_E_ALIGN, "faces / owner / status must be 4-byte aligned");
  if (!aligned({keys}, 7u)) return fail(GSR_E_ALIGN, "keys must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mesh_edge_keys_kernel, mesh_grid(F), dim3(MESH_BLOCK), 0, s, faces, F, (uint32_t)V, keys, owner,
                     status);
  return check(false, s, "mesh_edge_keys");
}
int gsr_mesh_cc_hook_runs(const int64_t* keys_sorted, const int64_t* order, const int32_t* owner, int64_t m, int64_t n,
                          int32_t* parent, int32_t* status, uint64_t* stats, void* stream) {
  if (m < 1 || m > 3 * (int64_t)INT32_MAX || !mesh_size_ok(n))
    return fail(GSR_E_BADARG, "n must lie in 1..2^31-1 and m in 1..3 (2^31-1)");
  if (!keys_sorted || !order || !owner || !parent || !status) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({owner, parent, status}, 3u)) return fail(GSR_E_ALIGN, "owner / parent / status must be 4-byte aligned");
  if (!aligned({keys_sorted, order, stats}, 7u)) return fail(GSR_E_ALIGN, "keys / order / stats must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (m >= 2)       // one lane per pair of neighbouring keys
    hipLaunchKernelGGL(mesh_hook_runs_kernel, mesh_grid(m - 1), dim3(MESH_BLOCK), 0, s, keys_sorted, order, owner, m,
                       (uint32_t)n, parent, status, reinterpret_cast<unsigned long long*>(stats));
  return check(false, s, "mesh_cc_hook_runs");
}
int gsr_mesh_cc_flatten(int64_t n, int32_t* parent, void* stream) {
  if (!mesh_size_ok(n)) return fail(GSR_E_BADARG, "n must lie in 1..2^31-1");
  if (!parent) return fail(GSR_E_BADARG, "parent is NULL");
  if (!aligned({parent}, 3u)) return fail(GSR_E_ALIGN, "parent must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mesh_flatten_kernel, mesh_grid(n), dim3(MESH_BLOCK), 0, s, n, parent);
  return check(false, s, "mesh_cc_flatten");
}
int gsr_mesh_cc_mark(const int32_t* faces, int64_t F, int64_t V, const int32_t* parent, int32_t* first,
                     int32_t* face_root, uint8_t* mark, void* stream) {
  if (!mesh_size_ok(F)) return fail(GSR_E_BADARG, "F must lie in 1..2^31-1");
  if (!parent || !mark) return fail(GSR_E_BADARG, "NULL argument");
  const int given = (faces != nullptr) + (first != nullptr) + (face_root != nullptr);
  if (given != 0 && given != 3) return fail(GSR_E_BADARG, "give faces, first and face_root together (vertex nodes) or none");
  if (given == 3 && !mesh_size_ok(V)) return fail(GSR_E_BADARG, "V must lie in 1..2^31-1");
  if (!aligned({faces, parent, first, face_root}, 3u)) return fail(GSR_E_ALIGN, "int32 arrays must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (faces) {
    hipLaunchKernelGGL(mesh_face_min_kernel, mesh_grid(F), dim3(MESH_BLOCK), 0, s, faces, F, (uint32_t)V, parent, first);
    hipLaunchKernelGGL(mesh_mark_kernel<true>, mesh_grid(F), dim3(MESH_BLOCK), 0, s, faces, F, (uint32_t)V, parent, first,
                       face_root, mark);
  } else {
    hipLaunchKernelGGL(mesh_mark_kernel<false>, mesh_grid(F), dim3(MESH_BLOCK), 0, s, faces, F, 0u, parent, first,
                       face_root, mark);
  }
  return check(false, s, "mesh_cc_mark");
}
int gsr_mesh_cc_label(const int32_t* face_root, const int64_t* ids, int64_t F, int64_t K, int32_t* face_component,
                      int64_t* component_faces, void* stream) {
  if (!mesh_size_ok(F) || K < 1 || K > F) return fail(GSR_E_BADARG, "F must lie in 1..2^31-1 and K in 1..F");
  if (!face_root || !ids || !face_component || !component_faces) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({face_root, face_component}, 3u)) return fail(GSR_E_ALIGN, "int32 arrays must be 4-byte aligned");
  if (!aligned({ids, component_faces}, 7u)) return fail(GSR_E_ALIGN, "int64 arrays must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mesh_label_kernel, mesh_grid(F), dim3(MESH_BLOCK), 0, s, face_root, ids, F, K, face_component,
                     reinterpret_cast<unsigned long long*>(component_faces));
  return check(false, s, "mesh_cc_label");
}
int gsr_mesh_mark_vertices(const int32_t* faces, const uint8_t* keep, int64_t F, int64_t V, uint8_t* vertex_mark,
                           int32_t* status, void* stream) {
  if (!mesh_size_ok(F) || !mesh_size_ok(V)) return fail(GSR_E_BADARG, "F and V must lie in 1..2^31-1");
  if (!faces || !keep || !vertex_mark || !status) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({faces, status}, 3u)) return fail(GSR_E_ALIGN, "faces / status must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mesh_mark_vertices_kernel, mesh_grid(F), dim3(MESH_BLOCK), 0, s, faces, keep, F, (uint32_t)V,
                     vertex_mark, status);
  return check(false, s, "mesh_mark_vertices");
}
int gsr_mesh_compact(const float* vertices, const float* colors, const int32_t* faces, const uint8_t* keep,
                     const uint8_t* vertex_mark, const int64_t* vert_offs, const int64_t* face_offs, int64_t V, int64_t F,
                     int64_t Vk, int64_t Fk, float* out_vertices, float* out_colors, int32_t* out_faces, int32_t* status,
                     void* stream) {
  if (!mesh_size_ok(F) || !mesh_size_ok(V)) return fail(GSR_E_BADARG, "F and V must lie in 1..2^31-1");
  if (Vk < 1 || Vk > V || Fk < 1 || Fk > F) return fail(GSR_E_BADARG, "Vk must lie in 1..V and Fk in 1..F");
  if (!vertices || !faces || !keep || !vertex_mark || !vert_offs || !face_offs || !out_vertices || !out_faces || !status)
    return fail(GSR_E_BADARG, "NULL argument");
  if ((colors != nullptr) != (out_colors != nullptr)) return fail(GSR_E_BADARG, "give colors and out_colors together or neither");
  if (!aligned({vertices, colors, faces, out_vertices, out_colors, out_faces, status}, 3u))
    return fail(GSR_E_ALIGN, "float and int32 arrays must be 4-byte aligned");
  if (!aligned({vert_offs, face_offs}, 7u)) return fail(GSR_E_ALIGN, "offsets must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mesh_compact_kernel, mesh_grid(V > F ? V : F), dim3(MESH_BLOCK), 0, s, vertices, colors, faces, keep,
                     vertex_mark, vert_offs, face_offs, V, F, Vk, Fk, out_vertices, out_colors, out_faces, status);
  return check(false, s, "mesh_compact");
}

}  // extern "C"

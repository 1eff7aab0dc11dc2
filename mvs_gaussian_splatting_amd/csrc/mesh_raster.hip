// Rasterizing an indexed triangle mesh from a camera (include/gsr.h, ABI v42; mesh.rasterize_mesh, mesh.face_view_counts,
// mesh.cull_invisible_faces): a z-buffer of 64-bit keys, depth bits above the face index, kept by integer
// atomicMin -- the nearest surface wins, the smallest face index at equal depth, whatever order the faces arrive in.  The
// rule of a (face, view) pair is csrc/mesh_raster_math.h, one body for device and host (the unit is built with
// -ffp-contract=off).
//
// raster_project_kernel (optional): one lane per vertex, world -> view space into a scratch [V,3]; the faces kernel then
//     gathers view-space corners and skips its own transform.  Which of the two is faster is a measurement
//     (tools/bench_mesh_raster.py; profiles/mesh_raster/NOTES.md); the default is the transform per face.
// raster_faces_kernel: one lane per face, 256-lane workgroups, no LDS, nothing waits on another workgroup.  An extracted
//     mesh is almost all sub-pixel to few-pixel triangles: a piece whose clipped bounding box holds at most
//     GSR_RASTER_LANE_PIXELS pixels is walked by its lane; a larger one is appended to a device queue as face << 1 | piece,
//     one atomicAdd per wave (ballot, popcount, the leader adds, the base is broadcast).
// raster_drain_kernel: a fixed grid of GSR_RASTER_DRAIN_WAVES waves strides over the queue -- its length is read on the
//     device, no read-back sizes anything.  Each wave takes one piece, sets it up again from the face (the same bits) and
//     its 64 lanes stride over the box.
// Per covered centre: a plain load skips the atomic when the stored key is already smaller -- the buffer only decreases,
//     so a stale read costs a redundant atomic and nothing else -- then one atomicMin on the uint64.
// raster_resolve_kernel: keys -> depth float32 (0: no surface), face_id int32 (-1: none).
// raster_count_kernel: one lane per pixel; the first pixel of every run of one face along a row exchanges the face's stamp
//     with this view's and adds 1 to counts[face] when the old stamp differed.  Integer atomics only.
//
// Safety: a face index outside 0 .. V-1 is counted and never used; pixel indices come from a box clipped to the image;
// a queue slot beyond the capacity is not written and not read; a face id read from the key buffer is used as an index
// only below F.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "mesh_raster_math.h"

namespace gsr {

namespace {

constexpr int RASTER_BLOCK = 256;
constexpr int RASTER_DRAIN_BLOCKS = GSR_RASTER_DRAIN_WAVES / (RASTER_BLOCK / WAVE);
constexpr int HEAD_QUEUED = 0, HEAD_DROPPED = 1, HEAD_BAD_FACES = 2;       // words of the queue's 256-byte head
constexpr size_t HEAD_BYTES = 256;
constexpr uint64_t KEY_NONE = ~(uint64_t)0;

struct RasterArgs {
  const float* vertices;      // world space, or view space when view_space != 0
  const int32_t* faces;
  uint64_t* keys;
  uint32_t* head;
  uint32_t* queue;
  uint32_t V, F, capacity;
  float near;
  int view_space, cull_backfaces, load_skip;
};

__device__ inline void plot(uint64_t* keys, size_t pix, uint64_t key, int load_skip) {
  if (load_skip && keys[pix] <= key) return;
  atomicMin(reinterpret_cast<unsigned long long*>(keys + pix), (unsigned long long)key);
}

// steps 1 and 2 of face f -> the number n of clipped corners (0, 3 or 4) in c0 .. c3: the pieces are (c0, c1, c2) and, when
// n = 4, (c0, c2, c3).  The corners stay in named registers; only a face that crosses the near plane goes through
// raster_clip's array.
__device__ inline int face_corners(const RasterArgs& a, const GsrCullView& view, uint32_t f, bool count_bad, RasterVert& c0,
                                   RasterVert& c1, RasterVert& c2, RasterVert& c3) {
  const int32_t* __restrict__ row = a.faces + 3 * (size_t)f;
  const uint32_t ia = (uint32_t)row[0], ib = (uint32_t)row[1], ic = (uint32_t)row[2];     // a negative index is large
  if (ia >= a.V || ib >= a.V || ic >= a.V) {
    if (count_bad) atomicAdd(a.head + HEAD_BAD_FACES, 1u);
    return 0;
  }
  const float* __restrict__ pa = a.vertices + 3 * (size_t)ia;
  const float* __restrict__ pb = a.vertices + 3 * (size_t)ib;
  const float* __restrict__ pc = a.vertices + 3 * (size_t)ic;
  RasterVert v[3];
  if (a.view_space) {
    v[0] = {pa[0], pa[1], pa[2]};
    v[1] = {pb[0], pb[1], pb[2]};
    v[2] = {pc[0], pc[1], pc[2]};
  } else {
    cull_transform(view.world_to_view, pa[0], pa[1], pa[2], v[0].x, v[0].y, v[0].z);
    cull_transform(view.world_to_view, pb[0], pb[1], pb[2], v[1].x, v[1].y, v[1].z);
    cull_transform(view.world_to_view, pc[0], pc[1], pc[2], v[2].x, v[2].y, v[2].z);
  }
  if (v[0].z > a.near && v[1].z > a.near && v[2].z > a.near) {       // raster_clip's first case, without its copy
    c0 = v[0];
    c1 = v[1];
    c2 = v[2];
    return 3;
  }
  RasterVert o[4];
  const int n = raster_clip(v, a.near, o);
  if (n >= 3) {
    c0 = o[0];
    c1 = o[1];
    c2 = o[2];
  }
  if (n == 4) c3 = o[3];
  return n;
}

__global__ __launch_bounds__(RASTER_BLOCK) void raster_project_kernel(const float* __restrict__ vertices, uint32_t V,
                                                                      GsrCullView view, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * RASTER_BLOCK + threadIdx.x;
  if (i >= V) return;
  const float* __restrict__ p = vertices + 3 * (size_t)i;
  float x, y, z;
  cull_transform(view.world_to_view, p[0], p[1], p[2], x, y, z);
  out[3 * (size_t)i] = x;
  out[3 * (size_t)i + 1] = y;
  out[3 * (size_t)i + 2] = z;
}

__global__ __launch_bounds__(RASTER_BLOCK) void raster_faces_kernel(RasterArgs a, GsrCullView view) {
  const uint32_t f = blockIdx.x * RASTER_BLOCK + threadIdx.x;
  const bool live = f < a.F;                     // no early return: every lane takes part in the ballots below
  const int lane = lane_id();
  RasterVert c0, c1, c2, c3;
  const int n = live ? face_corners(a, view, f, true, c0, c1, c2, c3) : 0;
  for (int k = 0; k < 2; ++k) {
    bool queued = false;
    if (n >= 3 + k) {
      RasterPiece p;
      const int r = raster_setup(view, c0, k == 0 ? c1 : c2, k == 0 ? c2 : c3, a.cull_backfaces != 0, p);
      if (r == RASTER_PIECE_DROPPED) atomicAdd(a.head + HEAD_DROPPED, 1u);
      if (r == RASTER_PIECE_OK && p.x0 <= p.x1 && p.y0 <= p.y1) {
        const int bw = p.x1 - p.x0 + 1, bh = p.y1 - p.y0 + 1;
        if ((int64_t)bw * bh > GSR_RASTER_LANE_PIXELS) {
          queued = true;
        } else {
          for (int iy = p.y0; iy <= p.y1; ++iy)
            for (int ix = p.x0; ix <= p.x1; ++ix) {
              float z;
              if (raster_cover(p, ix, iy, z))
                plot(a.keys, (size_t)iy * (size_t)view.width + (size_t)ix, raster_key(z, f), a.load_skip);
            }
        }
      }
    }
    const unsigned long long want = __ballot(queued);
    if (want != 0ull) {
      const int leader = __ffsll((long long)want) - 1;
      uint32_t base = 0;
      if (lane == leader) base = atomicAdd(a.head + HEAD_QUEUED, (uint32_t)__popcll(want));
      base = (uint32_t)__shfl((int)base, leader, WAVE);
      if (queued) {
        const uint32_t slot = base + (uint32_t)__popcll(want & ((1ull << lane) - 1ull));
        if (slot < a.capacity) a.queue[slot] = f << 1 | (uint32_t)k;
      }
    }
  }
}

__global__ __launch_bounds__(RASTER_BLOCK) void raster_drain_kernel(RasterArgs a, GsrCullView view) {
  const uint32_t queued = a.head[HEAD_QUEUED];
  const uint32_t count = queued < a.capacity ? queued : a.capacity;
  const uint32_t wave = blockIdx.x * (RASTER_BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = lane_id();
  for (uint32_t e = wave; e < count; e += GSR_RASTER_DRAIN_WAVES) {
    const uint32_t entry = a.queue[e];
    const uint32_t f = entry >> 1;
    const int k = (int)(entry & 1u);
    RasterVert c0, c1, c2, c3;
    RasterPiece p;
    if (f >= a.F || face_corners(a, view, f, false, c0, c1, c2, c3) < 3 + k) continue;
    if (raster_setup(view, c0, k == 0 ? c1 : c2, k == 0 ? c2 : c3, a.cull_backfaces != 0, p) != RASTER_PIECE_OK) continue;
    const int bw = p.x1 - p.x0 + 1, bh = p.y1 - p.y0 + 1;
    if (bw <= 0 || bh <= 0) continue;
    const int n = bw * bh;                                                 // at most H W <= 2^28
    for (int i = lane; i < n; i += WAVE) {
      const int dy = i / bw, ix = p.x0 + (i - dy * bw), iy = p.y0 + dy;
      float z;
      if (raster_cover(p, ix, iy, z))
        plot(a.keys, (size_t)iy * (size_t)view.width + (size_t)ix, raster_key(z, f), a.load_skip);
    }
  }
}

__global__ __launch_bounds__(RASTER_BLOCK) void raster_resolve_kernel(const uint64_t* __restrict__ keys, int npix,
                                                                      float* __restrict__ depth,
                                                                      int32_t* __restrict__ face_id) {
  const int i = (int)(blockIdx.x * RASTER_BLOCK + threadIdx.x);            // H W <= 2^28
  if (i >= npix) return;
  const uint64_t key = keys[i];
  const bool none = key == KEY_NONE;
  depth[i] = none ? 0.0f : __uint_as_float((uint32_t)(key >> 32));
  face_id[i] = none ? -1 : (int32_t)(uint32_t)key;
}

__global__ __launch_bounds__(RASTER_BLOCK) void raster_count_kernel(const uint64_t* __restrict__ keys, int npix, int W,
                                                                    uint32_t F, int32_t stamp_value, int32_t* stamp,
                                                                    int32_t* counts) {
  const int i = (int)(blockIdx.x * RASTER_BLOCK + threadIdx.x);
  if (i >= npix) return;
  const uint64_t key = keys[i];
  if (key == KEY_NONE) return;
  const uint32_t f = (uint32_t)key;
  if (f >= F) return;
  if (i % W != 0) {                                                        // not the first pixel of its row
    const uint64_t left = keys[i - 1];
    if (left != KEY_NONE && (uint32_t)left == f) return;                   // the run's first pixel speaks for it
  }
  if (atomicExch(stamp + f, stamp_value) != stamp_value) atomicAdd(counts + f, 1);
}

inline dim3 raster_grid(int64_t n) { return dim3((unsigned)((n + RASTER_BLOCK - 1) / RASTER_BLOCK)); }
inline bool finite(float v) { return v - v == 0.0f; }                      // false for NaN and +-inf
inline bool raster_shape_ok(int32_t H, int32_t W) {
  return H > 0 && W > 0 && H <= GSR_RASTER_MAX_SIDE && W <= GSR_RASTER_MAX_SIDE && image_shape_ok(H, W);
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_raster_queue_bytes(int64_t F) {
  if (F < 0 || F > (int64_t)INT32_MAX) return 0;
  return HEAD_BYTES + align_up(8 * (size_t)F, 256);
}

int gsr_raster_view(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const GsrCullView* view,
                    float near_plane, int32_t flags, uint64_t* keys, void* queue, size_t queue_bytes, float* view_scratch,
                    void* stream) {
  if (V < 0 || V > (int64_t)INT32_MAX || F < 0 || F > (int64_t)INT32_MAX)
    return fail(GSR_E_BADARG, "V and F must lie in 0..2^31-1");
  if (!view) return fail(GSR_E_BADARG, "the view is NULL");
  if (!raster_shape_ok(view->height, view->width))
    return fail(GSR_E_BADARG, "width and height must lie in 1..2^14 with at most 2^28 pixels");
  if (!(near_plane > 0.0f) || !finite(near_plane)) return fail(GSR_E_BADARG, "near must be positive and finite");
  if (flags & ~(GSR_RASTER_CLEAR | GSR_RASTER_CULL_BACKFACES | GSR_RASTER_NO_LOAD_SKIP))
    return fail(GSR_E_BADARG, "unknown flags");
  if (!keys || !queue) return fail(GSR_E_BADARG, "keys / queue is NULL");
  if ((V > 0 && !vertices) || (F > 0 && !faces)) return fail(GSR_E_BADARG, "vertices / faces is NULL");
  if (!aligned({vertices, faces, view_scratch}, 3u)) return fail(GSR_E_ALIGN, "vertices, faces and view_scratch must be 4-byte aligned");
  if (!aligned({keys, queue}, 7u)) return fail(GSR_E_ALIGN, "keys and queue must be 8-byte aligned");
  if (queue_bytes < gsr_raster_queue_bytes(F)) return fail(GSR_E_CAPACITY, "queue is smaller than gsr_raster_queue_bytes(F)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t npix = (size_t)view->height * (size_t)view->width;
  if (flags & GSR_RASTER_CLEAR) {
    GSR_HIP(hipMemsetAsync(keys, 0xff, 8 * npix, s));
    GSR_HIP(hipMemsetAsync(queue, 0, HEAD_BYTES, s));                      // the queue's length, dropped, bad faces
  } else {
    GSR_HIP(hipMemsetAsync(queue, 0, sizeof(int32_t), s));                 // the queue's length alone
  }
  if (F == 0) return 0;
  RasterArgs a;
  a.vertices = vertices;
  a.faces = faces;
  a.keys = keys;
  a.head = static_cast<uint32_t*>(queue);
  a.queue = reinterpret_cast<uint32_t*>(static_cast<char*>(queue) + HEAD_BYTES);
  a.V = (uint32_t)V;
  a.F = (uint32_t)F;
  a.capacity = (uint32_t)(2 * F);
  a.near = near_plane;
  a.view_space = 0;
  a.cull_backfaces = (flags & GSR_RASTER_CULL_BACKFACES) != 0;
  a.load_skip = (flags & GSR_RASTER_NO_LOAD_SKIP) == 0;
  if (view_scratch && V > 0) {
    hipLaunchKernelGGL(raster_project_kernel, raster_grid(V), dim3(RASTER_BLOCK), 0, s, vertices, (uint32_t)V, *view,
                       view_scratch);
    a.vertices = view_scratch;
    a.view_space = 1;
  }
  hipLaunchKernelGGL(raster_faces_kernel, raster_grid(F), dim3(RASTER_BLOCK), 0, s, a, *view);
  hipLaunchKernelGGL(raster_drain_kernel, dim3(RASTER_DRAIN_BLOCKS), dim3(RASTER_BLOCK), 0, s, a, *view);
  return check(false, s, "raster_view");
}

int gsr_raster_resolve(const uint64_t* keys, int32_t H, int32_t W, float* depth, int32_t* face_id, void* stream) {
  if (!raster_shape_ok(H, W)) return fail(GSR_E_BADARG, "H and W must lie in 1..2^14 with at most 2^28 pixels");
  if (!keys || !depth || !face_id) return fail(GSR_E_BADARG, "keys / depth / face_id is NULL");
  if (!aligned({depth, face_id}, 3u)) return fail(GSR_E_ALIGN, "depth and face_id must be 4-byte aligned");
  if (!aligned({keys}, 7u)) return fail(GSR_E_ALIGN, "keys must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(raster_resolve_kernel, raster_grid((int64_t)H * W), dim3(RASTER_BLOCK), 0, s, keys, (int)(H * W), depth,
                     face_id);
  return check(false, s, "raster_resolve");
}

int gsr_raster_count_faces(const uint64_t* keys, int32_t H, int32_t W, int64_t F, int32_t stamp_value, int32_t* stamp,
                           int32_t* counts, void* stream) {
  if (!raster_shape_ok(H, W)) return fail(GSR_E_BADARG, "H and W must lie in 1..2^14 with at most 2^28 pixels");
  if (F < 0 || F > (int64_t)INT32_MAX) return fail(GSR_E_BADARG, "F must lie in 0..2^31-1");
  if (stamp_value < 1) return fail(GSR_E_BADARG, "stamp_value must be positive (view + 1)");
  if (!keys) return fail(GSR_E_BADARG, "keys is NULL");
  if (F > 0 && (!stamp || !counts)) return fail(GSR_E_BADARG, "stamp / counts is NULL");
  if (F > 0 && stamp == counts) return fail(GSR_E_BADARG, "stamp must be an array of its own");
  if (!aligned({stamp, counts}, 3u)) return fail(GSR_E_ALIGN, "stamp and counts must be 4-byte aligned");
  if (!aligned({keys}, 7u)) return fail(GSR_E_ALIGN, "keys must be 8-byte aligned");
  if (F == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(raster_count_kernel, raster_grid((int64_t)H * W), dim3(RASTER_BLOCK), 0, s, keys, (int)(H * W), (int)W,
                     (uint32_t)F, stamp_value, stamp, counts);
  return check(false, s, "raster_count_faces");
}

}  // extern "C"

// Culling an extracted mesh by the views that saw it (include/gsr.h, ABI v41; mesh.py): the step of the
// DTU protocol (2DGS's cull_scan: a vertex stays where it lands on the dilated object mask of every view that sees it)
// and of the Tanks and Temples / Mip-NeRF 360 ones (a vertex no camera ever saw goes).  Both are rules on two counts per
// vertex, so the kernel counts and the caller decides.
//
// mesh_view_counts_kernel: one lane per vertex, 256-lane workgroups, no grid-stride loop, no LDS, no atomics, nothing
// waits on another workgroup.  The loop over the S views runs inside the kernel; the 96-byte table row of trip s is the
// same for every lane, so it arrives through scalar loads, and what a lane gathers per view is one mask byte and / or
// one depth float.  The pair's float32 arithmetic is csrc/mesh_cull_math.h (the unit is built with -ffp-contract=off).
// Both counters live in registers and are written once: the same bits from run to run.  Every gather is behind the
// in-image test of cull_view_test, formed from the row's own width and height.
//
// mesh_face_keep_kernel: keep[f] = all three corners kept; a corner outside 0..V-1 is never used as an index.
//
// mask_dilate_kernel<pass>: the (2r + 1)^2 square as two separable passes, rows (pass 0, mask -> tmp) then columns
// (pass 1, tmp -> out); one lane per pixel walks its 2r + 1 window, clipped to the image, and stops at the first set
// pixel.  Neighbouring lanes are neighbours in x in both passes, so the column pass reads whole rows of tmp.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "mesh_cull_math.h"

namespace gsr {

namespace {

constexpr int CULL_BLOCK = 256;

__global__ __launch_bounds__(CULL_BLOCK) void mesh_view_counts_kernel(const float* __restrict__ vertices, int64_t V,
                                                                      const GsrCullView* __restrict__ views, int S,
                                                                      float near, float depth_tol, int accumulate,
                                                                      int32_t* in_view, int32_t* visible) {
  const int64_t i = (int64_t)blockIdx.x * CULL_BLOCK + threadIdx.x;
  if (i >= V) return;
  const float* __restrict__ p = vertices + 3 * (size_t)i;
  const float x = p[0], y = p[1], z = p[2];
  int n_in = accumulate ? in_view[i] : 0, n_vis = accumulate ? visible[i] : 0;
  for (int s = 0; s < S; ++s) {
    const int r = cull_view_test(views[s], x, y, z, near, depth_tol);    // views[s]: uniform across the wave, scalar loads
    n_in += r & CULL_IN_VIEW;
    n_vis += (r & CULL_VISIBLE) >> 1;
  }
  in_view[i] = n_in;
  visible[i] = n_vis;
}

__global__ __launch_bounds__(CULL_BLOCK) void mesh_face_keep_kernel(const int32_t* __restrict__ faces,
                                                                    const uint8_t* __restrict__ vkeep, int64_t F, uint32_t V,
                                                                    uint8_t* __restrict__ keep, int32_t* status) {
  const int64_t f = (int64_t)blockIdx.x * CULL_BLOCK + threadIdx.x;
  if (f >= F) return;
  const int32_t* __restrict__ row = faces + 3 * (size_t)f;
  const uint32_t a = (uint32_t)row[0], b = (uint32_t)row[1], c = (uint32_t)row[2];       // a negative index is large
  if (a >= V || b >= V || c >= V) {
    atomicOr(status, 1);
    keep[f] = 0;
    return;
  }
  keep[f] = (uint8_t)((vkeep[a] != 0) & (vkeep[b] != 0) & (vkeep[c] != 0));
}

// PASS 0: dst[y, x] = any src[y, x - r .. x + r];  PASS 1: dst[y, x] = any src[y - r .. y + r, x]; outside counts as 0
template <int PASS>
__global__ __launch_bounds__(CULL_BLOCK) void mask_dilate_kernel(const uint8_t* __restrict__ src, int H, int W, int r,
                                                                 uint8_t* __restrict__ dst) {
  const int pix = (int)(blockIdx.x * CULL_BLOCK + threadIdx.x);          // H W <= 2^28
  if (pix >= H * W) return;
  const int y = pix / W, x = pix - y * W;
  const int at = PASS == 0 ? x : y, n = PASS == 0 ? W : H, step = PASS == 0 ? 1 : W;
  const int lo = at - r < 0 ? 0 : at - r, hi = at + r > n - 1 ? n - 1 : at + r;      // r <= 1024: no overflow
  const uint8_t* __restrict__ centre = src + pix;                         // centre[(k - at) step], k in [lo, hi]: inside the image
  uint8_t set = 0;
  for (int k = lo; k <= hi && !set; ++k) set = centre[(ptrdiff_t)(k - at) * step] != 0;
  dst[pix] = set;
}

inline dim3 cull_grid(int64_t n) { return dim3((unsigned)((n + CULL_BLOCK - 1) / CULL_BLOCK)); }
inline bool finite(float v) { return v - v == 0.0f; }                     // false for NaN and +-inf

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

int gsr_cull_view_counts(const float* vertices, int64_t V, const GsrCullView* views, int32_t S, float near_plane,
                         float depth_tol, int32_t accumulate, int32_t* in_view, int32_t* visible, void* stream) {
  if (V < 0 || V > (int64_t)INT32_MAX) return fail(GSR_E_BADARG, "V must lie in 0..2^31-1");
  if (S < 0 || S > GSR_CULL_MAX_VIEWS) return fail(GSR_E_BADARG, "S must lie in 0..65535");
  if (S > 0 && !views) return fail(GSR_E_BADARG, "the view table is NULL");
  if (!(near_plane > 0.0f) || !finite(near_plane)) return fail(GSR_E_BADARG, "near must be positive and finite");
  if (!(depth_tol >= 0.0f) || !finite(depth_tol)) return fail(GSR_E_BADARG, "depth_tol must be finite and not negative");
  if (V > 0 && (!vertices || !in_view || !visible)) return fail(GSR_E_BADARG, "vertices / in_view / visible is NULL");
  if (!aligned({vertices, in_view, visible}, 3u)) return fail(GSR_E_ALIGN, "vertices, in_view and visible must be 4-byte aligned");
  if (!aligned({views}, 7u)) return fail(GSR_E_ALIGN, "the view table must be 8-byte aligned");
  if (V == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mesh_view_counts_kernel, cull_grid(V), dim3(CULL_BLOCK), 0, s, vertices, V, views, (int)S, near_plane,
                     depth_tol, (int)accumulate, in_view, visible);
  return check(false, s, "mesh_view_counts");
}

int gsr_cull_face_keep(const int32_t* faces, const uint8_t* vkeep, int64_t F, int64_t V, uint8_t* keep, int32_t* status,
                       void* stream) {
  if (F < 0 || F > (int64_t)INT32_MAX || V < 0 || V > (int64_t)INT32_MAX)
    return fail(GSR_E_BADARG, "F and V must lie in 0..2^31-1");
  if (!status) return fail(GSR_E_BADARG, "status is NULL");
  if (F > 0 && (!faces || !keep)) return fail(GSR_E_BADARG, "faces / keep is NULL");
  if (F > 0 && V > 0 && !vkeep) return fail(GSR_E_BADARG, "vkeep is NULL");
  if (!aligned({faces, status}, 3u)) return fail(GSR_E_ALIGN, "faces / status must be 4-byte aligned");
  if (F == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mesh_face_keep_kernel, cull_grid(F), dim3(CULL_BLOCK), 0, s, faces, vkeep, F, (uint32_t)V, keep,
                     status);
  return check(false, s, "mesh_face_keep");
}

int gsr_mask_dilate(const uint8_t* mask, int32_t H, int32_t W, int32_t radius, uint8_t* tmp, uint8_t* out, void* stream) {
  if (!mask || !tmp || !out) return fail(GSR_E_BADARG, "mask / tmp / out is NULL");
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "H and W must be positive and H * W at most 2^28");
  if (radius < 0 || radius > GSR_DILATE_MAX_RADIUS) return fail(GSR_E_BADARG, "radius must lie in 0..1024");
  if (tmp == mask || tmp == out) return fail(GSR_E_BADARG, "tmp must be an array of its own");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid = cull_grid((int64_t)H * W);
  hipLaunchKernelGGL(mask_dilate_kernel<0>, grid, dim3(CULL_BLOCK), 0, s, mask, (int)H, (int)W, (int)radius, tmp);
  hipLaunchKernelGGL(mask_dilate_kernel<1>, grid, dim3(CULL_BLOCK), 0, s, (const uint8_t*)tmp, (int)H, (int)W, (int)radius,
                     out);
  return check(false, s, "mask_dilate");
}

}  // extern "C"

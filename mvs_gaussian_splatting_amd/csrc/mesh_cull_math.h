// One (vertex, view) pair of csrc/mesh_cull.hip (mesh.vertex_view_counts), written once for device and
// host: tests/mesh_cull_host_check.cpp builds it with the host compiler, so the float32 operation order below is checked
// against the numpy restatement (tests/mesh_cull_restate.py) bit for bit without a GPU.
//
// float32, every operation rounded on its own (both builds pass -ffp-contract=off):
//     (xv, yv, zv) = (x, y, z, 1) through world_to_view, the association of mvs_geom.h's mvs_transform
//     out unless zv > near                                             (a NaN fails)
//     cx = ((float)width - 1) * 0.5f      cy = ((float)height - 1) * 0.5f
//     u = (fx * xv) / zv + cx             v = (fy * yv) / zv + cy
//     ix = floorf(u + 0.5f)               iy = floorf(v + 0.5f)
//     out unless 0 <= ix && ix <= width - 1 && 0 <= iy && iy <= height - 1      (in float; a NaN fails)
//     IN VIEW
//     idx = (size_t)(int)iy * width + (int)ix                          (every gather is behind the test above)
//     out if mask and mask[idx] == 0
//     out if depth and not (ds = depth[idx]; ds > 0 && zv - ds <= depth_tol * ds)
//     VISIBLE
//
// Safety.  ix and iy are integers in [0, width - 1] x [0, height - 1] when the test passes -- width and height at most
// 2^24 convert to float exactly -- so idx lies inside [0, width height); the table row must describe its arrays.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gsr.h"

#ifndef GSR_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GSR_HD __host__ __device__ inline
#else
#define GSR_HD inline
#endif
#endif

namespace gsr {

constexpr int CULL_IN_VIEW = 1, CULL_VISIBLE = 2;      // bits of cull_view_test's result

// (x, y, z, 1) through M, row-vector convention: mvs_transform's association
GSR_HD void cull_transform(const float* M, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = ((x * M[0] + y * M[4]) + z * M[8]) + M[12];
  oy = ((x * M[1] + y * M[5]) + z * M[9]) + M[13];
  oz = ((x * M[2] + y * M[6]) + z * M[10]) + M[14];
}

// -> 0, CULL_IN_VIEW, or CULL_IN_VIEW | CULL_VISIBLE
GSR_HD int cull_view_test(const GsrCullView& view, float x, float y, float z, float near, float depth_tol) {
  float xv, yv, zv;
  cull_transform(view.world_to_view, x, y, z, xv, yv, zv);
  if (!(zv > near)) return 0;
  const float W = (float)view.width, H = (float)view.height;
  const float cx = (W - 1.0f) * 0.5f, cy = (H - 1.0f) * 0.5f;
  const float u = (view.fx * xv) / zv + cx, v = (view.fy * yv) / zv + cy;
  const float ix = floorf(u + 0.5f), iy = floorf(v + 0.5f);
  if (!(ix >= 0.0f && ix <= W - 1.0f && iy >= 0.0f && iy <= H - 1.0f)) return 0;   // a NaN fails
  const size_t idx = (size_t)(int)iy * (size_t)view.width + (size_t)(int)ix;
  if (view.mask && view.mask[idx] == 0) return CULL_IN_VIEW;
  if (view.depth) {
    const float ds = view.depth[idx];
    if (!(ds > 0.0f && zv - ds <= depth_tol * ds)) return CULL_IN_VIEW;
  }
  return CULL_IN_VIEW | CULL_VISIBLE;
}

}  // namespace gsr

// One (face, view) pair of csrc/mesh_raster.hip (mesh.rasterize_mesh, mesh.face_view_counts), written
// once for device and host: tests/mesh_raster_host_check.cpp builds it with the host compiler, so the rule below is checked
// against the numpy restatement (tests/mesh_raster_restate.py) bit for bit without a GPU.
//
// float32 up to the snap, every operation rounded on its own (both builds pass -ffp-contract=off); integers from there on;
// float64 for the depth, rounded to float32 once.
//
//  1. To view space.  (xv, yv, zv) of each corner = cull_transform of csrc/mesh_cull_math.h.
//  2. Near plane.  inside(k) = zv_k > near (a NaN fails).  All three inside: the face goes on as it is.  None inside: the
//     face is dropped.  Otherwise Sutherland-Hodgman against z = near: for the edges (0,1), (1,2), (2,0) in this order,
//     emit the edge's first corner if it is inside, then, if exactly one end is inside, the intersection
//         t = (near - za) / (zb - za),  x = xa + t (xb - xa),  y = ya + t (yb - ya),  z = near exactly
//     with a ALWAYS the inside end and b the outside one: two faces that share a clipped edge compute the same bits.  That
//     gives 3 or 4 vertices o0.., and the pieces (o0, o1, o2) and (o0, o2, o3).  Pieces carry the parent face's index.
//  3. To the image.  cx = ((float)W - 1) * 0.5f, cy likewise;  u = (fx * xv) / zv + cx,  v = (fy * yv) / zv + cy: pixel
//     centres at integers, mesh_cull's convention.  X = (int32) rintf(u * 256.0f): 8 sub-pixel bits.  A piece with a
//     coordinate whose rounded value lies outside [-2^29, 2^29] (a NaN and an infinity do) is DROPPED AND COUNTED: the
//     documented limit (+-2^21 pixels: more than 89.9 degrees off axis at the near plane).
//  4. Coverage.  edge(a, b, P) = (Xb - Xa) (Py - Ya) - (Yb - Ya) (Px - Xa) in int64.  A = edge(p0, p1, p2); A = 0 drops the
//     piece; A < 0 (the piece faces the camera: y points down, so its normal (p1 - p0) x (p2 - p0) has z < 0) swaps p1 and
//     p2; with cull_backfaces a piece with A > 0 before the swap is dropped.  At the pixel centre P = (256 ix, 256 iy):
//     E0 = edge(p1, p2, P), E1 = edge(p2, p0, P), E2 = edge(p0, p1, P); E0 + E1 + E2 = A.  The centre is covered when every
//     E_k > 0, or E_k = 0 on a top or left edge: with (dx, dy) = b - a of that edge, dy < 0 (left) or dy = 0 and dx > 0
//     (top) -- Direct3D's rule for the orientation normalised to (clockwise on a screen whose y points down).
//     Only the pixels of the piece's bounding box, clipped to the image, are visited:
//     ceil(min X / 256) .. floor(max X / 256) within 0 .. W - 1, rows likewise.
//     Exactness: |X|, |Y| <= 2^29 and 0 <= Px, Py < 2^14 * 2^8 = 2^22, so every difference is below 2^30 + 2^22 < 2^31,
//     every product below 2^62 and every edge function and A below 2^63 in magnitude: int64 never overflows.
//  5. Depth.  lambda_k = (double)E_k / (double)A;  1/z = (lambda_0 / z0 + lambda_1 / z1) + lambda_2 / z2 in float64, in that
//     order; z = (float)(1.0 / that); then z is clamped to [min z_k, max z_k] of the piece.  So z >= near > 0 and its bits
//     order as an unsigned integer.
//  6. key = (uint64)float_bits(z) << 32 | face.  The z-buffer keeps the smallest key per pixel.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "mesh_cull_math.h"

namespace gsr {

constexpr int RASTER_SUB = 256;                          // sub-pixel units per pixel
constexpr float RASTER_COORD_MAX = 536870912.0f;         // 2^29 sub-pixel units

struct RasterVert {
  float x, y, z;                                         // view space
};

struct RasterPiece {
  int32_t X[3], Y[3];                                    // snapped, orientation normalised: area > 0
  float z[3];
  int64_t area;
  int32_t x0, x1, y0, y1;                                // the pixels to visit, inclusive; empty when x0 > x1 or y0 > y1
};

constexpr int RASTER_PIECE_NONE = 0, RASTER_PIECE_OK = 1, RASTER_PIECE_DROPPED = -1;

// step 2: out[0 .. n) with n = 0, 3 or 4
GSR_HD int raster_clip(const RasterVert* v, float near, RasterVert* out) {
  const bool in0 = v[0].z > near, in1 = v[1].z > near, in2 = v[2].z > near;
  if (in0 && in1 && in2) {
    out[0] = v[0];
    out[1] = v[1];
    out[2] = v[2];
    return 3;
  }
  if (!in0 && !in1 && !in2) return 0;
  const bool in[3] = {in0, in1, in2};
  int n = 0;
  for (int i = 0; i < 3; ++i) {
    const int j = i == 2 ? 0 : i + 1;
    if (in[i]) out[n++] = v[i];
    if (in[i] != in[j]) {
      const RasterVert& a = in[i] ? v[i] : v[j];         // the inside end
      const RasterVert& b = in[i] ? v[j] : v[i];
      const float t = (near - a.z) / (b.z - a.z);
      RasterVert p;
      p.x = a.x + t * (b.x - a.x);
      p.y = a.y + t * (b.y - a.y);
      p.z = near;
      out[n++] = p;
    }
  }
  return n;
}

GSR_HD bool raster_snap(float u, int32_t& X) {
  const float r = rintf(u * 256.0f);
  if (!(r >= -RASTER_COORD_MAX && r <= RASTER_COORD_MAX)) return false;      // a NaN fails
  X = (int32_t)r;
  return true;
}

GSR_HD int64_t raster_edge(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py) {
  return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

// steps 3 and 4 up to the bounding box: RASTER_PIECE_OK, _NONE (no area, or culled) or _DROPPED (out of range: counted)
GSR_HD int raster_setup(const GsrCullView& view, const RasterVert& a, const RasterVert& b, const RasterVert& c,
                        bool cull_backfaces, RasterPiece& p) {
  const float W = (float)view.width, H = (float)view.height;
  const float cx = (W - 1.0f) * 0.5f, cy = (H - 1.0f) * 0.5f;
  const RasterVert* v[3] = {&a, &b, &c};
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    const float u = (view.fx * v[k]->x) / v[k]->z + cx, w = (view.fy * v[k]->y) / v[k]->z + cy;
    ok = raster_snap(u, p.X[k]) && ok;
    ok = raster_snap(w, p.Y[k]) && ok;
    p.z[k] = v[k]->z;
  }
  if (!ok) return RASTER_PIECE_DROPPED;
  int64_t area = raster_edge(p.X[0], p.Y[0], p.X[1], p.Y[1], p.X[2], p.Y[2]);
  if (area == 0) return RASTER_PIECE_NONE;
  if (area < 0) {
    int32_t ti = p.X[1];
    p.X[1] = p.X[2];
    p.X[2] = ti;
    ti = p.Y[1];
    p.Y[1] = p.Y[2];
    p.Y[2] = ti;
    const float tf = p.z[1];
    p.z[1] = p.z[2];
    p.z[2] = tf;
    area = -area;
  } else if (cull_backfaces) {
    return RASTER_PIECE_NONE;
  }
  p.area = area;
  int32_t lox = p.X[0], hix = p.X[0], loy = p.Y[0], hiy = p.Y[0];
  for (int k = 1; k < 3; ++k) {
    lox = p.X[k] < lox ? p.X[k] : lox;
    hix = p.X[k] > hix ? p.X[k] : hix;
    loy = p.Y[k] < loy ? p.Y[k] : loy;
    hiy = p.Y[k] > hiy ? p.Y[k] : hiy;
  }
  // ceil(lo / 256) and floor(hi / 256) for either sign: >> of a negative int32 is arithmetic on every compiler used here
  p.x0 = (lox + (RASTER_SUB - 1)) >> 8;
  p.x1 = hix >> 8;
  p.y0 = (loy + (RASTER_SUB - 1)) >> 8;
  p.y1 = hiy >> 8;
  p.x0 = p.x0 < 0 ? 0 : p.x0;
  p.y0 = p.y0 < 0 ? 0 : p.y0;
  p.x1 = p.x1 > view.width - 1 ? view.width - 1 : p.x1;
  p.y1 = p.y1 > view.height - 1 ? view.height - 1 : p.y1;
  return RASTER_PIECE_OK;
}

GSR_HD bool raster_top_left(int32_t dx, int32_t dy) { return dy < 0 || (dy == 0 && dx > 0); }

// steps 4 and 5 at the pixel centre (ix, iy): covered?  then z
GSR_HD bool raster_cover(const RasterPiece& p, int32_t ix, int32_t iy, float& z) {
  const int64_t px = (int64_t)ix * RASTER_SUB, py = (int64_t)iy * RASTER_SUB;
  const int64_t e0 = raster_edge(p.X[1], p.Y[1], p.X[2], p.Y[2], px, py);
  const int64_t e1 = raster_edge(p.X[2], p.Y[2], p.X[0], p.Y[0], px, py);
  const int64_t e2 = raster_edge(p.X[0], p.Y[0], p.X[1], p.Y[1], px, py);
  if (e0 < 0 || e1 < 0 || e2 < 0) return false;
  if (e0 == 0 && !raster_top_left(p.X[2] - p.X[1], p.Y[2] - p.Y[1])) return false;
  if (e1 == 0 && !raster_top_left(p.X[0] - p.X[2], p.Y[0] - p.Y[2])) return false;
  if (e2 == 0 && !raster_top_left(p.X[1] - p.X[0], p.Y[1] - p.Y[0])) return false;
  const double A = (double)p.area;
  const double l0 = (double)e0 / A, l1 = (double)e1 / A, l2 = (double)e2 / A;
  const double inv = (l0 / (double)p.z[0] + l1 / (double)p.z[1]) + l2 / (double)p.z[2];
  float zf = (float)(1.0 / inv);
  float lo = p.z[0], hi = p.z[0];
  for (int k = 1; k < 3; ++k) {
    lo = p.z[k] < lo ? p.z[k] : lo;
    hi = p.z[k] > hi ? p.z[k] : hi;
  }
  zf = zf < lo ? lo : zf;
  zf = zf > hi ? hi : zf;
  z = zf;
  return true;
}

GSR_HD uint64_t raster_key(float z, uint32_t face) {
  uint32_t bits;
  memcpy(&bits, &z, sizeof bits);
  return (uint64_t)bits << 32 | (uint64_t)face;
}

// steps 1 and 2 of one face: the view-space corners (NaN and all) -> out[0 .. n)
GSR_HD int raster_face(const GsrCullView& view, const float* pa, const float* pb, const float* pc, float near,
                       RasterVert* out) {
  RasterVert v[3];
  cull_transform(view.world_to_view, pa[0], pa[1], pa[2], v[0].x, v[0].y, v[0].z);
  cull_transform(view.world_to_view, pb[0], pb[1], pb[2], v[1].x, v[1].y, v[1].z);
  cull_transform(view.world_to_view, pc[0], pc[1], pc[2], v[2].x, v[2].y, v[2].z);
  return raster_clip(v, near, out);
}

}  // namespace gsr

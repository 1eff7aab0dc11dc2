// Multi-view geometric consistency of depth maps and back-projection to points (include/gsr.h, ABI v34; mvs.py;
// DESIGN.md §7.21): the check of MVSNet's and COLMAP's fusion.  A reference pixel is taken into a source view at its
// depth, the source's depth is read there (bilinear), the result is taken back, and the pixel is consistent with that
// source when it lands where it started, at the depth it started with.
//
// Pixel convention of tsdf.hip: the centre of pixel (px, py) is the ray through ((px - cx) / fx, (py - cy) / fy, 1),
// cx = (W - 1) / 2, cy = (H - 1) / 2, formed in float32 as (W - 1) * 0.5.  Matrices in the row-vector convention,
// M[4 * row + col]; per source A = ref_to_src = inv(V_r) V_s and B = src_to_ref = inv(V_s) V_r, formed on the host in
// float64 from the float32 world_view_transforms and rounded once.
//
// mvs_consistency_kernel, per reference pixel (px, py) with d = depth[py, px], float32, every operation rounded on its
// own (the unit is built with -ffp-contract=off).  If d is not > 0: count = 0, fused = 0.  Otherwise n = 0, sum = 0 and
// for each source in table order:
//     xr = ((px - cx_r) * d) / fx_r      yr = ((py - cy_r) * d) / fy_r      zr = d
//     xs = ((xr A[0] + yr A[4]) + zr A[8]) + A[12]     ys: A[1], A[5], A[9], A[13]     zs: A[2], A[6], A[10], A[14]
//     next source unless zs > 0.2
//     us = (fx_s xs) / zs + cx_s         vs = (fy_s ys) / zs + cy_s
//     x0 = floorf(us), y0 = floorf(vs)   next source unless 0 <= x0, x0 + 1 <= W_s - 1, 0 <= y0, y0 + 1 <= H_s - 1 (NaN fails)
//     ax = us - x0, ay = vs - y0         d00, d10, d01, d11 = source depth at (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1)
//     next source unless all four > 0
//     ds = (d00 (1 - ax) + d10 ax) (1 - ay) + (d01 (1 - ax) + d11 ax) ay
//     xb' = ((us - cx_s) * ds) / fx_s    yb' = ((vs - cy_s) * ds) / fy_s    zb' = ds
//     (xb, yb, zb) = (xb', yb', zb') through B, same association as through A
//     next source unless zb > 0.2
//     ub = (fx_r xb) / zb + cx_r         vb = (fy_r yb) / zb + cy_r
//     du = ub - px, dv = vb - py
//     consistent iff  du du + dv dv < pix_thresh pix_thresh   and   fabsf(zb - d) < depth_thresh * d
//     if consistent:  n += 1;  sum += zb
// Then count[py, px] = n (uint8) and fused[py, px] = n >= min_views ? (d + sum) / (float)(n + 1) : 0.  Every pixel of
// both outputs is written.
//
// depth_backproject_kernel, one lane per pixel: (xr, yr, zr) as above through cam_to_world (the host's float64 inverse
// of the view matrix, rounded once) with the same association -> xyz[py W + px]; a pixel without depth writes a zero row.
//
// Launch shape: 256-lane workgroups, a tile of MVS_TILE_X x (256 / MVS_TILE_X) reference pixels (64 x 4: a wave is 64
// x-neighbours of one row, reads 256 consecutive bytes of the reference and writes 256 + 64; profiles/mvs/NOTES.md has
// the comparison with 16 x 16).  One lane per pixel, no grid-stride loop, no LDS, no atomics, nothing waits on another
// workgroup.  The loop over the sources runs inside the kernel; its trip count S <= 64 is a kernel argument and the
// table row of trip s is the same for every lane, so its 152 bytes arrive through scalar loads.  A pixel's sum is
// accumulated in table order in registers: the same bits from run to run.
//
// Safety.  Every gather is behind the footprint test in float32, formed from the table's own W_s, H_s: 0 <= x0 and
// x0 + 1 <= W_s - 1 (likewise y), so the four addresses lie inside [0, W_s H_s); a NaN fails the test.  The entry point
// refuses reference images above 2^28 pixels, so py W + px stays in int; the source index is formed in size_t.  The
// table is device memory that the host cannot inspect: a row whose width / height do not describe its depth array is
// the caller's error (mvs.depth_consistency checks every source against its camera before it builds the table).
#include "gsr_common.h"
#include "gsr_entry.h"
#include "mvs_geom.h"      // the round trip, shared with mvs_loss.hip: MVS_TILE_X, MVS_BLOCK, mvs_transform, mvs_round_trip

namespace gsr {

namespace {

struct Mat4 {
  float m[16];
};

__global__ __launch_bounds__(MVS_BLOCK) void mvs_consistency_kernel(const float* __restrict__ depth, int H, int W, float fx,
                                                                    float fy, const GsrMvsSource* __restrict__ sources,
                                                                    int S, float pix_thresh, float depth_thresh,
                                                                    int min_views, unsigned xtiles,
                                                                    uint8_t* __restrict__ count, float* __restrict__ fused) {
  const unsigned tx = blockIdx.x % xtiles, ty = blockIdx.x / xtiles;
  const int px = (int)(tx * MVS_TILE_X + threadIdx.x % MVS_TILE_X);
  const int py = (int)(ty * MVS_TILE_Y + threadIdx.x / MVS_TILE_X);
  if (px >= W || py >= H) return;
  const int pix = py * W + px;
  const float d = depth[pix];
  if (!(d > 0.0f)) {
    count[pix] = 0;
    fused[pix] = 0.0f;
    return;
  }
  const float fpx = (float)px, fpy = (float)py;
  const float cx = ((float)W - 1.0f) * 0.5f, cy = ((float)H - 1.0f) * 0.5f;
  const float xr = ((fpx - cx) * d) / fx, yr = ((fpy - cy) * d) / fy;
  const float pix2 = pix_thresh * pix_thresh, dtol = depth_thresh * d;
  int n = 0;
  float sum = 0.0f;
  for (int s = 0; s < S; ++s) {
    MvsTrip t;                                                           // sources[s]: uniform across the wave, scalar loads
    if (!mvs_round_trip(sources[s], fpx, fpy, cx, cy, fx, fy, xr, yr, d, t)) continue;
    if (t.du * t.du + t.dv * t.dv < pix2 && fabsf(t.zb - d) < dtol) {
      n += 1;
      sum += t.zb;
    }
  }
  count[pix] = (uint8_t)n;
  fused[pix] = n >= min_views ? (d + sum) / (float)(n + 1) : 0.0f;
}

__global__ __launch_bounds__(MVS_BLOCK) void depth_backproject_kernel(const float* __restrict__ depth, int H, int W, float fx,
                                                                      float fy, Mat4 c2w, float* __restrict__ xyz) {
  const int pix = (int)(blockIdx.x * MVS_BLOCK + threadIdx.x);
  if (pix >= H * W) return;
  const int py = pix / W, px = pix - py * W;
  const float d = depth[pix];
  float x = 0.0f, y = 0.0f, z = 0.0f;
  if (d > 0.0f) {
    const float cx = ((float)W - 1.0f) * 0.5f, cy = ((float)H - 1.0f) * 0.5f;
    const float xr = (((float)px - cx) * d) / fx, yr = (((float)py - cy) * d) / fy;
    mvs_transform(c2w.m, xr, yr, d, x, y, z);
  }
  float* __restrict__ row = xyz + 3 * (size_t)pix;
  row[0] = x;
  row[1] = y;
  row[2] = z;
}

void launch_mvs_consistency(const float* depth, int H, int W, float fx, float fy, const GsrMvsSource* sources, int S,
                            float pix_thresh, float depth_thresh, int min_views, uint8_t* count, float* fused,
                            hipStream_t s) {
  const unsigned xtiles = ((unsigned)W + MVS_TILE_X - 1) / MVS_TILE_X, ytiles = ((unsigned)H + MVS_TILE_Y - 1) / MVS_TILE_Y;
  hipLaunchKernelGGL(mvs_consistency_kernel, dim3(xtiles * ytiles), dim3(MVS_BLOCK), 0, s, depth, H, W, fx, fy, sources, S,
                     pix_thresh, depth_thresh, min_views, xtiles, count, fused);
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

int gsr_mvs_consistency(const float* depth, int32_t H, int32_t W, float fx, float fy, const GsrMvsSource* sources, int32_t S,
                        float pix_thresh, float depth_thresh, int32_t min_views, uint8_t* count, float* fused,
                        void* stream) {
  if (!depth || !count || !fused) return fail(GSR_E_BADARG, "depth / count / fused is NULL");
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "H and W must be positive and H * W at most 2^28");
  if (S < 0 || S > GSR_MVS_MAX_SOURCES) return fail(GSR_E_BADARG, "S must lie in 0..64");
  if (S > 0 && !sources) return fail(GSR_E_BADARG, "the source table is NULL");
  if (!mvs_positive_finite(fx) || !mvs_positive_finite(fy)) return fail(GSR_E_BADARG, "fx and fy must be positive and finite");
  if (!mvs_positive_finite(pix_thresh) || !mvs_positive_finite(depth_thresh))
    return fail(GSR_E_BADARG, "pix_thresh and depth_thresh must be positive and finite");
  if (min_views < 0) return fail(GSR_E_BADARG, "min_views must not be negative");
  if (!aligned({depth, fused}, 3u)) return fail(GSR_E_ALIGN, "depth and fused must be 4-byte aligned");
  if (!aligned({sources}, 7u)) return fail(GSR_E_ALIGN, "the source table must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mvs_consistency(depth, H, W, fx, fy, sources, S, pix_thresh, depth_thresh, min_views, count, fused, s);
  return check(false, s, "mvs_consistency");
}

int gsr_depth_backproject(const float* depth, int32_t H, int32_t W, float fx, float fy, const float* cam_to_world,
                          float* xyz, void* stream) {
  if (H < 0 || W < 0 || (int64_t)H * (int64_t)W > (int64_t)1 << 28)
    return fail(GSR_E_BADARG, "H and W must not be negative and H * W at most 2^28");
  if (!mvs_positive_finite(fx) || !mvs_positive_finite(fy)) return fail(GSR_E_BADARG, "fx and fy must be positive and finite");
  if (!cam_to_world) return fail(GSR_E_BADARG, "cam_to_world is NULL");
  if (H == 0 || W == 0) return 0;
  if (!depth || !xyz) return fail(GSR_E_BADARG, "depth / xyz is NULL");
  if (!aligned({depth, xyz, cam_to_world}, 3u)) return fail(GSR_E_ALIGN, "depth, xyz and cam_to_world must be 4-byte aligned");
  Mat4 c2w;
  for (int i = 0; i < 16; ++i) c2w.m[i] = cam_to_world[i];
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned blocks = (unsigned)(((int64_t)H * W + MVS_BLOCK - 1) / MVS_BLOCK);
  hipLaunchKernelGGL(depth_backproject_kernel, dim3(blocks), dim3(MVS_BLOCK), 0, s, depth, (int)H, (int)W, fx, fy, c2w, xyz);
  return check(false, s, "depth_backproject");
}

}  // extern "C"

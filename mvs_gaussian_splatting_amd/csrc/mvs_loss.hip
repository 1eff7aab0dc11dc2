// Multi-view geometric consistency loss of a (reference, source) pair of depth maps, value and both gradients in one
// launch (include/gsr.h, ABI v35; mvs.py): the multi-view geometric term of PGSR, the forward-backward
// reprojection error of mvs.hip turned into a training signal.
//
// Per reference pixel (px, py) with d = ref_depth[py, px] > 0, float32, every operation rounded on its own (the unit is
// built with -ffp-contract=off): the round trip of mvs.hip's header comment up to (ub, vb, zb), the same code
// (mvs_geom.h) and so the same bits.  Then
//     du = ub - px, dv = vb - py         phi = sqrtf(du du + dv dv)
//     valid iff every gate of the trip passed, phi < pix_max, and (depth_thresh > 0 only) fabsf(zb - d) < depth_thresh d
//     w = expf(-phi)   (a constant for the gradients, as in PGSR)        e = w phi
//     raw = sum_valid e      n = the number of valid pixels      loss = raw / max(n, 1)
// Backward of raw, validity a decision without gradient, floor piecewise constant; reverse mode, per valid pixel with
// phi > 0 (phi == 0: value 0, gradients 0):
//     g_du = du / phi, g_dv = dv / phi
//     g_xb = (g_du fx_r) / zb      g_yb = (g_dv fy_r) / zb      g_zb = -(((g_du fx_r) xb + (g_dv fy_r) yb) / (zb zb))
//     g_xb' = (g_xb B[0] + g_yb B[1]) + g_zb B[2]      g_yb': B[4], B[5], B[6]      g_zb': B[8], B[9], B[10]
//     g_ds = (g_zb' + (g_xb' (us - cx_s)) / fx_s) + (g_yb' (vs - cy_s)) / fy_s
//     sx = (d10 - d00) (1 - ay) + (d11 - d01) ay       sy = (d01 (1 - ax) + d11 ax) - (d00 (1 - ax) + d10 ax)
//     g_us = (g_xb' ds) / fx_s + g_ds sx               g_vs = (g_yb' ds) / fy_s + g_ds sy
//     g_xs = (g_us fx_s) / zs      g_ys = (g_vs fy_s) / zs      g_zs = -(((g_us fx_s) xs + (g_vs fy_s) ys) / (zs zs))
//     g_xr = (g_xs A[0] + g_ys A[1]) + g_zs A[2]       g_yr: A[4], A[5], A[6]       g_zr: A[8], A[9], A[10]
//     grad_ref[py, px] = w ((g_xr ((px - cx_r) / fx_r) + g_yr ((py - cy_r) / fy_r)) + g_zr)
//     grad_src[y0, x0] += (w g_ds) ((1 - ax) (1 - ay))    [y0, x0 + 1] += (w g_ds) (ax (1 - ay))
//     grad_src[y0 + 1, x0] += (w g_ds) ((1 - ax) ay)      [y0 + 1, x0 + 1] += (w g_ds) (ax ay)
// Both are unit gradients of raw; the caller scales them by upstream / max(n, 1).
//
// Launch shape of mvs.hip: 256-lane workgroups over 64 x 4 reference pixels, one lane per pixel, no grid-stride loop,
// nothing waits on another workgroup.  The one table row is the same for every lane, so its 152 bytes arrive through
// scalar loads.  grad_ref is a gather: every lane writes its own pixel (zero where not valid), the same bits from run to
// run.  grad_src is a scatter: four atomicAdd(float*) per valid pixel into a map the entry point zeroed on the stream
// (global_atomic_add_f32, no compare-and-swap loop); the order of the additions varies, so grad_src is NOT
// bit-reproducible.  The loss: e in double, one (double sum, uint32 count) pair per workgroup in the workspace; a
// one-block kernel behind it adds the pairs and writes the record -- every sum in the fixed order of ordered_sum.h, the
// same bits from run to run.  LDS: the eight reduction slots only.
//
// Safety.  Every gather and every atomic is behind the footprint test of mvs_round_trip, formed from the row's own W_s,
// H_s, so the four addresses lie inside [0, W_s H_s) of the row's depth.  grad_src is sized by the caller's src_H, src_W:
// the kernel scatters only when they equal the row's height and width (a uniform test), so a row that does not describe
// grad_src leaves it zero instead of writing outside it.  The entry point refuses images above 2^28 pixels and launches
// of 2^32 work-items or more.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "mvs_geom.h"
#include "ordered_sum.h"

namespace gsr {

namespace {

constexpr int MVL_FIN_THREADS = 1024;

__global__ __launch_bounds__(MVS_BLOCK) void mvs_geo_loss_kernel(const float* __restrict__ depth, int H, int W, float fx,
                                                                 float fy, const GsrMvsSource* __restrict__ source,
                                                                 float pix_max, float depth_thresh, int src_H, int src_W,
                                                                 unsigned xtiles, float* __restrict__ grad_ref,
                                                                 float* __restrict__ grad_src,
                                                                 double* __restrict__ part_sum,
                                                                 uint32_t* __restrict__ part_n) {
  __shared__ PairSlots<double, MVS_BLOCK / WAVE> red;
  const unsigned tx = blockIdx.x % xtiles, ty = blockIdx.x / xtiles;
  const int px = (int)(tx * MVS_TILE_X + threadIdx.x % MVS_TILE_X);
  const int py = (int)(ty * MVS_TILE_Y + threadIdx.x / MVS_TILE_X);
  const bool in = px < W && py < H;
  const int pix = py * W + px;                                           // used under `in` only
  const GsrMvsSource& src = source[0];                                   // uniform across the grid: scalar loads
  const float d = in ? depth[pix] : 0.0f;
  bool valid = false;
  float e = 0.0f, g_ref = 0.0f;
  if (d > 0.0f) {
    const float fpx = (float)px, fpy = (float)py;
    const float cx = ((float)W - 1.0f) * 0.5f, cy = ((float)H - 1.0f) * 0.5f;
    const float xr = ((fpx - cx) * d) / fx, yr = ((fpy - cy) * d) / fy;
    MvsTrip t;
    if (mvs_round_trip(src, fpx, fpy, cx, cy, fx, fy, xr, yr, d, t)) {
      const float phi = sqrtf(t.du * t.du + t.dv * t.dv);
      valid = phi < pix_max && (!(depth_thresh > 0.0f) || fabsf(t.zb - d) < depth_thresh * d);
      if (valid && phi > 0.0f) {
        const float w = expf(-phi);
        e = w * phi;
        if (grad_ref || grad_src) {
          const float* __restrict__ A = src.ref_to_src;
          const float* __restrict__ B = src.src_to_ref;
          const float gu = (t.du / phi) * fx, gv = (t.dv / phi) * fy;
          const float g_xb = gu / t.zb, g_yb = gv / t.zb, g_zb = -((gu * t.xb + gv * t.yb) / (t.zb * t.zb));
          const float g_xb0 = (g_xb * B[0] + g_yb * B[1]) + g_zb * B[2];
          const float g_yb0 = (g_xb * B[4] + g_yb * B[5]) + g_zb * B[6];
          const float g_zb0 = (g_xb * B[8] + g_yb * B[9]) + g_zb * B[10];
          const float g_ds = (g_zb0 + (g_xb0 * (t.us - t.cxs)) / src.fx) + (g_yb0 * (t.vs - t.cys)) / src.fy;
          const float bx = 1.0f - t.ax, by = 1.0f - t.ay;
          if (grad_ref) {
            const float sx = (t.d10 - t.d00) * by + (t.d11 - t.d01) * t.ay;
            const float sy = (t.d01 * bx + t.d11 * t.ax) - (t.d00 * bx + t.d10 * t.ax);
            const float hu = ((g_xb0 * t.ds) / src.fx + g_ds * sx) * src.fx;
            const float hv = ((g_yb0 * t.ds) / src.fy + g_ds * sy) * src.fy;
            const float g_xs = hu / t.zs, g_ys = hv / t.zs, g_zs = -((hu * t.xs + hv * t.ys) / (t.zs * t.zs));
            const float g_xr = (g_xs * A[0] + g_ys * A[1]) + g_zs * A[2];
            const float g_yr = (g_xs * A[4] + g_ys * A[5]) + g_zs * A[6];
            const float g_zr = (g_xs * A[8] + g_ys * A[9]) + g_zs * A[10];
            g_ref = w * ((g_xr * ((fpx - cx) / fx) + g_yr * ((fpy - cy) / fy)) + g_zr);
          }
          if (grad_src && src.height == src_H && src.width == src_W) {   // uniform; the taps lie inside the row's size
            const float k = w * g_ds;
            float* __restrict__ row0 = grad_src + t.tap;
            float* __restrict__ row1 = row0 + src_W;
            atomicAdd(row0, k * (bx * by));
            atomicAdd(row0 + 1, k * (t.ax * by));
            atomicAdd(row1, k * (bx * t.ay));
            atomicAdd(row1 + 1, k * (t.ax * t.ay));
          }
        }
      }
    }
  }
  if (in && grad_ref) grad_ref[pix] = g_ref;

  // the workgroup's partial and count (ordered_sum.h)
  double ts = (double)e;
  uint32_t tn = valid ? 1u : 0u;
  ordered_pair_sum(ts, tn, red);
  if (threadIdx.x == 0) {
    part_sum[blockIdx.x] = ts;
    part_n[blockIdx.x] = tn;
  }
}

// One block: the pairs in the fixed order of ordered_pair_finish.
// record = {float raw / max(n, 1), uint32 n, float raw, 0}: written, not accumulated.
__global__ __launch_bounds__(MVL_FIN_THREADS) void mvs_geo_loss_finish_kernel(const double* __restrict__ part_sum,
                                                                              const uint32_t* __restrict__ part_n,
                                                                              unsigned nblocks, float* __restrict__ record) {
  __shared__ PairSlots<double, MVL_FIN_THREADS / WAVE> red;
  double ts;
  uint32_t tn;
  ordered_pair_finish(part_sum, part_n, nblocks, ts, tn, red);
  if (threadIdx.x != 0) return;
  record[0] = (float)(ts / (double)(tn > 0u ? tn : 1u));
  reinterpret_cast<uint32_t*>(record)[1] = tn;
  record[2] = (float)ts;
  record[3] = 0.0f;
}

// false when the image is refused or the launch would reach 2^32 work-items
bool mvs_geo_loss_blocks(int32_t H, int32_t W, unsigned* xtiles, unsigned* blocks) {
  if (!image_shape_ok(H, W)) return false;
  const unsigned long long xt = ((unsigned long long)W + MVS_TILE_X - 1) / MVS_TILE_X;
  const unsigned long long yt = ((unsigned long long)H + MVS_TILE_Y - 1) / MVS_TILE_Y;
  if (xt * yt * MVS_BLOCK >= (1ull << 32)) return false;                 // HIP's bound on the work-items of a launch
  *xtiles = (unsigned)xt;
  *blocks = (unsigned)(xt * yt);
  return true;
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_mvs_geo_loss_workspace_bytes(int32_t H, int32_t W) {
  unsigned xtiles, blocks;
  if (!mvs_geo_loss_blocks(H, W, &xtiles, &blocks)) return 0;
  return (size_t)blocks * (sizeof(double) + sizeof(uint32_t));
}

int gsr_mvs_geo_loss_fwd_bwd(const float* ref_depth, int32_t H, int32_t W, float fx, float fy, const GsrMvsSource* source,
                             float pix_max, float depth_thresh, float* record, float* grad_ref, float* grad_src,
                             int32_t src_H, int32_t src_W, void* workspace, void* stream) {
  if (!ref_depth || !source || !record || !workspace) return fail(GSR_E_BADARG, "ref_depth / source / record / workspace is NULL");
  unsigned xtiles, blocks;
  if (!mvs_geo_loss_blocks(H, W, &xtiles, &blocks))
    return fail(GSR_E_BADARG, "H and W must be positive, H * W at most 2^28 and the launch below 2^32 work-items");
  if (!mvs_positive_finite(fx) || !mvs_positive_finite(fy)) return fail(GSR_E_BADARG, "fx and fy must be positive and finite");
  if (!mvs_positive_finite(pix_max)) return fail(GSR_E_BADARG, "pix_max must be positive and finite");
  if (depth_thresh != depth_thresh) return fail(GSR_E_BADARG, "depth_thresh is NaN (<= 0 switches the depth test off)");
  if (grad_src && !image_shape_ok(src_H, src_W))
    return fail(GSR_E_BADARG, "grad_src needs the source's size: src_H and src_W positive, src_H * src_W at most 2^28");
  if (!aligned({ref_depth, record, grad_ref, grad_src}, 3u))
    return fail(GSR_E_ALIGN, "ref_depth, record, grad_ref and grad_src must be 4-byte aligned");
  if (!aligned({source, workspace}, 7u)) return fail(GSR_E_ALIGN, "the table row and the workspace must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (grad_src) GSR_HIP(hipMemsetAsync(grad_src, 0, (size_t)src_H * (size_t)src_W * sizeof(float), s));
  double* part_sum = static_cast<double*>(workspace);
  uint32_t* part_n = reinterpret_cast<uint32_t*>(part_sum + blocks);
  hipLaunchKernelGGL(mvs_geo_loss_kernel, dim3(blocks), dim3(MVS_BLOCK), 0, s, ref_depth, (int)H, (int)W, fx, fy, source,
                     pix_max, depth_thresh, (int)src_H, (int)src_W, xtiles, grad_ref, grad_src, part_sum, part_n);
  hipLaunchKernelGGL(mvs_geo_loss_finish_kernel, dim3(1), dim3(MVL_FIN_THREADS), 0, s, part_sum, part_n, blocks, record);
  return check(false, s, "mvs_geo_loss_fwd_bwd");
}

}  // extern "C"

// PGSR's unbiased depth of a rendered frame: the pixel's ray met with the blended plane, value and unit gradients in
// one launch (include/gsr.h, ABI v37; surface.plane_depth).  Inputs normal = sum w n ([3,H,W],
// un-normalised), distance = sum w d and alpha = sum w ([H,W] each).  Per pixel, with the pixel convention of
// GsrTsdfView and the normal-consistency kernel (cx = (W - 1) / 2, cy = (H - 1) / 2, fx, fy from the host):
//     r = ((x - cx) / fx, (y - cy) / fy, 1)        c = -(N . r)
//     valid = alpha >= alpha_min, D > 0, c > 0, c >= min_cos |N| |r|, every input finite, every result a float32
//     z = D / c        dz/dD = 1 / c        dz/dN = (D / c^2) r        on valid pixels, zeros elsewhere
// alpha cancels in the quotient: it decides validity and gets no gradient.  The arithmetic is planes_math.h's.
//
// One lane per pixel, 256-lane workgroups over the flat image; three coalesced 4-byte loads of `normal` and one each of
// `distance` and `alpha`, one to five coalesced stores.  The backward scales the saved unit gradients by the upstream
// map: a gather onto the lane's own pixel.  No LDS, no atomics: the same bits from run to run.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "planes_math.h"

namespace gsr {

namespace {

constexpr int PD_THREADS = 256;

template <bool GRAD>
__global__ __launch_bounds__(PD_THREADS) void plane_depth_fwd_kernel(const float* __restrict__ normal,
                                                                     const float* __restrict__ distance,
                                                                     const float* __restrict__ alpha, int H, int W,
                                                                     PlaneDepthCamera cam, float* __restrict__ z,
                                                                     float* __restrict__ dz_ddistance,
                                                                     float* __restrict__ dz_dnormal) {
  const size_t plane = (size_t)W * (size_t)H;
  const size_t pix = (size_t)blockIdx.x * PD_THREADS + threadIdx.x;
  if (pix >= plane) return;
  const int y = (int)(pix / (size_t)W), x = (int)(pix - (size_t)y * (size_t)W);
  const float N[3] = {normal[pix], normal[plane + pix], normal[2 * plane + pix]};
  float zz, gd, gn[3];
  plane_depth_pixel(N, distance[pix], alpha[pix], x, y, cam, &zz, &gd, gn);
  z[pix] = zz;
  if constexpr (GRAD) {
    dz_ddistance[pix] = gd;
#pragma unroll
    for (int a = 0; a < 3; ++a) dz_dnormal[a * plane + pix] = gn[a];
  }
}

__global__ __launch_bounds__(PD_THREADS) void plane_depth_bwd_kernel(const float* __restrict__ dL_dz,
                                                                     const float* __restrict__ dz_ddistance,
                                                                     const float* __restrict__ dz_dnormal, size_t plane,
                                                                     float* __restrict__ dL_ddistance,
                                                                     float* __restrict__ dL_dnormal) {
  const size_t pix = (size_t)blockIdx.x * PD_THREADS + threadIdx.x;
  if (pix >= plane) return;
  const float g = dL_dz[pix];
  // a pixel that is not valid has zero unit gradients: it stays zero whatever the upstream holds there (a NaN too)
  const float ud = dz_ddistance[pix];
  dL_ddistance[pix] = ud == 0.0f ? 0.0f : g * ud;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float un = dz_dnormal[a * plane + pix];
    dL_dnormal[a * plane + pix] = un == 0.0f ? 0.0f : g * un;
  }
}

// image_shape_ok bounds H W by 2^28, so the block count fits an unsigned and the launch stays below 2^32 work-items
unsigned plane_depth_blocks(int32_t H, int32_t W) {
  return (unsigned)(((size_t)H * (size_t)W + PD_THREADS - 1) / PD_THREADS);
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

int gsr_plane_depth_fwd(const float* normal, const float* distance, const float* alpha, int32_t H, int32_t W,
                        float tanfovx, float tanfovy, float alpha_min, float min_cos, float* z, float* dz_ddistance,
                        float* dz_dnormal, void* stream) {
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "bad image shape");
  if (!(tanfovx > 0.0f) || !(tanfovy > 0.0f) || tanfovx > 3.0e38f || tanfovy > 3.0e38f)
    return fail(GSR_E_BADARG, "tanfovx and tanfovy must be positive and finite");
  if (!(alpha_min > 0.0f) || !(alpha_min <= 1.0f)) return fail(GSR_E_BADARG, "alpha_min must lie in (0, 1]");
  if (!(min_cos >= 0.0f) || !(min_cos < 1.0f)) return fail(GSR_E_BADARG, "min_cos must lie in [0, 1)");
  if (!normal || !distance || !alpha || !z) return fail(GSR_E_BADARG, "NULL argument");
  if ((dz_ddistance != nullptr) != (dz_dnormal != nullptr))
    return fail(GSR_E_BADARG, "give both unit-gradient pointers or neither");
  if (!aligned({normal, distance, alpha, z, dz_ddistance, dz_dnormal}, 3u))
    return fail(GSR_E_ALIGN, "maps must be 4-byte aligned");
  // one double division and one cast each, as gsr_normal_consistency_fwd_bwd builds them
  const float fx = (float)((double)W / (2.0 * (double)tanfovx)), fy = (float)((double)H / (2.0 * (double)tanfovy));
  const PlaneDepthCamera cam = {fx, fy, (float)(((double)W - 1.0) * 0.5), (float)(((double)H - 1.0) * 0.5), alpha_min,
                                min_cos};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(plane_depth_blocks(H, W)), block(PD_THREADS);
  if (dz_ddistance)
    hipLaunchKernelGGL(plane_depth_fwd_kernel<true>, grid, block, 0, s, normal, distance, alpha, H, W, cam, z,
                       dz_ddistance, dz_dnormal);
  else
    hipLaunchKernelGGL(plane_depth_fwd_kernel<false>, grid, block, 0, s, normal, distance, alpha, H, W, cam, z,
                       dz_ddistance, dz_dnormal);
  return check(false, s, "plane_depth_fwd");
}

int gsr_plane_depth_bwd(const float* dL_dz, const float* dz_ddistance, const float* dz_dnormal, int32_t H, int32_t W,
                        float* dL_ddistance, float* dL_dnormal, void* stream) {
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "bad image shape");
  if (!dL_dz || !dz_ddistance || !dz_dnormal || !dL_ddistance || !dL_dnormal) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({dL_dz, dz_ddistance, dz_dnormal, dL_ddistance, dL_dnormal}, 3u))
    return fail(GSR_E_ALIGN, "maps must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(plane_depth_bwd_kernel, dim3(plane_depth_blocks(H, W)), dim3(PD_THREADS), 0, s, dL_dz, dz_ddistance,
                     dz_dnormal, (size_t)H * (size_t)W, dL_ddistance, dL_dnormal);
  return check(false, s, "plane_depth_bwd");
}

}  // extern "C"

// Multi-view photometric (NCC) loss of a (reference, source) pair, value and the gradients to the reference's depth and
// normal maps in one launch (include/gsr.h, ABI v36; mvs.multi_view_ncc_loss): the photometric half of
// PGSR's multi-view term.  A (2R+1)^2 patch of the reference's grey image is carried into the source's grey image by the
// homography of the pixel's rendered plane (depth + normal), and one minus the normalised cross-correlation of the two
// patches is penalised.
//
// Conventions of mvs.hip: depth 0 means none, cx = (W - 1) / 2, row-vector matrices, A = ref_to_src, one GsrMvsSource row.
// r(q) = ((qx - cx) / fx, (qy - cy) / fy, 1).  Per reference pixel p = (px, py) with d = ref_depth[p] > 0 and
// N = ref_normal[:, p], float32, every operation rounded on its own (the unit is built with -ffp-contract=off):
//   patch    px - R >= 0, px + R <= W - 1, py - R >= 0, py + R <= H - 1
//   plane    (rx, ry, 1) = r(p)     nn = (Nx Nx + Ny Ny) + Nz Nz     s = (Nx rx + Ny ry) + Nz     rr = (rx rx + ry ry) + 1
//            gate nn > 1e-12 and |s| >= min_cos sqrtf(nn rr)
//            ds = d s      m = (Nx / ds, Ny / ds, Nz / ds)            (m . (d r(p)) = 1; of degree 0 in |N|)
//   weight   the round trip of mvs_geom.h (the bits of mvs.hip); every gate passes; phi = sqrtf(du du + dv dv) < pix_max;
//            w = expf(-phi), a constant for the gradients
//   tap(q)   (qx', qy', 1) = r(q)      k = (mx qx' + my qy') + mz, gate k > 0
//            Yc = ((qx' A[c] + qy' A[4 + c]) + A[8 + c]) + k A[12 + c]  for c = x, y, z (0, 1, 2), gate Yz > 0
//            ix = Yx / Yz, iy = Yy / Yz      u = fxs ix + cxs, v = fys iy + cys      x0 = floorf(u), y0 = floorf(v)
//            gate x0 >= 0, x0 + 1 <= Ws - 1, y0 >= 0, y0 + 1 <= Hs - 1 (a NaN fails)      ax = u - x0, ay = v - y0
//            top = s00 (1 - ax) + s10 ax      bot = s01 (1 - ax) + s11 ax      S = top (1 - ay) + bot ay
//            Sx = (s10 - s00) (1 - ay) + (s11 - s01) ay      Sy = bot - top
//            hu = (fxs (A[12] - ix A[14])) / Yz      hv = (fys (A[13] - iy A[14])) / Yz      g = Sx hu + Sy hv
//            (d S / d m = g r(q): k is linear in m and Y in k)
//   sums     the centre tap first: Sc = S(p), Rp = gray[p].  Then q = p + (i, j), j = -R..R outer, i = -R..R inner; any
//            tap failing a gate makes the pixel invalid.  a = gray[q] - Rp, b = S(q) - Sc (the sums below are invariant
//            under both shifts, so holding Sc constant is exact), (gx, gy, gz) = (g qx', g qy', g), each += in tap order:
//            sR += a, sS += b, sRR += a a, sSS += b b, sRS += a b,
//            D_c += g_c, SD_c += b g_c, RD_c += a g_c  for c = x, y, z
//   ncc      T = (2R+1)^2      cross = sRS - (sR sS) / T      vr = sRR - (sR sR) / T      vs = sSS - (sS sS) / T
//            den = vr vs + 1e-8      cc = (cross cross) / den      t = 1 - cc      ncc = fminf(fmaxf(t, 0), 2)
//            counted iff ncc < ncc_max      e = w ncc
//   loss     raw = sum_counted e      n = the number of counted pixels      loss = raw / max(n, 1)
//   backward of raw, per counted pixel with 0 < t < 2 (the clamp's flat parts, every gate and the ncc_max test carry none):
//            dcross_c = RD_c - (sR D_c) / T      dvs_c = 2 (SD_c - (sS D_c) / T)
//            dcc_c = ((2 cross) dcross_c) / den - (((cross cross) vr) dvs_c) / (den den)      G_c = -(w dcc_c)
//            gm = (Gx mx + Gy my) + Gz mz
//            grad_depth[p] = -(gm / d)      grad_normal[c, p] = G_c / ds - (gm r(p)_c) / s
// Both are unit gradients of raw; the caller scales them by upstream / max(n, 1).
//
// Launch: 256-lane workgroups, one lane per pixel of a 64 x 4 tile (pixels == NULL) or per entry of the list of flat
// pixel indices; no grid-stride loop, nothing waits on another workgroup.  The source row is the same for every lane: its
// 152 bytes arrive through scalar loads.  One runtime loop over the taps carries the five sums and the nine forward-mode
// accumulators; there is no second walk and no per-tap storage.  Every gradient is a gather onto the lane's own pixel: no
// atomics, all outputs the same bits from run to run.  Dense mode writes every pixel (zero where not counted); with a
// list the entry point zeroes both maps on the stream first and the lanes write their own pixels only (duplicate indices
// are the caller's error: the lanes would race, with equal values).  The value: e in double, one (double, uint32) pair
// per workgroup in the workspace, a one-block finish kernel behind it, every sum in the fixed order of ordered_sum.h.
// LDS: the eight reduction slots only.
//
// Safety.  A list entry outside [0, H W) is skipped before anything is addressed with it.  Reference taps lie inside the
// image by the patch gate; source taps are behind the footprint test formed from the row's own width and height; the
// source's grey image must be of that size (the wrapper checks it against the camera).  The entry point refuses images
// above 2^28 pixels and launches of 2^32 work-items or more.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "mvs_geom.h"
#include "ordered_sum.h"

namespace gsr {

namespace {

constexpr int NCC_FIN_THREADS = 1024;

struct NccTap {
  float S, g;
};

// One tap of the header comment: the source's grey value where the plane m carries the reference ray (qx, qy, 1), and g
// with d S / d m = g (qx, qy, 1).  false when a gate fails.  Every gather is behind the footprint test.
__device__ inline bool ncc_tap(const GsrMvsSource& src, const float* __restrict__ src_gray, float cxs, float cys, float Ws1,
                               float Hs1, float mx, float my, float mz, float qx, float qy, NccTap& t) {
  const float* __restrict__ A = src.ref_to_src;
  const float k = (mx * qx + my * qy) + mz;
  if (!(k > 0.0f)) return false;
  const float Yx = ((qx * A[0] + qy * A[4]) + A[8]) + k * A[12];
  const float Yy = ((qx * A[1] + qy * A[5]) + A[9]) + k * A[13];
  const float Yz = ((qx * A[2] + qy * A[6]) + A[10]) + k * A[14];
  if (!(Yz > 0.0f)) return false;
  const float ix = Yx / Yz, iy = Yy / Yz;
  const float u = src.fx * ix + cxs, v = src.fy * iy + cys;
  const float x0 = floorf(u), y0 = floorf(v);
  if (!(x0 >= 0.0f && x0 + 1.0f <= Ws1 && y0 >= 0.0f && y0 + 1.0f <= Hs1)) return false;       // a NaN fails
  const float ax = u - x0, ay = v - y0;
  const float* __restrict__ row0 = src_gray + ((size_t)(int)y0 * (size_t)src.width + (size_t)(int)x0);
  const float* __restrict__ row1 = row0 + src.width;
  const float s00 = row0[0], s10 = row0[1], s01 = row1[0], s11 = row1[1];
  const float bx = 1.0f - ax, by = 1.0f - ay;
  const float top = s00 * bx + s10 * ax, bot = s01 * bx + s11 * ax;
  t.S = top * by + bot * ay;
  const float Sx = (s10 - s00) * by + (s11 - s01) * ay, Sy = bot - top;
  const float hu = (src.fx * (A[12] - ix * A[14])) / Yz, hv = (src.fy * (A[13] - iy * A[14])) / Yz;
  t.g = Sx * hu + Sy * hv;
  return true;
}

__global__ __launch_bounds__(MVS_BLOCK) void mvs_ncc_loss_kernel(
    const float* __restrict__ depth, const float* __restrict__ normal, const float* __restrict__ gray, int H, int W, float fx,
    float fy, const GsrMvsSource* __restrict__ source, const float* __restrict__ src_gray, const int* __restrict__ pixels,
    int n_pixels, int R, float pix_max, float ncc_max, float min_cos, unsigned xtiles, float* __restrict__ grad_depth,
    float* __restrict__ grad_normal, double* __restrict__ part_sum, uint32_t* __restrict__ part_n) {
  __shared__ PairSlots<double, MVS_BLOCK / WAVE> red;
  const int HW = H * W;                                                  // at most 2^28
  int px, py;
  bool in;
  if (pixels) {
    const unsigned idx = blockIdx.x * (unsigned)MVS_BLOCK + threadIdx.x;
    int pix = -1;
    if (idx < (unsigned)n_pixels) pix = pixels[idx];
    in = pix >= 0 && pix < HW;                                           // an entry outside the image is skipped
    py = in ? pix / W : 0;
    px = in ? pix - py * W : 0;
  } else {
    const unsigned tx = blockIdx.x % xtiles, ty = blockIdx.x / xtiles;
    px = (int)(tx * MVS_TILE_X + threadIdx.x % MVS_TILE_X);
    py = (int)(ty * MVS_TILE_Y + threadIdx.x / MVS_TILE_X);
    in = px < W && py < H;
  }
  const int pix = py * W + px;                                           // used under `in` only
  const GsrMvsSource& src = source[0];                                   // uniform across the grid: scalar loads
  const float d = in ? depth[pix] : 0.0f;
  bool counted = false;
  float e = 0.0f, g_d = 0.0f, g_nx = 0.0f, g_ny = 0.0f, g_nz = 0.0f;
  if (d > 0.0f && px - R >= 0 && px + R <= W - 1 && py - R >= 0 && py + R <= H - 1) {
    const float fpx = (float)px, fpy = (float)py;
    const float cx = ((float)W - 1.0f) * 0.5f, cy = ((float)H - 1.0f) * 0.5f;
    const float rx = (fpx - cx) / fx, ry = (fpy - cy) / fy;
    const float Nx = normal[pix], Ny = normal[(size_t)HW + pix], Nz = normal[2 * (size_t)HW + pix];
    const float nn = (Nx * Nx + Ny * Ny) + Nz * Nz;
    const float s = (Nx * rx + Ny * ry) + Nz;
    const float rr = (rx * rx + ry * ry) + 1.0f;
    MvsTrip t;
    if (nn > 1e-12f && fabsf(s) >= min_cos * sqrtf(nn * rr) &&
        mvs_round_trip(src, fpx, fpy, cx, cy, fx, fy, ((fpx - cx) * d) / fx, ((fpy - cy) * d) / fy, d, t)) {
      const float phi = sqrtf(t.du * t.du + t.dv * t.dv);
      if (phi < pix_max) {
        const float w = expf(-phi);
        const float ds = d * s;
        const float mx = Nx / ds, my = Ny / ds, mz = Nz / ds;
        const float Ws1 = (float)src.width - 1.0f, Hs1 = (float)src.height - 1.0f;
        NccTap tap;
        bool ok = ncc_tap(src, src_gray, t.cxs, t.cys, Ws1, Hs1, mx, my, mz, rx, ry, tap);
        const float Sc = tap.S, Rp = gray[pix];
        float sR = 0.0f, sS = 0.0f, sRR = 0.0f, sSS = 0.0f, sRS = 0.0f;
        float Dx = 0.0f, Dy = 0.0f, Dz = 0.0f, SDx = 0.0f, SDy = 0.0f, SDz = 0.0f, RDx = 0.0f, RDy = 0.0f, RDz = 0.0f;
        const int side = 2 * R + 1, taps = side * side;
#pragma unroll 1
        for (int n = 0; ok && n < taps; ++n) {
          const int j = n / side - R, i = n % side - R;
          const float qx = ((float)(px + i) - cx) / fx, qy = ((float)(py + j) - cy) / fy;
          ok = ncc_tap(src, src_gray, t.cxs, t.cys, Ws1, Hs1, mx, my, mz, qx, qy, tap);
          if (ok) {
            const float a = gray[pix + j * W + i] - Rp, b = tap.S - Sc;
            const float gx = tap.g * qx, gy = tap.g * qy, gz = tap.g;
            sR += a; sS += b; sRR += a * a; sSS += b * b; sRS += a * b;
            Dx += gx; Dy += gy; Dz += gz;
            SDx += b * gx; SDy += b * gy; SDz += b * gz;
            RDx += a * gx; RDy += a * gy; RDz += a * gz;
          }
        }
        if (ok) {
          const float T = (float)taps;
          const float cross = sRS - (sR * sS) / T, vr = sRR - (sR * sR) / T, vs = sSS - (sS * sS) / T;
          const float den = vr * vs + 1e-8f;
          const float cc = (cross * cross) / den;
          const float tt = 1.0f - cc;
          const float ncc = fminf(fmaxf(tt, 0.0f), 2.0f);
          counted = ncc < ncc_max;
          if (counted) {
            e = w * ncc;
            if ((grad_depth || grad_normal) && tt > 0.0f && tt < 2.0f) {
              const float c2 = 2.0f * cross, q2 = (cross * cross) * vr, den2 = den * den;
              const float Gx = -(w * ((c2 * (RDx - (sR * Dx) / T)) / den - (q2 * (2.0f * (SDx - (sS * Dx) / T))) / den2));
              const float Gy = -(w * ((c2 * (RDy - (sR * Dy) / T)) / den - (q2 * (2.0f * (SDy - (sS * Dy) / T))) / den2));
              const float Gz = -(w * ((c2 * (RDz - (sR * Dz) / T)) / den - (q2 * (2.0f * (SDz - (sS * Dz) / T))) / den2));
              const float gm = (Gx * mx + Gy * my) + Gz * mz;
              g_d = -(gm / d);
              g_nx = Gx / ds - (gm * rx) / s;
              g_ny = Gy / ds - (gm * ry) / s;
              g_nz = Gz / ds - gm / s;
            }
          }
        }
      }
    }
  }
  if (in) {
    if (grad_depth) grad_depth[pix] = g_d;
    if (grad_normal) {
      grad_normal[pix] = g_nx;
      grad_normal[(size_t)HW + pix] = g_ny;
      grad_normal[2 * (size_t)HW + pix] = g_nz;
    }
  }

  // the workgroup's partial and count (ordered_sum.h)
  double ts = (double)e;
  uint32_t tn = counted ? 1u : 0u;
  ordered_pair_sum(ts, tn, red);
  if (threadIdx.x == 0) {
    part_sum[blockIdx.x] = ts;
    part_n[blockIdx.x] = tn;
  }
}

// One block: the pairs in the fixed order of ordered_pair_finish.
// record = {float raw / max(n, 1), uint32 n, float raw, 0}: written, not accumulated.  nblocks may be 0 (an empty list).
__global__ __launch_bounds__(NCC_FIN_THREADS) void mvs_ncc_loss_finish_kernel(const double* __restrict__ part_sum,
                                                                              const uint32_t* __restrict__ part_n,
                                                                              unsigned nblocks, float* __restrict__ record) {
  __shared__ PairSlots<double, NCC_FIN_THREADS / WAVE> red;
  double ts;
  uint32_t tn;
  ordered_pair_finish(part_sum, part_n, nblocks, ts, tn, red);
  if (threadIdx.x != 0) return;
  record[0] = (float)(ts / (double)(tn > 0u ? tn : 1u));
  reinterpret_cast<uint32_t*>(record)[1] = tn;
  record[2] = (float)ts;
  record[3] = 0.0f;
}

// The workgroups of a call: of the 64 x 4 tiles (n_pixels == 0) or of the list.  false when the image or n_pixels is
// refused or the launch would reach 2^32 work-items.
bool mvs_ncc_blocks(int32_t H, int32_t W, int32_t n_pixels, unsigned* xtiles, unsigned* blocks) {
  if (!image_shape_ok(H, W)) return false;
  if (n_pixels < 0 || (long long)n_pixels > (long long)H * (long long)W) return false;
  const unsigned long long xt = ((unsigned long long)W + MVS_TILE_X - 1) / MVS_TILE_X;
  const unsigned long long yt = ((unsigned long long)H + MVS_TILE_Y - 1) / MVS_TILE_Y;
  if (xt * yt * MVS_BLOCK >= (1ull << 32)) return false;                 // HIP's bound on the work-items of a launch
  *xtiles = (unsigned)xt;
  *blocks = n_pixels > 0 ? (unsigned)(((unsigned long long)n_pixels + MVS_BLOCK - 1) / MVS_BLOCK) : (unsigned)(xt * yt);
  return true;
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_mvs_ncc_loss_workspace_bytes(int32_t H, int32_t W, int32_t n_pixels) {
  unsigned xtiles, blocks;
  if (!mvs_ncc_blocks(H, W, n_pixels, &xtiles, &blocks)) return 0;
  return (size_t)blocks * (sizeof(double) + sizeof(uint32_t));
}

int gsr_mvs_ncc_loss_fwd_bwd(const float* ref_depth, const float* ref_normal, const float* ref_gray, int32_t H, int32_t W,
                             float fx, float fy, const GsrMvsSource* source, const float* src_gray, const int32_t* pixels,
                             int32_t n_pixels, int32_t patch_radius, float pix_max, float ncc_max, float min_cos,
                             float* record, float* grad_depth, float* grad_normal, void* workspace, void* stream) {
  if (!ref_depth || !ref_normal || !ref_gray || !source || !src_gray || !record || !workspace)
    return fail(GSR_E_BADARG, "ref_depth / ref_normal / ref_gray / source / src_gray / record / workspace is NULL");
  unsigned xtiles, blocks;
  if (!mvs_ncc_blocks(H, W, pixels ? n_pixels : 0, &xtiles, &blocks) || n_pixels < 0 ||
      (long long)n_pixels > (long long)H * (long long)W)
    return fail(GSR_E_BADARG, "H and W must be positive, H * W at most 2^28, the launch below 2^32 work-items and "
                              "0 <= n_pixels <= H * W");
  if (patch_radius < 1 || patch_radius > 4) return fail(GSR_E_BADARG, "patch_radius must lie in 1..4");
  if (!mvs_positive_finite(fx) || !mvs_positive_finite(fy)) return fail(GSR_E_BADARG, "fx and fy must be positive and finite");
  if (!mvs_positive_finite(pix_max)) return fail(GSR_E_BADARG, "pix_max must be positive and finite");
  if (!(ncc_max > 0.0f && ncc_max <= 2.0f)) return fail(GSR_E_BADARG, "ncc_max must lie in (0, 2]");
  if (!(min_cos >= 0.0f && min_cos < 1.0f)) return fail(GSR_E_BADARG, "min_cos must lie in [0, 1)");
  if (!aligned({ref_depth, ref_normal, ref_gray, src_gray, pixels, record, grad_depth, grad_normal}, 3u))
    return fail(GSR_E_ALIGN, "the maps, the images, pixels, record and the gradients must be 4-byte aligned");
  if (!aligned({source, workspace}, 7u)) return fail(GSR_E_ALIGN, "the table row and the workspace must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t hw = (size_t)H * (size_t)W;
  if (pixels) {                                                          // the lanes write the listed pixels only
    if (grad_depth) GSR_HIP(hipMemsetAsync(grad_depth, 0, hw * sizeof(float), s));
    if (grad_normal) GSR_HIP(hipMemsetAsync(grad_normal, 0, 3 * hw * sizeof(float), s));
    if (n_pixels == 0) blocks = 0;
  }
  double* part_sum = static_cast<double*>(workspace);
  uint32_t* part_n = reinterpret_cast<uint32_t*>(part_sum + blocks);
  if (blocks > 0)
    hipLaunchKernelGGL(mvs_ncc_loss_kernel, dim3(blocks), dim3(MVS_BLOCK), 0, s, ref_depth, ref_normal, ref_gray, (int)H,
                       (int)W, fx, fy, source, src_gray, pixels, (int)n_pixels, (int)patch_radius, pix_max, ncc_max, min_cos,
                       xtiles, grad_depth, grad_normal, part_sum, part_n);
  hipLaunchKernelGGL(mvs_ncc_loss_finish_kernel, dim3(1), dim3(NCC_FIN_THREADS), 0, s, part_sum, part_n, blocks, record);
  return check(false, s, "mvs_ncc_loss_fwd_bwd");
}

}  // extern "C"

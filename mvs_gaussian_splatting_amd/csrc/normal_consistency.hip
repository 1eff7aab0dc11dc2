// Depth-normal consistency loss of a rendered frame, value and gradients in one launch (include/gsr.h, ABI v28;
// DESIGN.md §7.15).  Inputs depth = sum w z, alpha = sum w ([H,W] each) and normal = sum w n ([3,H,W], un-normalised).
// Per pixel, float32, every operation rounded on its own (the unit is built with -ffp-contract=off):
//     covered(q) = alpha(q) >= alpha_min          d(q) = depth(q) / alpha(q)
//     P(q)  = ((d (x - cx)) / fx, (d (y - cy)) / fy, d)           cx = (W - 1) / 2, cy = (H - 1) / 2, fx, fy from the host
//     tx = P(x+1,y) - P(x-1,y)    ty = P(x,y+1) - P(x,y-1)    c = ty x tx    s = (c0 c0 + c1 c1) + c2 c2    r = sqrt(s)
//     valid(q) = interior, q and its four axis neighbours covered, s finite and s > 1e-20
//     n_d = c / r  (faces the camera: a fronto-parallel plane gives (0,0,-1))      dot = (N0 n0 + N1 n1) + N2 n2
//     e = alpha - dot                                  loss = sum_valid e / (H W)
// Backward, validity a decision without gradient.  With k = 1 / (H W):
//     g_c  = (((dot n_d) - N) / r) k                   d(-N . c/|c|)/dc = -(N - (N . n_d) n_d) / |c|
//     G_tx = g_c x ty,  G_ty = tx x g_c                dL/dtx, dL/dty of the stencil centred on q
//     dL/dP(q) = G_tx(x-1,y) - G_tx(x+1,y) + G_ty(x,y-1) - G_ty(x,y+1)         a gather over the four neighbours' stencils
//     g_d  = (dL/dP0 ((x - cx) / fx) + dL/dP1 ((y - cy) / fy)) + dL/dP2
//     dL/ddepth = g_d / alpha      dL/dalpha = valid k - (g_d d) / alpha      dL/dnormal = -(n_d k) on valid pixels
// and zeros on a pixel that is not covered (none of its neighbours is valid then).
//
// One kernel, the single-kernel form of the two the issue allows: 16x16-pixel workgroups of 256 lanes, one lane per
// pixel.  d and the covered bit of the 20x20 pixels around the tile are staged in LDS (a two-pixel halo: the stencils of
// the tile's one-pixel ring read one pixel further).  Every lane evaluates the stencil of its own pixel, lanes 0..67
// also one of the 68 ring pixels (1.27 stencils per pixel instead of 5), and G_tx, G_ty of the 18x18 pixels go to LDS;
// after one barrier every lane gathers its four neighbours' entries.  `normal` is read straight from memory: every
// stencil reads its own pixel's only, so LDS would not save a byte.  No atomics; nothing waits on another workgroup.
// The loss: e in double, one (double sum, uint32 count) pair per workgroup in the workspace; a one-block kernel behind
// it adds the pairs and writes the record.  Every sum in the fixed order of ordered_sum.h.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "ordered_sum.h"

namespace gsr {

namespace {

constexpr int NC_T = 16;                  // tile edge
constexpr int NC_D = NC_T + 4;            // staged depth: two-pixel halo
constexpr int NC_G = NC_T + 2;            // stencils evaluated: one-pixel ring
constexpr int NC_RING = NC_G * NC_G - NC_T * NC_T;
constexpr int NC_FIN_THREADS = 1024;

struct NcCamera {
  float fx, fy, cx, cy, alpha_min, inv_hw;
};

struct NcStencil {
  bool valid;
  float n[3];      // n_d
  float dot;       // N . n_d
  float gtx[3], gty[3];
};

// The stencil centred on image pixel (x, y) = LDS position (lx, ly) of the staged depth, 1 <= lx, ly <= NC_D - 2.
template <bool GRAD>
__device__ inline void nc_stencil(const float (&sd)[NC_D][NC_D + 1], const uint8_t (&sc)[NC_D][NC_D], int lx, int ly,
                                  int x, int y, int W, int H, const NcCamera& cam, const float* __restrict__ normal,
                                  NcStencil& o) {
  o.valid = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) o.n[a] = o.gtx[a] = o.gty[a] = 0.0f;
  o.dot = 0.0f;
  if (x < 1 || y < 1 || x > W - 2 || y > H - 2) return;
  if (!(sc[ly][lx] && sc[ly][lx - 1] && sc[ly][lx + 1] && sc[ly - 1][lx] && sc[ly + 1][lx])) return;
  const float dl = sd[ly][lx - 1], dr = sd[ly][lx + 1], du = sd[ly - 1][lx], dd = sd[ly + 1][lx];
  const float fxc = (float)x - cam.cx, fyc = (float)y - cam.cy;
  const float tx[3] = {(dr * ((float)(x + 1) - cam.cx)) / cam.fx - (dl * ((float)(x - 1) - cam.cx)) / cam.fx,
                       (dr * fyc) / cam.fy - (dl * fyc) / cam.fy, dr - dl};
  const float ty[3] = {(dd * fxc) / cam.fx - (du * fxc) / cam.fx,
                       (dd * ((float)(y + 1) - cam.cy)) / cam.fy - (du * ((float)(y - 1) - cam.cy)) / cam.fy, dd - du};
  const float c[3] = {ty[1] * tx[2] - ty[2] * tx[1], ty[2] * tx[0] - ty[0] * tx[2], ty[0] * tx[1] - ty[1] * tx[0]};
  const float s = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
  if (!(s > 1e-20f) || !(s <= 3.402823466e38f)) return;                 // NaN fails the first test, +inf the second
  const float r = sqrtf(s);
  const size_t plane = (size_t)W * (size_t)H, pix = (size_t)y * (size_t)W + (size_t)x;
  const float N[3] = {normal[pix], normal[plane + pix], normal[2 * plane + pix]};
  o.valid = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) o.n[a] = c[a] / r;
  o.dot = (N[0] * o.n[0] + N[1] * o.n[1]) + N[2] * o.n[2];
  if constexpr (GRAD) {
    float g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] = ((o.dot * o.n[a] - N[a]) / r) * cam.inv_hw;
    o.gtx[0] = g[1] * ty[2] - g[2] * ty[1];
    o.gtx[1] = g[2] * ty[0] - g[0] * ty[2];
    o.gtx[2] = g[0] * ty[1] - g[1] * ty[0];
    o.gty[0] = tx[1] * g[2] - tx[2] * g[1];
    o.gty[1] = tx[2] * g[0] - tx[0] * g[2];
    o.gty[2] = tx[0] * g[1] - tx[1] * g[0];
  }
}

template <bool GRAD>
__global__ __launch_bounds__(NC_T* NC_T) void normal_consistency_kernel(
    const float* __restrict__ depth, const float* __restrict__ alpha, const float* __restrict__ normal, int H, int W,
    NcCamera cam, unsigned xtiles, float* __restrict__ dL_ddepth, float* __restrict__ dL_dalpha,
    float* __restrict__ dL_dnormal, float* __restrict__ depth_normal, double* __restrict__ part_sum,
    uint32_t* __restrict__ part_n) {
  __shared__ float sd[NC_D][NC_D + 1];
  __shared__ uint8_t sc[NC_D][NC_D];
  __shared__ float sg[GRAD ? 6 : 1][NC_G][NC_G + 1];
  __shared__ PairSlots<double, NC_T * NC_T / WAVE> red;
  const int tid = threadIdx.x, lx0 = tid & (NC_T - 1), ly0 = tid / NC_T;
  const int x0 = (int)(blockIdx.x % xtiles) * NC_T, y0 = (int)(blockIdx.x / xtiles) * NC_T;
  const size_t plane = (size_t)W * (size_t)H;

  for (int i = tid; i < NC_D * NC_D; i += NC_T * NC_T) {
    const int hy = i / NC_D, hx = i - hy * NC_D;
    const int x = x0 + hx - 2, y = y0 + hy - 2;
    float d = 0.0f;
    bool cov = false;
    if (x >= 0 && x < W && y >= 0 && y < H) {
      const size_t pix = (size_t)y * (size_t)W + (size_t)x;
      const float a = alpha[pix];
      cov = a >= cam.alpha_min;
      if (cov) d = depth[pix] / a;
    }
    sd[hy][hx] = d;
    sc[hy][hx] = cov ? 1 : 0;
  }
  __syncthreads();

  const int x = x0 + lx0, y = y0 + ly0;
  const bool in = x < W && y < H;
  NcStencil own;
  nc_stencil<GRAD>(sd, sc, lx0 + 2, ly0 + 2, x, y, W, H, cam, normal, own);
  const size_t pix = (size_t)y * (size_t)W + (size_t)x;          // used under `in` only
  float a_own = 0.0f;
  double e = 0.0;
  if (own.valid) {                                               // valid implies in
    a_own = alpha[pix];
    e = (double)(a_own - own.dot);
  }
  if (in && depth_normal) {
#pragma unroll
    for (int a = 0; a < 3; ++a) depth_normal[a * plane + pix] = own.n[a];
  }

  // the workgroup's loss partial and count (ordered_sum.h, the split form: the barrier below is the kernel's one)
  ordered_pair_stage(e, own.valid ? 1u : 0u, red);

  if constexpr (GRAD) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      sg[a][ly0 + 1][lx0 + 1] = own.gtx[a];
      sg[3 + a][ly0 + 1][lx0 + 1] = own.gty[a];
    }
    if (tid < NC_RING) {
      int gx, gy;
      if (tid < NC_G) { gx = tid; gy = 0; }
      else if (tid < 2 * NC_G) { gx = tid - NC_G; gy = NC_G - 1; }
      else if (tid < 2 * NC_G + NC_T) { gx = 0; gy = tid - 2 * NC_G + 1; }
      else { gx = NC_G - 1; gy = tid - 2 * NC_G - NC_T + 1; }
      NcStencil ring;
      nc_stencil<true>(sd, sc, gx + 1, gy + 1, x0 + gx - 1, y0 + gy - 1, W, H, cam, normal, ring);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        sg[a][gy][gx] = ring.gtx[a];
        sg[3 + a][gy][gx] = ring.gty[a];
      }
    }
  }
  __syncthreads();

  if (tid == 0) {
    double ts;
    uint32_t tn;
    ordered_pair_fold(red, ts, tn);
    part_sum[blockIdx.x] = ts;
    part_n[blockIdx.x] = tn;
  }

  if constexpr (GRAD) {
    if (!in) return;
    const int gx = lx0 + 1, gy = ly0 + 1;
    float gp[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
      gp[a] = ((sg[a][gy][gx - 1] - sg[a][gy][gx + 1]) + sg[3 + a][gy - 1][gx]) - sg[3 + a][gy + 1][gx];
    float g_depth = 0.0f, g_alpha = 0.0f;
    if (sc[ly0 + 2][lx0 + 2]) {
      const float ax = ((float)x - cam.cx) / cam.fx, ay = ((float)y - cam.cy) / cam.fy;
      const float gd = (gp[0] * ax + gp[1] * ay) + gp[2];
      const float a = own.valid ? a_own : alpha[pix];
      g_depth = gd / a;
      g_alpha = (own.valid ? cam.inv_hw : 0.0f) - (gd * sd[ly0 + 2][lx0 + 2]) / a;
    }
    dL_ddepth[pix] = g_depth;
    dL_dalpha[pix] = g_alpha;
#pragma unroll
    for (int a = 0; a < 3; ++a) dL_dnormal[a * plane + pix] = own.valid ? -(own.n[a] * cam.inv_hw) : 0.0f;
  }
}

// One block: the pairs in the fixed order of ordered_pair_finish.
// record = {float loss, uint32 n_valid, 0, 0}: written, not accumulated.
__global__ __launch_bounds__(NC_FIN_THREADS) void normal_consistency_finish_kernel(const double* __restrict__ part_sum,
                                                                                   const uint32_t* __restrict__ part_n,
                                                                                   unsigned nblocks, double inv_hw,
                                                                                   float* __restrict__ record) {
  __shared__ PairSlots<double, NC_FIN_THREADS / WAVE> red;
  double ts;
  uint32_t tn;
  ordered_pair_finish(part_sum, part_n, nblocks, ts, tn, red);
  if (threadIdx.x != 0) return;
  record[0] = (float)(ts * inv_hw);
  reinterpret_cast<uint32_t*>(record)[1] = tn;
  record[2] = 0.0f;
  record[3] = 0.0f;
}

// false when the launch would exceed 2^32 work-items
bool normal_consistency_blocks(int H, int W, unsigned* xtiles, unsigned* blocks) {
  if (H < 1 || W < 1) return false;
  const unsigned long long xt = ((unsigned long long)W + NC_T - 1) / NC_T, yt = ((unsigned long long)H + NC_T - 1) / NC_T;
  if (xt * yt * (NC_T * NC_T) >= (1ull << 32)) return false;             // HIP's bound on the work-items of a launch
  *xtiles = (unsigned)xt;
  *blocks = (unsigned)(xt * yt);
  return true;
}

// The three gradient pointers are all set or all nullptr (forward only); depth_normal may be nullptr
void launch_normal_consistency(const float* depth, const float* alpha, const float* normal, int H, int W, float fx,
                               float fy, float alpha_min, float* record, float* dL_ddepth, float* dL_dalpha,
                               float* dL_dnormal, float* depth_normal, void* workspace, hipStream_t s) {
  unsigned xtiles, blocks;
  if (!normal_consistency_blocks(H, W, &xtiles, &blocks)) return;
  const double inv_hw = 1.0 / ((double)H * (double)W);
  const NcCamera cam = {fx, fy, (float)(((double)W - 1.0) * 0.5), (float)(((double)H - 1.0) * 0.5), alpha_min,
                        (float)inv_hw};
  double* part_sum = static_cast<double*>(workspace);
  uint32_t* part_n = reinterpret_cast<uint32_t*>(part_sum + blocks);
  const dim3 grid(blocks), block(NC_T * NC_T);
  if (dL_ddepth)
    hipLaunchKernelGGL(normal_consistency_kernel<true>, grid, block, 0, s, depth, alpha, normal, H, W, cam, xtiles,
                       dL_ddepth, dL_dalpha, dL_dnormal, depth_normal, part_sum, part_n);
  else
    hipLaunchKernelGGL(normal_consistency_kernel<false>, grid, block, 0, s, depth, alpha, normal, H, W, cam, xtiles,
                       dL_ddepth, dL_dalpha, dL_dnormal, depth_normal, part_sum, part_n);
  hipLaunchKernelGGL(normal_consistency_finish_kernel, dim3(1), dim3(NC_FIN_THREADS), 0, s, part_sum, part_n, blocks,
                     inv_hw, record);
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_normal_consistency_workspace_bytes(int32_t H, int32_t W) {
  unsigned xtiles, blocks;
  if (!image_shape_ok(H, W) || !normal_consistency_blocks(H, W, &xtiles, &blocks)) return 0;
  return (size_t)blocks * (sizeof(double) + sizeof(uint32_t));
}
int gsr_normal_consistency_fwd_bwd(const float* depth, const float* alpha, const float* normal, int32_t H, int32_t W,
                                   float tanfovx, float tanfovy, float alpha_min, float* record, float* dL_ddepth,
                                   float* dL_dalpha, float* dL_dnormal, float* depth_normal, void* workspace,
                                   void* stream) {
  unsigned xtiles, blocks;
  if (!image_shape_ok(H, W) || !normal_consistency_blocks(H, W, &xtiles, &blocks))
    return fail(GSR_E_BADARG, "bad image shape");
  if (!(tanfovx > 0.0f) || !(tanfovy > 0.0f) || tanfovx > 3.0e38f || tanfovy > 3.0e38f)
    return fail(GSR_E_BADARG, "tanfovx and tanfovy must be positive and finite");
  if (!(alpha_min > 0.0f) || !(alpha_min <= 1.0f)) return fail(GSR_E_BADARG, "alpha_min must lie in (0, 1]");
  if (!depth || !alpha || !normal || !record || !workspace) return fail(GSR_E_BADARG, "NULL argument");
  const int ngrad = (dL_ddepth != nullptr) + (dL_dalpha != nullptr) + (dL_dnormal != nullptr);
  if (ngrad != 0 && ngrad != 3) return fail(GSR_E_BADARG, "give all three gradient pointers or none");
  if (!aligned({depth, alpha, normal, dL_ddepth, dL_dalpha, dL_dnormal, depth_normal}, 3u))
    return fail(GSR_E_ALIGN, "maps must be 4-byte aligned");
  if (!aligned({record}, 15u)) return fail(GSR_E_ALIGN, "the record must be 16-byte aligned");
  if (!aligned({workspace}, 7u)) return fail(GSR_E_ALIGN, "the workspace must be 8-byte aligned");
  // each focal length is one double division and one cast: nothing for -ffp-contract to fuse, so this file's flags
  // give the bits the default flags gave
  const float fx = (float)((double)W / (2.0 * (double)tanfovx)), fy = (float)((double)H / (2.0 * (double)tanfovy));
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_normal_consistency(depth, alpha, normal, H, W, fx, fy, alpha_min, record, dL_ddepth, dL_dalpha, dL_dnormal,
                            depth_normal, workspace, s);
  return check(false, s, "normal_consistency_fwd_bwd");
}

}  // extern "C"

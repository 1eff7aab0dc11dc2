// Per-image exposure compensation (include/gsr.h, ABI v23): upstream 3DGS's learnable 3x4 colour affine, applied to the
// rendered image before the loss.  Image x [3,H,W] in planes, exposure A [3,4] row-major in device memory; k is the
// input channel, c the output channel, p the pixel:
//
//   y[c,p]  = x[0,p]*A[0,c] + x[1,p]*A[1,c] + x[2,p]*A[2,c] + A[c,3]
//   dx[k,p] = A[k,0]*g[0,p] + A[k,1]*g[1,p] + A[k,2]*g[2,p]                     g = dL/dy
//   dA[k,c] = sum_p x[k,p]*g[c,p]      dA[c,3] = sum_p g[c,p]
//
//   * exposure_apply_fwd_kernel / exposure_apply_bwd_kernel: one pixel per lane with a grid stride; a wave reads and
//     writes 256 consecutive bytes of each plane.  The sums above are written left to right in float32 and the unit is
//     built with -ffp-contract=off, so with A = eye(3,4) the products by 1 and 0 and the sums with 0 leave y = x and
//     dx = g bit for bit (finite inputs; a -0 comes out as +0).
//   * dA: a lane keeps the 12 sums in double (operands converted before the multiply, so a product is exact), the
//     block adds them in the fixed order of ordered_sum.h and stores 12 doubles in its own slot of the workspace;
//     exposure_grad_finish_kernel (one block) adds the slots in a fixed order and rounds once to float32.  No atomics:
//     dA depends on H, W and the data only, and is the same bits from run to run.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "ordered_sum.h"

namespace gsr {

namespace {

constexpr int EXPOSURE_MAX_BLOCKS = 480;      // just under two 256-lane blocks per CU; 30 slots per finish stripe
constexpr int EXP_THREADS = 256;
constexpr int EXP_WAVES = EXP_THREADS / WAVE;
constexpr int EXP_TERMS = 12;                                    // dA[k][c] at 4 k + c, as A is laid out
constexpr int EXP_FIN_THREADS = 256, EXP_FIN_STRIPES = EXP_FIN_THREADS / 16;

__global__ __launch_bounds__(EXP_THREADS) void exposure_apply_fwd_kernel(const float* __restrict__ x,
                                                                         const float* __restrict__ A, size_t pixels,
                                                                         float* __restrict__ y) {
  float a[EXP_TERMS];
#pragma unroll
  for (int i = 0; i < EXP_TERMS; ++i) a[i] = A[i];
  const size_t stride = (size_t)gridDim.x * EXP_THREADS;
  for (size_t p = (size_t)blockIdx.x * EXP_THREADS + threadIdx.x; p < pixels; p += stride) {
    const float x0 = x[p], x1 = x[pixels + p], x2 = x[2 * pixels + p];
#pragma unroll
    for (int c = 0; c < 3; ++c) y[c * pixels + p] = x0 * a[c] + x1 * a[4 + c] + x2 * a[8 + c] + a[4 * c + 3];
  }
}

// DX: dx is written.  DA: the block leaves its 12 sums in slots[blockIdx.x * 12 ..].
template <bool DX, bool DA>
__global__ __launch_bounds__(EXP_THREADS) void exposure_apply_bwd_kernel(const float* __restrict__ x,
                                                                         const float* __restrict__ A,
                                                                         const float* __restrict__ g, size_t pixels,
                                                                         float* __restrict__ dx,
                                                                         double* __restrict__ slots) {
  float a[EXP_TERMS];
  double acc[DA ? EXP_TERMS : 1];
  if constexpr (DX) {
#pragma unroll
    for (int i = 0; i < EXP_TERMS; ++i) a[i] = A[i];
  }
  if constexpr (DA) {
#pragma unroll
    for (int i = 0; i < EXP_TERMS; ++i) acc[i] = 0.0;
  }
  const size_t stride = (size_t)gridDim.x * EXP_THREADS;
  for (size_t p = (size_t)blockIdx.x * EXP_THREADS + threadIdx.x; p < pixels; p += stride) {
    const float gv[3] = {g[p], g[pixels + p], g[2 * pixels + p]};
    if constexpr (DX) {
#pragma unroll
      for (int k = 0; k < 3; ++k) dx[k * pixels + p] = a[4 * k] * gv[0] + a[4 * k + 1] * gv[1] + a[4 * k + 2] * gv[2];
    }
    if constexpr (DA) {
      const double xd[3] = {(double)x[p], (double)x[pixels + p], (double)x[2 * pixels + p]};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double gd = (double)gv[c];
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[4 * k + c] += xd[k] * gd;
        acc[4 * c + 3] += gd;
      }
    }
  }
  if constexpr (DA) {
    // every lane of the block arrives here (a lane without a pixel carries zeros); term t is folded by lane t
    __shared__ double wave_sum[EXP_WAVES][EXP_TERMS];
    const double d = ordered_block_sum_by_lane<EXP_WAVES>(acc, wave_sum);
    if (threadIdx.x < EXP_TERMS) slots[(size_t)blockIdx.x * EXP_TERMS + threadIdx.x] = d;
  }
}

// One block.  Thread (stripe, term) walks the slots stripe, stripe + 16, ... of its term, then the 16 stripe sums are
// added in stripe order and rounded to float32 once.
__global__ __launch_bounds__(EXP_FIN_THREADS) void exposure_grad_finish_kernel(const double* __restrict__ slots,
                                                                               int nslots, float* __restrict__ dA) {
  __shared__ double part[EXP_FIN_STRIPES][EXP_TERMS];
  const int term = threadIdx.x & 15, stripe = threadIdx.x >> 4;
  if (term < EXP_TERMS) {
    double acc = 0.0;
    for (int b = stripe; b < nslots; b += EXP_FIN_STRIPES) acc += slots[(size_t)b * EXP_TERMS + term];
    part[stripe][term] = acc;
  }
  __syncthreads();
  if (threadIdx.x < EXP_TERMS) {
    double acc = part[0][threadIdx.x];
    for (int k = 1; k < EXP_FIN_STRIPES; ++k) acc += part[k][threadIdx.x];
    dA[threadIdx.x] = (float)acc;
  }
}

int exposure_blocks(size_t pixels) {
  const size_t b = (pixels + EXP_THREADS - 1) / EXP_THREADS;
  return (int)(b < (size_t)EXPOSURE_MAX_BLOCKS ? (b ? b : 1) : (size_t)EXPOSURE_MAX_BLOCKS);
}

// dx / dA may be nullptr; with dA the backward leaves 12 double sums per block in `workspace` (at most
// EXPOSURE_MAX_BLOCKS slots) and a one-block kernel behind it adds them in a fixed order
void launch_exposure_apply_bwd(const float* x, const float* A, const float* g, size_t pixels, float* dx, float* dA,
                               void* workspace, hipStream_t s) {
  const int blocks = exposure_blocks(pixels);
  double* slots = static_cast<double*>(workspace);
  const dim3 grid(blocks), block(EXP_THREADS);
  if (dx && dA) hipLaunchKernelGGL((exposure_apply_bwd_kernel<true, true>), grid, block, 0, s, x, A, g, pixels, dx, slots);
  else if (dx) hipLaunchKernelGGL((exposure_apply_bwd_kernel<true, false>), grid, block, 0, s, x, A, g, pixels, dx, slots);
  else if (dA) hipLaunchKernelGGL((exposure_apply_bwd_kernel<false, true>), grid, block, 0, s, x, A, g, pixels, dx, slots);
  if (dA) hipLaunchKernelGGL(exposure_grad_finish_kernel, dim3(1), dim3(EXP_FIN_THREADS), 0, s, slots, blocks, dA);
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_exposure_workspace_bytes(int32_t H, int32_t W) {
  if (!image_shape_ok(H, W)) return 0;
  return align_up((size_t)exposure_blocks((size_t)H * (size_t)W) * EXP_TERMS * sizeof(double), 256);
}
int gsr_exposure_apply_fwd(const float* x, const float* A, int32_t H, int32_t W, float* y, void* stream) {
  if (!x || !A || !y) return fail(GSR_E_BADARG, "NULL argument");
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "bad image shape");
  if (!aligned({x, A, y}, 3u)) return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t pixels = (size_t)H * (size_t)W;
  hipLaunchKernelGGL(exposure_apply_fwd_kernel, dim3(exposure_blocks(pixels)), dim3(EXP_THREADS), 0, s, x, A, pixels, y);
  return check(false, s, "exposure_apply_fwd");
}
int gsr_exposure_apply_bwd(const float* x, const float* A, const float* g, int32_t H, int32_t W, float* dx, float* dA,
                           void* workspace, void* stream) {
  if (!g || (dx && !A) || (dA && (!x || !workspace))) return fail(GSR_E_BADARG, "NULL argument");
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "bad image shape");
  if (!aligned({x, A, g, dx, dA}, 3u)) return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  if (dA && !aligned({workspace}, 7u)) return fail(GSR_E_ALIGN, "the workspace must be 8-byte aligned");
  if (!dx && !dA) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_exposure_apply_bwd(x, A, g, (size_t)H * (size_t)W, dx, dA, workspace, s);
  return check(false, s, "exposure_apply_bwd");
}

}  // extern "C"

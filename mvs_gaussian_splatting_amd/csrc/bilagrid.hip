// Per-image bilateral grids (include/gsr.h, ABI v38): the grid of 3x4 colour affines of "Bilateral
// Guided Radiance Field Processing", indexed by pixel position and by the pixel's own luminance, sliced trilinearly and
// applied to the rendered image before the loss; its gradients; and the total-variation term that regularises it.  The
// arithmetic of a pixel is csrc/bilagrid_math.h: doubles between float32 loads and one rounding per output.
//
//   * bilagrid_pixel_kernel<DX, STAGED>: one pixel per lane, a wave reads and writes 256 consecutive bytes of each image
//     plane.  Forward (DX = false): Y.  Backward (DX = true): dL/dX, a gather on the lane's own pixel through the same 96
//     grid reads.  STAGED = false: the cells come through the caches (every pixel of a wave's run of a row reads the same
//     one or two columns of cells).  STAGED = true: a block of 1024 lanes first copies the whole grid into LDS (96 KB at
//     the default shape; at most BG_STAGE_FLOATS floats) and then walks pixels with a grid stride.  Which of the two a
//     call takes is pick_staging's; the bits do not depend on it.
//   * bilagrid_grid_grad_kernel: dL/dG without atomics, gathered by grid vertex.  Block (vertex (i, j), share s) walks
//     the rows y_lo + s, y_lo + s + S, ... of the rectangle of pixels that can put a weight on the vertex (its up to four
//     adjacent cells); wave l of the block keeps the 12 sums of z level l (the dense hat weight of the level, zero on
//     most pixels), a lane the columns x_lo + lane, + 64, ...  The lanes are added with an xor butterfly and the wave
//     stores 12 doubles in its slot; bilagrid_grid_grad_finish_kernel adds the S slots of an element in share order and
//     rounds once.  Every element is written, zero where no pixel touches it.  The order is fixed by the shapes alone:
//     the same bits from run to run.
//   * bilagrid_tv_kernel: one lane per grid element computes the element's forward and backward differences along z, y
//     and x: the forward ones give its share of the value, both give d tv / d element.  Block sums in double
//     (ordered_sum.h), bilagrid_tv_finish_kernel adds the block slots in a fixed order and rounds once.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "ordered_sum.h"
#include "bilagrid_math.h"

namespace gsr {

namespace {

constexpr int BG_THREADS = 256;
constexpr int BG_STAGE_THREADS = 1024;
constexpr int BG_STAGE_FLOATS = BG_TERMS * 8 * 16 * 16;     // the default grid: 96 KB of the CU's 160 KB
constexpr int BG_STAGE_BLOCKS = 256;                        // one per CU: two do not fit beside each other
constexpr int BG_MAX_SHARES = 8;                            // S: row shares of a vertex's rectangle
constexpr int BG_TV_THREADS = 256, BG_TV_WAVES = BG_TV_THREADS / WAVE;
constexpr int BG_TV_MAX_BLOCKS = 1024;
constexpr int BG_TV_FIN_THREADS = 256;

template <bool DX, bool STAGED>
__global__ __launch_bounds__(STAGED ? BG_STAGE_THREADS : BG_THREADS) void bilagrid_pixel_kernel(
    const float* __restrict__ x, const float* __restrict__ grid, const float* __restrict__ g, BilagridShape s,
    float* __restrict__ out) {
  const size_t pixels = (size_t)s.H * (size_t)s.W;
  const float* G = grid;
  size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = pixels;                                   // not staged: one pixel per lane
  if constexpr (STAGED) {
    __shared__ float staged[BG_STAGE_FLOATS];
    const int n = BG_TERMS * s.L * s.Hg * s.Wg;             // <= BG_STAGE_FLOATS: the entry point checked
    for (int i = threadIdx.x; i < n; i += BG_STAGE_THREADS) staged[i] = grid[i];
    __syncthreads();
    G = staged;
    stride = (size_t)gridDim.x * BG_STAGE_THREADS;
  }
  for (; p < pixels; p += stride) {
    const int py = (int)(p / (size_t)s.W), px = (int)(p - (size_t)py * (size_t)s.W);
    const float X[3] = {x[p], x[pixels + p], x[2 * pixels + p]};
    BilagridPixel pix;
    bg_pixel(X, px, py, s, pix);
    double A[BG_TERMS], dA_dz[BG_TERMS];
    bg_slice(G, s, pix, A, dA_dz);
    float r[3];
    if constexpr (DX) {
      const float gv[3] = {g[p], g[pixels + p], g[2 * pixels + p]};
      bg_image_grad(A, dA_dz, X, gv, pix.dz_dgray, r);
    } else {
      bg_apply(A, X, r);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c * pixels + p] = r[c];
  }
}

// rows of the rectangle of pixels around a vertex, at most: two cells and the slack of bg_vertex_range
__host__ __device__ inline int bilagrid_shares(int H, int Hg) {
  const int rows = 2 * (H / (Hg - 1) + 1) + 3;
  const int s = (rows + 15) / 16;
  return s < 1 ? 1 : (s > BG_MAX_SHARES ? BG_MAX_SHARES : s);
}

// grid (Wg, Hg, S), block 64 L.  slots[(((j Wg + i) S + share) L + l) 12 + term]
__global__ __launch_bounds__(WAVE * BG_MAX_L) void bilagrid_grid_grad_kernel(const float* __restrict__ x,
                                                                            const float* __restrict__ g, BilagridShape s,
                                                                            double* __restrict__ slots) {
  const int vi = blockIdx.x, vj = blockIdx.y, share = blockIdx.z, shares = gridDim.z;
  const int lane = threadIdx.x & (WAVE - 1), level = threadIdx.x / WAVE;
  const size_t pixels = (size_t)s.H * (size_t)s.W;
  int x_lo, x_hi, y_lo, y_hi;
  bg_vertex_range(vi, s.W, s.Wg, x_lo, x_hi);
  bg_vertex_range(vj, s.H, s.Hg, y_lo, y_hi);
  double acc[BG_TERMS];
#pragma unroll
  for (int t = 0; t < BG_TERMS; ++t) acc[t] = 0.0;
  for (int py = y_lo + share; py <= y_hi; py += shares) {
    int j0;
    double tv;
    bg_cell(bg_axis_coord(py, s.H, s.Hg), s.Hg, j0, tv);
    const double wy = bg_axis_weight(j0, tv, vj);
    if (wy == 0.0) continue;                                 // the same for the whole block
    const size_t row = (size_t)py * (size_t)s.W;
    for (int px = x_lo + lane; px <= x_hi; px += WAVE) {
      const size_t p = row + (size_t)px;
      const float X[3] = {x[p], x[pixels + p], x[2 * pixels + p]};
      BilagridPixel pix;
      bg_pixel(X, px, py, s, pix);
      const double w = (bg_axis_weight(pix.i0, pix.tu, vi) * wy) * bg_axis_weight(pix.l0, pix.tz, level);
      if (w != 0.0) {
        const float gv[3] = {g[p], g[pixels + p], g[2 * pixels + p]};
        bg_grid_terms(X, gv, w, acc);
      }
    }
  }
  // every lane of the wave arrives here; a lane's partners are fixed
  double mine = 0.0;
#pragma unroll
  for (int t = 0; t < BG_TERMS; ++t) {
    const double d = wave_reduce_add_f64(acc[t]);
    if (lane == t) mine = d;
  }
  if (lane < BG_TERMS)
    slots[((((size_t)vj * s.Wg + vi) * shares + share) * s.L + level) * BG_TERMS + lane] = mine;
}

// one lane per element of dG [12, L, Hg, Wg]
__global__ __launch_bounds__(BG_THREADS) void bilagrid_grid_grad_finish_kernel(const double* __restrict__ slots,
                                                                               BilagridShape s, int shares,
                                                                               float* __restrict__ dG) {
  const int cells = s.L * s.Hg * s.Wg;
  const int e = blockIdx.x * BG_THREADS + threadIdx.x;
  if (e >= BG_TERMS * cells) return;
  const int term = e / cells, cell = e - term * cells;
  const int level = cell / (s.Hg * s.Wg), vertex = cell - level * (s.Hg * s.Wg);
  double acc = 0.0;
  for (int k = 0; k < shares; ++k) acc += slots[(((size_t)vertex * shares + k) * s.L + level) * BG_TERMS + term];
  dG[e] = (float)acc;
}

// tv = (1/N) sum_n sum_axis mean((G[n] shifted by one along the axis - G[n])^2); coef[a] = 1 / (N M_a), M_a the number
// of differences of one image along axis a (z, y, x)
struct BilagridTv {
  int Wg, Hg, L;
  size_t total;          // N 12 L Hg Wg
  double coef[3];
};

__global__ __launch_bounds__(BG_TV_THREADS) void bilagrid_tv_kernel(const float* __restrict__ G, BilagridTv tv,
                                                                    float* __restrict__ dG, double* __restrict__ slots) {
  const size_t stride = (size_t)gridDim.x * BG_TV_THREADS;
  const int size[3] = {tv.L, tv.Hg, tv.Wg};
  const size_t step[3] = {(size_t)tv.Hg * tv.Wg, (size_t)tv.Wg, 1};
  double value = 0.0;
  for (size_t e = (size_t)blockIdx.x * BG_TV_THREADS + threadIdx.x; e < tv.total; e += stride) {
    const int ix = (int)(e % tv.Wg), iy = (int)((e / tv.Wg) % tv.Hg), iz = (int)((e / step[0]) % tv.L);
    const int at[3] = {iz, iy, ix};
    const double here = G[e];
    double grad = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double fwd = at[a] + 1 < size[a] ? (double)G[e + step[a]] - here : 0.0;
      const double bwd = at[a] > 0 ? here - (double)G[e - step[a]] : 0.0;
      value += tv.coef[a] * (fwd * fwd);
      grad += (2.0 * tv.coef[a]) * (bwd - fwd);
    }
    if (dG) dG[e] = (float)grad;
  }
  __shared__ double wave_sum[BG_TV_WAVES];
  const double b = ordered_block_sum<BG_TV_WAVES, FROM_WAVE0>(value, wave_sum);
  if (threadIdx.x == 0) slots[blockIdx.x] = b;
}

// One block.  Thread t walks the slots t, t + 256, ...; the 256 sums are added in thread order and rounded once.
__global__ __launch_bounds__(BG_TV_FIN_THREADS) void bilagrid_tv_finish_kernel(const double* __restrict__ slots,
                                                                               int nslots, float* __restrict__ value) {
  __shared__ double part[BG_TV_FIN_THREADS];
  double acc = 0.0;
  for (int b = threadIdx.x; b < nslots; b += BG_TV_FIN_THREADS) acc += slots[b];
  part[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = part[0];
    for (int k = 1; k < BG_TV_FIN_THREADS; ++k) total += part[k];
    *value = (float)total;
  }
}

int tv_blocks(size_t total) {
  const size_t b = (total + BG_TV_THREADS - 1) / BG_TV_THREADS;
  return (int)(b < (size_t)BG_TV_MAX_BLOCKS ? b : (size_t)BG_TV_MAX_BLOCKS);
}

size_t grid_grad_bytes(int H, int Wg, int Hg, int L) {
  return (size_t)Wg * Hg * bilagrid_shares(H, Hg) * L * BG_TERMS * sizeof(double);
}

bool staged_fits(int Wg, int Hg, int L) { return BG_TERMS * L * Hg * Wg <= BG_STAGE_FLOATS; }

bool staging_ok(int staging, int Wg, int Hg, int L) {
  if (staging == GSR_BILAGRID_STAGE_LDS) return staged_fits(Wg, Hg, L);
  return staging == GSR_BILAGRID_STAGE_AUTO || staging == GSR_BILAGRID_STAGE_CACHE;
}

// GSR_BILAGRID_STAGE_AUTO: the grid goes to LDS when it fits and every block of the staged launch has at least one full
// pass of pixels to spread its copy of the grid over (measured at 1920 x 1080 with the default grid: 73 us staged, 137 us
// through the caches; profiles/bilagrid/NOTES.md); a smaller image is read through the caches
int pick_staging(int staging, size_t pixels, int Wg, int Hg, int L) {
  if (staging != GSR_BILAGRID_STAGE_AUTO) return staging;
  return staged_fits(Wg, Hg, L) && pixels >= (size_t)BG_STAGE_BLOCKS * BG_STAGE_THREADS ? GSR_BILAGRID_STAGE_LDS
                                                                                       : GSR_BILAGRID_STAGE_CACHE;
}

// staging: GSR_BILAGRID_STAGE_*; `g` NULL: forward into out, else dL/dX into out
template <bool DX>
void launch_pixels(const float* x, const float* grid, const float* g, const BilagridShape& s, int staging, float* out,
                   hipStream_t st) {
  const size_t pixels = (size_t)s.H * (size_t)s.W;
  if (pick_staging(staging, pixels, s.Wg, s.Hg, s.L) == GSR_BILAGRID_STAGE_LDS) {
    const size_t b = (pixels + BG_STAGE_THREADS - 1) / BG_STAGE_THREADS;
    const int blocks = (int)(b < (size_t)BG_STAGE_BLOCKS ? b : (size_t)BG_STAGE_BLOCKS);
    hipLaunchKernelGGL((bilagrid_pixel_kernel<DX, true>), dim3(blocks), dim3(BG_STAGE_THREADS), 0, st, x, grid, g, s, out);
  } else {
    const unsigned blocks = (unsigned)((pixels + BG_THREADS - 1) / BG_THREADS);
    hipLaunchKernelGGL((bilagrid_pixel_kernel<DX, false>), dim3(blocks), dim3(BG_THREADS), 0, st, x, grid, g, s, out);
  }
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_bilagrid_workspace_bytes(int32_t H, int32_t W, int32_t Wg, int32_t Hg, int32_t L) {
  if (!bilagrid_shape_ok(Wg, Hg, L)) return 0;
  if (H == 0 && W == 0) return align_up((size_t)BG_TV_MAX_BLOCKS * sizeof(double), 256);   // the TV term's
  if (!image_shape_ok(H, W)) return 0;
  return align_up(grid_grad_bytes(H, Wg, Hg, L), 256);
}

int gsr_bilagrid_slice_fwd(const float* x, const float* grid, int32_t H, int32_t W, int32_t Wg, int32_t Hg, int32_t L,
                           int32_t staging, float* y, void* stream) {
  if (!x || !grid || !y) return fail(GSR_E_BADARG, "NULL argument");
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "bad image shape");
  if (!bilagrid_shape_ok(Wg, Hg, L)) return fail(GSR_E_BADARG, "the grid must be 2..64 x 2..64 x 2..16 (Wg, Hg, L)");
  if (!staging_ok(staging, Wg, Hg, L))
    return fail(GSR_E_BADARG, "staging must be one of GSR_BILAGRID_STAGE_*, _LDS with a grid of at most 24576 floats");
  if (!aligned({x, grid, y}, 3u)) return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const BilagridShape shape = {H, W, Wg, Hg, L};
  launch_pixels<false>(x, grid, nullptr, shape, staging, y, s);
  return check(false, s, "bilagrid_slice_fwd");
}

int gsr_bilagrid_slice_bwd(const float* x, const float* grid, const float* g, int32_t H, int32_t W, int32_t Wg,
                           int32_t Hg, int32_t L, int32_t staging, float* dx, float* dgrid, void* workspace, void* stream) {
  if (!x || !g || (dx && !grid) || (dgrid && !workspace)) return fail(GSR_E_BADARG, "NULL argument");
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "bad image shape");
  if (!bilagrid_shape_ok(Wg, Hg, L)) return fail(GSR_E_BADARG, "the grid must be 2..64 x 2..64 x 2..16 (Wg, Hg, L)");
  if (!staging_ok(staging, Wg, Hg, L))
    return fail(GSR_E_BADARG, "staging must be one of GSR_BILAGRID_STAGE_*, _LDS with a grid of at most 24576 floats");
  if (!aligned({x, grid, g, dx, dgrid}, 3u)) return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  if (dgrid && !aligned({workspace}, 7u)) return fail(GSR_E_ALIGN, "the workspace must be 8-byte aligned");
  if (!dx && !dgrid) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const BilagridShape shape = {H, W, Wg, Hg, L};
  if (dx) launch_pixels<true>(x, grid, g, shape, staging, dx, s);
  if (dgrid) {
    double* slots = static_cast<double*>(workspace);
    const int shares = bilagrid_shares(H, Hg);
    hipLaunchKernelGGL(bilagrid_grid_grad_kernel, dim3(Wg, Hg, shares), dim3(WAVE * L), 0, s, x, g, shape, slots);
    const int elements = BG_TERMS * L * Hg * Wg;
    hipLaunchKernelGGL(bilagrid_grid_grad_finish_kernel, dim3((elements + BG_THREADS - 1) / BG_THREADS),
                       dim3(BG_THREADS), 0, s, slots, shape, shares, dgrid);
  }
  return check(false, s, "bilagrid_slice_bwd");
}

int gsr_bilagrid_tv_fwd_bwd(const float* grids, int32_t N, int32_t Wg, int32_t Hg, int32_t L, float* value,
                            float* dgrids, void* workspace, void* stream) {
  if (!grids || !value || !workspace) return fail(GSR_E_BADARG, "NULL argument");
  if (N < 1 || N > (1 << 16)) return fail(GSR_E_BADARG, "N must lie in 1..65536");
  if (!bilagrid_shape_ok(Wg, Hg, L)) return fail(GSR_E_BADARG, "the grids must be 2..64 x 2..64 x 2..16 (Wg, Hg, L)");
  if (!aligned({grids, value, dgrids}, 3u)) return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  if (!aligned({workspace}, 7u)) return fail(GSR_E_ALIGN, "the workspace must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  BilagridTv tv;
  tv.Wg = Wg; tv.Hg = Hg; tv.L = L;
  tv.total = (size_t)N * BG_TERMS * L * Hg * Wg;
  const double n = (double)N, terms = (double)BG_TERMS;
  tv.coef[0] = 1.0 / (n * (terms * (double)(L - 1) * (double)Hg * (double)Wg));
  tv.coef[1] = 1.0 / (n * (terms * (double)L * (double)(Hg - 1) * (double)Wg));
  tv.coef[2] = 1.0 / (n * (terms * (double)L * (double)Hg * (double)(Wg - 1)));
  double* slots = static_cast<double*>(workspace);
  const int blocks = tv_blocks(tv.total);
  hipLaunchKernelGGL(bilagrid_tv_kernel, dim3(blocks), dim3(BG_TV_THREADS), 0, s, grids, tv, dgrids, slots);
  hipLaunchKernelGGL(bilagrid_tv_finish_kernel, dim3(1), dim3(BG_TV_FIN_THREADS), 0, s, slots, blocks, value);
  return check(false, s, "bilagrid_tv_fwd_bwd");
}

}  // extern "C"

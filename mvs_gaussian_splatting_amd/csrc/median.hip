// Median-depth map of a rendered frame (the second depth of 2DGS) and the per-pixel Gaussian id map, with gradients
// (DESIGN.md §7.17).
//
//   k* = the last composited entry with T_k > 0.5 (T_k: the transmittance BEFORE entry k)
//   median = z_{k*},   median_id = id_{k*}                 (0 / -1 on a pixel without a composited entry)
//
// over the list entries the colour pass composited at the pixel -- the entries of depth.hip (§7.9): the first
// n_contrib[pixel] entries of the tile's list whose alpha passes the 1/255 test, alpha evaluated by the walk the maps share
// (map_walk.h) and T updated with the colour pass's single fma, so the decisions and the running T come out bit for bit.
// z is BinInfo::depth.  This is 2DGS's rule `if (T > 0.5) { median_depth = depth; median_contributor = i; }`, taken
// before the blend: the first composited entry always qualifies (T = 1), and a ray that never gets below one half keeps
// its last composited entry.
//
// Once T <= 0.5 no later entry can qualify (T only falls), so a lane is done there: the forward is the first map here
// that stops early, and a tile's round loop ends when every lane of the workgroup is done.
//
// The selection is piecewise constant: dL/dz_{k*} = g[pixel] and nothing else.  The forward leaves the list position of
// k* per pixel (state, NONE where there is no entry); the backward adds g into one float per Gaussian of a zeroed [P]
// accumulator of its own, and a per-Gaussian kernel takes z to means3D through the view matrix's third column, the step
// aux_geom_bwd_kernel takes for its d z word.  Nothing of the colour path is read-modified; nothing waits on another
// workgroup.
//
// Built with the flags of depth.o; the arithmetic that has to match the colour pass is explicit fma.
#include "gsr_common.h"
#include "gsr_launch.h"
#include "map_walk.h"

namespace gsr {

constexpr uint32_t MED_NONE = 0xffffffffu;      // state of a pixel without a composited entry

// ------------------------------------------------------------------------------------------------------------------
// Forward: one 256-lane workgroup per tile (the colour pass's tile order), one lane per pixel.  A round stages up to 256
// entries in LDS; every lane that is not done walks the round's entries in list order up to ITS n_contrib and leaves the
// walk when its T has fallen to one half.  Whether a further round is needed is one flag per wave, read by every lane
// behind the barrier that also ends the previous round: both barriers of a round are reached by all 256 lanes, the
// lane-dependent work sits between them.  No atomics: the maps are the same bits from run to run.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_CHUNK) void median_depth_fwd_kernel(int W, int H, int grid_x,
                                                                     const uint32_t* __restrict__ tile_order,
                                                                     const uint2* __restrict__ ranges,
                                                                     const uint32_t* __restrict__ point_list,
                                                                     const GeomRec* __restrict__ rec,
                                                                     const BinInfo* __restrict__ bin,
                                                                     const uint32_t* __restrict__ n_contrib,
                                                                     float* __restrict__ median,
                                                                     int32_t* __restrict__ median_id,
                                                                     uint32_t* __restrict__ state) {
  __shared__ float4 sA[MAP_CHUNK];
  __shared__ float4 sB[MAP_CHUNK];
  __shared__ float sZ[MAP_CHUNK];
  __shared__ uint32_t sId[MAP_CHUNK];
  __shared__ uint32_t sMax[4];
  __shared__ uint32_t sLive[4];
  const int tid = threadIdx.x;
  const MapPixel m = map_pixel(W, H, grid_x, tile_order, ranges);
  const float pxf = (float)m.px, pyf = (float)m.py;
  const uint32_t last = map_last(m, n_contrib, m.inside);
  const uint32_t tmax = block_max_u32(last, sMax);

  float T = 1.0f, med = 0.0f;
  int32_t mid = -1;
  uint32_t pos = MED_NONE;
  bool live = last > 0u;      // not done: T > 0.5 and entries of its own left
  for (uint32_t base = 0;; base += MAP_CHUNK) {
    const bool wave_live = __builtin_amdgcn_ballot_w64(live) != 0ull;
    if ((tid & (WAVE - 1)) == 0) sLive[tid / WAVE] = wave_live ? 1u : 0u;
    __syncthreads();      // the flags are in; every lane has left the previous round's entries
    if ((sLive[0] | sLive[1] | sLive[2] | sLive[3]) == 0u) break;      // the same four words in every lane
    // a live lane has last > base, so tmax > base
    const uint32_t n = min((uint32_t)MAP_CHUNK, tmax - base);
    if ((uint32_t)tid < n) {
      const MapEntry e = load_entry(rec, point_list[m.start + base + tid]);
      sA[tid] = e.lr.A;
      sB[tid] = e.lr.B;
      sZ[tid] = bin[e.id].depth;
      sId[tid] = e.id;
    }
    __syncthreads();      // the round is staged; the flags have been read
    if (live) {
      const uint32_t mine = min(n, last - base);
      for (uint32_t k = 0; k < mine; ++k) {
        const float4 a = sA[k], b = sB[k];
        const float alpha = map_alpha(a, b, pxf, pyf);
        if (alpha >= ALPHA_MIN) {
          // T > 0.5 here: the walk leaves at the first update that takes it to one half
          med = sZ[k];
          mid = (int32_t)sId[k];
          pos = base + k;
          T = __builtin_fmaf(-alpha, T, T);      // T (1 - alpha), rounded once: the colour pass's update
          if (!(T > 0.5f)) break;
        }
      }
      live = T > 0.5f && last - base > n;
    }
  }
  if (m.inside) {
    median[m.pix] = med;
    median_id[m.pix] = mid;
    state[m.pix] = pos;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Backward: same grid.  Per 256-entry round the lanes whose saved position falls in the round add their g into the LDS
// float slot of that entry; the lane that would have staged the entry then issues ONE global float atomic add for a
// non-zero slot: at most one per tile and entry, however many of the tile's pixels chose it.  acc [P] is zeroed by the
// caller.  Rounds in front of the tile's first chosen position and behind its last are not visited.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_CHUNK) void median_depth_bwd_kernel(int W, int H, int grid_x,
                                                                     const uint32_t* __restrict__ tile_order,
                                                                     const uint2* __restrict__ ranges,
                                                                     const uint32_t* __restrict__ point_list,
                                                                     const uint32_t* __restrict__ state,
                                                                     const float* __restrict__ dL_dmedian,
                                                                     float* __restrict__ acc) {
  __shared__ float sSum[MAP_CHUNK];
  __shared__ uint32_t sMax[4];
  __shared__ uint32_t sMin[4];
  const int tid = threadIdx.x;
  const MapPixel m = map_pixel(W, H, grid_x, tile_order, ranges);
  const uint32_t start = m.start;
  uint32_t pos = m.inside ? state[m.pix] : MED_NONE;
  if (pos >= m.len) pos = MED_NONE;      // a state of this frame never is; no index leaves the tile's list whatever it holds
  const float g = pos != MED_NONE ? dL_dmedian[m.pix] : 0.0f;
  const uint32_t end = block_max_u32(pos != MED_NONE ? pos + 1u : 0u, sMax);                 // one past the last chosen
  const uint32_t first = MED_NONE - block_max_u32(pos != MED_NONE ? MED_NONE - pos : 0u, sMin);  // the first chosen

  for (uint32_t base = end > 0u ? first - first % MAP_CHUNK : 0u; base < end; base += MAP_CHUNK) {
    sSum[tid] = 0.0f;
    __syncthreads();
    if (pos != MED_NONE && pos - base < (uint32_t)MAP_CHUNK) atomicAdd(&sSum[pos - base], g);      // pos >= base: unsigned wrap
    __syncthreads();
    // the lane reads the slot it zeroes in the next round: no barrier between the two
    if ((uint32_t)tid < end - base) {
      const float s = sSum[tid];
      if ((__float_as_uint(s) << 1) != 0u) atomicAdd(acc + point_list[start + base + tid], s);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Per Gaussian: d z -> d mean3D through the view matrix's third column (z_view = sum_i m[4 i + 2] mean_i + m[14]).  Every
// row is written; a row whose accumulator is zero is zero and reads nothing else.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PRE_BLOCK) void median_depth_finish_kernel(int P, const float* __restrict__ viewmatrix,
                                                                        const float* __restrict__ acc,
                                                                        float* __restrict__ d_means3D) {
  const int idx = blockIdx.x * PRE_BLOCK + threadIdx.x;
  if (idx >= P) return;
  const float dz = acc[idx];
  float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
  if ((__float_as_uint(dz) << 1) != 0u) {
    d0 = viewmatrix[2] * dz;
    d1 = viewmatrix[6] * dz;
    d2 = viewmatrix[10] * dz;
  }
  d_means3D[3 * (size_t)idx + 0] = d0;
  d_means3D[3 * (size_t)idx + 1] = d1;
  d_means3D[3 * (size_t)idx + 2] = d2;
}

void launch_median_depth_fwd(const MapFrame& f, float* median, int32_t* median_id, uint32_t* state, hipStream_t s) {
  hipLaunchKernelGGL(median_depth_fwd_kernel, dim3(f.tiles), dim3(MAP_CHUNK), 0, s, f.W, f.H, f.grid_x, f.tile_order,
                     f.ranges, f.point_list, f.rec, f.bin, f.n_contrib, median, median_id, state);
}

void launch_median_depth_bwd(const MapFrame& f, const uint32_t* state, const float* dL_dmedian, float* acc, hipStream_t s) {
  hipLaunchKernelGGL(median_depth_bwd_kernel, dim3(f.tiles), dim3(MAP_CHUNK), 0, s, f.W, f.H, f.grid_x, f.tile_order,
                     f.ranges, f.point_list, state, dL_dmedian, acc);
}

void launch_median_depth_finish(int P, const float* viewmatrix, const float* acc, float* d_means3D, hipStream_t s) {
  const int nb = (P + PRE_BLOCK - 1) / PRE_BLOCK;
  if (nb > 0)
    hipLaunchKernelGGL(median_depth_finish_kernel, dim3(nb), dim3(PRE_BLOCK), 0, s, P, viewmatrix, acc, d_means3D);
}

}  // namespace gsr

// Per-Gaussian contribution statistics of a rendered frame: which Gaussians the pictures are made of.
//
// For Gaussian g let p run over the pixels where the colour pass composited g: the entries among the first
// n_contrib[p] of the tile's list that pass alpha >= 1/255 (the rule of depth.hip), and w = alpha T with T the
// transmittance in front of the entry -- the w of every map: the shared walk's alpha (map_walk.h: map_alpha) and the
// colour pass's single-fma T update, so the decisions and the weights are the colour pass's bit for bit.  Per Gaussian, int64:
//
//    stats[g][0] += sum_p q(w),  q(w) = round-to-nearest(w 2^30)    (w <= 0.99: 30 bits)
//    stats[g][1] += number of such pixels
//    stats[g][2]  = max(stats[g][2], float32 bits of max_p w)        (w > 0: unsigned integer order is float order)
//
// Only integer adds and an integer max touch the buffer, in LDS and in device memory: whatever order the waves, the
// tiles and the views arrive in, the result is the same bits.  Range: 2^63 / 2^30 weight units, about 4000 fully covered
// 1080p frames for a single Gaussian.
//
// The grid and the staging are map_walk.h's (map_pixel, load_entry): one 256-lane workgroup per tile in the colour pass's tile order,
// one lane per pixel, 256 list entries staged in LDS per round.  Per entry a wave reduces its 64 pixels (ballot +
// popcount for the count, shuffles for the max and for the 64-bit sum: a wave's sum can reach 2^36), the four waves
// meet in LDS, and the lane that staged the entry issues at most three 64-bit atomics into the entry's row.  A simple
// mapping: the statistics are an optional side output.
//
// Built like depth.hip (-ffp-contract=off, no SLP): w = alpha * T must stay a product of its own.
#include "gsr_common.h"
#include "gsr_launch.h"
#include "map_walk.h"

namespace gsr {

constexpr float CONTRIB_FX_ONE = 1073741824.0f;      // 2^30: the fixed-point unit of column 0

__device__ inline unsigned long long wave_reduce_add_u64(unsigned long long v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
  return v;
}

__global__ __launch_bounds__(MAP_CHUNK) void contribution_kernel(int W, int H, int grid_x,
                                                                     const uint32_t* __restrict__ tile_order,
                                                                     const uint2* __restrict__ ranges,
                                                                     const uint32_t* __restrict__ point_list,
                                                                     const GeomRec* __restrict__ rec,
                                                                     const uint32_t* __restrict__ n_contrib,
                                                                     const uint8_t* __restrict__ pixel_mask,
                                                                     unsigned long long* __restrict__ stats) {
  __shared__ float4 sA[MAP_CHUNK];
  __shared__ float4 sB[MAP_CHUNK];
  __shared__ unsigned long long sSum[MAP_CHUNK];
  __shared__ uint32_t sCount[MAP_CHUNK];
  __shared__ uint32_t sWmax[MAP_CHUNK];
  __shared__ uint32_t sLast[4];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const MapPixel m = map_pixel(W, H, grid_x, tile_order, ranges);
  const float pxf = (float)m.px, pyf = (float)m.py;
  // a pixel outside the image or taken out by the mask composites nothing here: it walks no entry at all
  const bool counted = m.inside && (pixel_mask == nullptr || pixel_mask[m.pix] != 0);
  const uint32_t last = map_last(m, n_contrib, counted);
  const uint32_t wlast = wave_reduce_max_u32(last);      // how far this wave's pixels walk
  const uint32_t tmax = block_max_of_waves(wlast, sLast);

  float T = 1.0f;
  uint32_t id = 0u;
  for (uint32_t base = 0; base < tmax; base += MAP_CHUNK) {
    const uint32_t n = min((uint32_t)MAP_CHUNK, tmax - base);
    if ((uint32_t)tid < n) {
      const MapEntry e = load_entry(rec, point_list[m.start + base + tid]);
      id = e.id;
      sA[tid] = e.lr.A;
      sB[tid] = e.lr.B;
    }
    sSum[tid] = 0ull;
    sCount[tid] = 0u;
    sWmax[tid] = 0u;
    __syncthreads();
    const uint32_t wmine = wlast > base ? min(n, wlast - base) : 0u;      // uniform over the wave
    for (uint32_t k = 0; k < wmine; ++k) {
      const float4 a = sA[k], b = sB[k];
      const float alpha = map_alpha(a, b, pxf, pyf);
      const bool ok = base + k < last && alpha >= ALPHA_MIN;
      const unsigned long long votes = __builtin_amdgcn_ballot_w64(ok);
      if (votes == 0ull) continue;      // uniform over the wave: none of its pixels composited the entry
      float w = 0.0f;
      if (ok) {
        w = alpha * T;
        T = __builtin_fmaf(-alpha, T, T);      // T (1 - alpha), rounded once: the colour pass's update
      }
      // w < 1: w 2^30 is exact in float32 and below 2^30; lanes that did not composite add 0 and offer 0 to the max
      const unsigned long long sum = wave_reduce_add_u64((unsigned long long)(uint32_t)__builtin_rintf(w * CONTRIB_FX_ONE));
      const uint32_t wmax = wave_reduce_max_u32(__float_as_uint(w));
      if (lane == 0) {
        atomicAdd(&sSum[k], sum);
        atomicAdd(&sCount[k], (uint32_t)__popcll(votes));
        atomicMax(&sWmax[k], wmax);
      }
    }
    __syncthreads();
    if ((uint32_t)tid < n) {
      const uint32_t count = sCount[tid];
      if (count != 0u) {
        unsigned long long* row = stats + 3 * (size_t)id;
        atomicAdd(row + 0, sSum[tid]);
        atomicAdd(row + 1, (unsigned long long)count);
        atomicMax(row + 2, (unsigned long long)sWmax[tid]);
      }
    }
    __syncthreads();
  }
}

void launch_contribution(const MapFrame& f, const uint8_t* pixel_mask, int64_t* stats, hipStream_t s) {
  // the buffer holds non-negative values only: the unsigned atomics are the signed ones
  hipLaunchKernelGGL(contribution_kernel, dim3(f.tiles), dim3(MAP_CHUNK), 0, s, f.W, f.H, f.grid_x, f.tile_order, f.ranges,
                     f.point_list, f.rec, f.n_contrib, pixel_mask, reinterpret_cast<unsigned long long*>(stats));
}

}  // namespace gsr

// Per-Gaussian contribution statistics of a rendered frame: which Gaussians the pictures are made of.
//
// For Gaussian g let p run over the pixels where the colour pass composited g: the entries among the first
// n_contrib[p] of the tile's list that pass alpha >= 1/255 (the rule of depth.hip), and w = alpha T with T the
// transmittance in front of the entry -- the w of aux_maps_fwd_kernel: the colour pass's own functions (render_pair.h)
// and its single-fma T update, so the decisions and the weights are the colour pass's bit for bit.  Per Gaussian, int64:
//
//    stats[g][0] += sum_p q(w),  q(w) = round-to-nearest(w 2^30)    (w <= 0.99: 30 bits)
//    stats[g][1] += number of such pixels
//    stats[g][2]  = max(stats[g][2], float32 bits of max_p w)        (w > 0: unsigned integer order is float order)
//
// Only integer adds and an integer max touch the buffer, in LDS and in device memory: whatever order the waves, the
// tiles and the views arrive in, the result is the same bits.  Range: 2^63 / 2^30 weight units, about 4000 fully covered
// 1080p frames for a single Gaussian.
//
// The grid and the staging are aux_maps_fwd_kernel's: one 256-lane workgroup per tile in the colour pass's tile order,
// one lane per pixel, 256 list entries staged in LDS per round.  Per entry a wave reduces its 64 pixels (ballot +
// popcount for the count, shuffles for the max and for the 64-bit sum: a wave's sum can reach 2^36), the four waves
// meet in LDS, and the lane that staged the entry issues at most three 64-bit atomics into the entry's row.  A simple
// mapping: the statistics are an optional side output.
//
// Built like depth.hip (-ffp-contract=off, no SLP): w = alpha * T must stay a product of its own.
#include "gsr_common.h"
#include "gsr_launch.h"
#include "render_pair.h"

namespace gsr {

constexpr int CONTRIB_CHUNK = 256;      // list entries staged per round: one per lane of the workgroup
constexpr float CONTRIB_FX_ONE = 1073741824.0f;      // 2^30: the fixed-point unit of column 0

__device__ inline uint32_t wave_reduce_max_u32(uint32_t v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, WAVE));
  return v;
}

__device__ inline unsigned long long wave_reduce_add_u64(unsigned long long v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
  return v;
}

__global__ __launch_bounds__(CONTRIB_CHUNK) void contribution_kernel(int W, int H, int grid_x,
                                                                     const uint32_t* __restrict__ tile_order,
                                                                     const uint2* __restrict__ ranges,
                                                                     const uint32_t* __restrict__ point_list,
                                                                     const GeomRec* __restrict__ rec,
                                                                     const uint32_t* __restrict__ n_contrib,
                                                                     const uint8_t* __restrict__ pixel_mask,
                                                                     unsigned long long* __restrict__ stats) {
  __shared__ float4 sA[CONTRIB_CHUNK];
  __shared__ float4 sB[CONTRIB_CHUNK];
  __shared__ unsigned long long sSum[CONTRIB_CHUNK];
  __shared__ uint32_t sCount[CONTRIB_CHUNK];
  __shared__ uint32_t sWmax[CONTRIB_CHUNK];
  __shared__ uint32_t sLast[4];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int tile = __builtin_amdgcn_readfirstlane((int)tile_order[blockIdx.x]);
  const int tile_x = tile % grid_x, tile_y = tile / grid_x;
  const int px = tile_x * TILE + (tid & (TILE - 1)), py = tile_y * TILE + tid / TILE;
  const bool inside = px < W && py < H;
  const size_t pix = (size_t)py * W + px;
  const float pxf = (float)px, pyf = (float)py;
  const uint2 range = ranges[tile];
  const uint32_t start = range.x, len = range.y - range.x;
  // a pixel outside the image or taken out by the mask composites nothing here: it walks no entry at all
  const bool counted = inside && (pixel_mask == nullptr || pixel_mask[pix] != 0);
  const uint32_t last = counted ? min(n_contrib[pix], len) : 0u;
  const uint32_t wlast = wave_reduce_max_u32(last);      // how far this wave's pixels walk
  if (lane == 0) sLast[tid / WAVE] = wlast;
  __syncthreads();
  const uint32_t tmax = max(max(sLast[0], sLast[1]), max(sLast[2], sLast[3]));

  float T = 1.0f;
  uint32_t id = 0u;
  for (uint32_t base = 0; base < tmax; base += CONTRIB_CHUNK) {
    const uint32_t n = min((uint32_t)CONTRIB_CHUNK, tmax - base);
    if ((uint32_t)tid < n) {
      id = point_list[start + base + tid];
      const GeomRec* r = rec + id;
      Staged st;      // the words of the record the alpha needs, as aux_load_entry of depth.hip stages them
      st.q0 = make_float4(r->x, r->y, r->cxx, 0.0f);
      st.q1 = make_float4(0.0f, r->opacity, 0.0f, 0.0f);
      st.q2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      st.kk = r->kk;
      st.isyy = r->isyy;
      LdsRec lr;
      make_lds(st, lr);
      sA[tid] = lr.A;
      sB[tid] = lr.B;
    }
    sSum[tid] = 0ull;
    sCount[tid] = 0u;
    sWmax[tid] = 0u;
    __syncthreads();
    const uint32_t wmine = wlast > base ? min(n, wlast - base) : 0u;      // uniform over the wave
    for (uint32_t k = 0; k < wmine; ++k) {
      const float4 a = sA[k], b = sB[k];
      const float alpha = clamp_alpha(__builtin_amdgcn_exp2f(pair_p2(a.x - pxf, a.y - pyf, a.z, a.w, b.x, b.y)), b.x);
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

void launch_contribution(int W, int H, const uint2* ranges, const uint32_t* point_list, const GeomRec* rec,
                         const uint32_t* n_contrib, const uint32_t* tile_order, const uint8_t* pixel_mask, int64_t* stats,
                         hipStream_t s) {
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  // the buffer holds non-negative values only: the unsigned atomics are the signed ones
  hipLaunchKernelGGL(contribution_kernel, dim3(gx * gy), dim3(CONTRIB_CHUNK), 0, s, W, H, gx, tile_order, ranges, point_list,
                     rec, n_contrib, pixel_mask, reinterpret_cast<unsigned long long*>(stats));
}

}  // namespace gsr

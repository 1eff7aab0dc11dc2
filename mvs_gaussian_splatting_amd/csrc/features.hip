// Per-Gaussian feature vectors F[P,C] composited to C-channel maps of a rendered frame, with gradients.
//
//   feat[c] = sum_i w_i F[id_i, c],   w_i = alpha_i T_i,   c = 0 .. C-1      (no background term, no clamp)
//
// over the list entries the colour pass composited at the pixel -- the entries of depth.hip (§7.9): the first
// n_contrib[pixel] entries of the tile's list whose alpha passes the 1/255 test, alpha evaluated and T updated by the
// walk the maps share (map_walk.h), so the decisions and the running T come out bit for bit.
//
// Channels are processed in groups of FEAT_GROUP in the grid's second dimension: a workgroup composites its tile for its
// group's slice of the rows of F.  The last group is predicated (no read past a row's end, no write past channel C-1).
// Nothing of the colour path or of depth.hip is read-modified; the backward's geometry sums go into a zeroed [P,8]
// accumulator in the layout aux_geom_bwd_kernel reads (word 6, d z, stays 0: a feature does not depend on the depth).
//
// Built with the flags of depth.o; the compositing arithmetic that has to match the colour pass is explicit fma.
#include "gsr_common.h"
#include "gsr_launch.h"
#include "map_walk.h"

namespace gsr {

constexpr int FEAT_GROUP = 8;       // channels per workgroup: two float4 of LDS per staged entry

// channels [c0, c0 + FEAT_GROUP) of row id of F, zero past the row's end
__device__ inline void feat_load_row(const float* __restrict__ F, int C, int c0, uint32_t id, float (&f)[FEAT_GROUP]) {
  const float* row = F + (size_t)id * (size_t)C;
#pragma unroll
  for (int j = 0; j < FEAT_GROUP; ++j) f[j] = c0 + j < C ? row[c0 + j] : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------------
// Forward: grid (tiles, channel groups).  One 256-lane workgroup per tile in the colour pass's tile order, one lane per
// pixel; a round stages up to 256 entries (the colour pass's LDS image and the group's slice of the F row); every lane
// walks the round's entries in list order up to ITS n_contrib.  No atomics: the map is the same bits from run to run.
// T is updated with the colour pass's single fma, so 1 - T at the end is 1 - final_T of the frame bit for bit.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_CHUNK) void feature_maps_fwd_kernel(int W, int H, int grid_x,
                                                                     const uint32_t* __restrict__ tile_order,
                                                                     const uint2* __restrict__ ranges,
                                                                     const uint32_t* __restrict__ point_list,
                                                                     const GeomRec* __restrict__ rec,
                                                                     const uint32_t* __restrict__ n_contrib,
                                                                     const float* __restrict__ F, int C,
                                                                     float* __restrict__ out) {
  __shared__ float4 sA[MAP_CHUNK];
  __shared__ float4 sB[MAP_CHUNK];
  __shared__ float4 sF0[MAP_CHUNK];      // channels c0 .. c0 + 3 of the entry's row
  __shared__ float4 sF1[MAP_CHUNK];      // channels c0 + 4 .. c0 + 7
  __shared__ uint32_t sMax[4];
  const int tid = threadIdx.x;
  const int c0 = (int)blockIdx.y * FEAT_GROUP;
  const MapPixel m = map_pixel(W, H, grid_x, tile_order, ranges);
  const size_t pix = m.pix, HW = (size_t)W * H;
  const float pxf = (float)m.px, pyf = (float)m.py;
  const uint32_t last = map_last(m, n_contrib, m.inside);
  const uint32_t tmax = block_max_u32(last, sMax);

  // The sum is taken about the row of the pixel's FIRST composited entry, R:
  //    feat[c] = R[c] (1 - T_final) + sum_i w_i (F[id_i, c] - R[c]),
  // which is sum_i w_i F[id_i, c] because sum_i w_i = 1 - T_final.  The rounding error is that of the plain sum (every
  // term is bounded by w_i times twice the largest |F|), and a field that is constant over the pixel's contributors
  // comes out as that constant times 1 - T_final rounded once: the channel of F = ones is the alpha map bit for bit.
  float T = 1.0f;
  bool first = true;
  float S[FEAT_GROUP], R[FEAT_GROUP];
#pragma unroll
  for (int j = 0; j < FEAT_GROUP; ++j) S[j] = R[j] = 0.0f;
  for (uint32_t base = 0; base < tmax; base += MAP_CHUNK) {
    const uint32_t n = min((uint32_t)MAP_CHUNK, tmax - base);
    if ((uint32_t)tid < n) {
      const MapEntry e = load_entry(rec, point_list[m.start + base + tid]);
      float f[FEAT_GROUP];
      feat_load_row(F, C, c0, e.id, f);
      sA[tid] = e.lr.A;
      sB[tid] = e.lr.B;
      sF0[tid] = make_float4(f[0], f[1], f[2], f[3]);
      sF1[tid] = make_float4(f[4], f[5], f[6], f[7]);
    }
    __syncthreads();
    const uint32_t mine = last > base ? min(n, last - base) : 0u;
    for (uint32_t k = 0; k < mine; ++k) {
      const float4 a = sA[k], b = sB[k];
      const float alpha = map_alpha(a, b, pxf, pyf);
      if (alpha >= ALPHA_MIN) {
        const float4 f0 = sF0[k], f1 = sF1[k];
        const float f[FEAT_GROUP] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
        const float w = alpha * T;
#pragma unroll
        for (int j = 0; j < FEAT_GROUP; ++j) {
          R[j] = first ? f[j] : R[j];
          S[j] = __builtin_fmaf(f[j] - R[j], w, S[j]);
        }
        first = false;
        T = __builtin_fmaf(-alpha, T, T);      // T (1 - alpha), rounded once: the colour pass's update
      }
    }
    __syncthreads();
  }
  if (m.inside) {
    const float cover = 1.0f - T;      // the alpha map of depth.hip: T is the colour pass's final T
#pragma unroll
    for (int j = 0; j < FEAT_GROUP; ++j)
      if (c0 + j < C) out[(size_t)(c0 + j) * HW + pix] = __builtin_fmaf(R[j], cover, S[j]);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Backward: same grid and staging, back to front from the pixel's final T (final_T of the frame).  The recurrence of
// map_walk.h (map_bwd_test, map_bwd_advance, map_bwd_dalpha) with the entry's channel values c_i = F[id_i, c0 .. c0 + 7] and g the
// incoming gradient of the pixel's channels of this group.
// dL/dalpha_i is LINEAR in c . g = sum_c F[id_i, c] g[c]: the recurrence run on a subset of the channels gives that
// subset's share of dL/dalpha_i, and the shares of disjoint subsets add up to the whole.  So every channel group runs
// the recurrence on its own channels and adds its six geometry sums (geom_terms) into the SAME [P,8] accumulator: that
// is what makes the grouping legal.  (Word 6, d z, is never written.)
// Per entry and channel, sum over the tile's pixels of w_i g[c] is dL/dF[id_i, c]: one float atomic per
// (entry, tile, channel) into dL_dF [P,C].  All sums are added across the wave with shuffles and across the four waves
// in LDS; the lane that staged the entry issues the global atomics.  A wave none of whose pixels the entry reaches
// skips the entry.  GEOM / FEAT: which of the two sides the caller wants.
// ------------------------------------------------------------------------------------------------------------------
template <bool GEOM, bool FEAT>
__global__ __launch_bounds__(MAP_CHUNK) void feature_maps_bwd_kernel(int W, int H, int grid_x,
                                                                     const uint32_t* __restrict__ tile_order,
                                                                     const uint2* __restrict__ ranges,
                                                                     const uint32_t* __restrict__ point_list,
                                                                     const GeomRec* __restrict__ rec,
                                                                     const uint32_t* __restrict__ n_contrib,
                                                                     const float* __restrict__ final_T,
                                                                     const float* __restrict__ F, int C,
                                                                     const float* __restrict__ dL_dmaps,
                                                                     float* __restrict__ acc, float* __restrict__ dL_dF) {
  constexpr int NSUM = (GEOM ? MAP_GEOM : 0) + (FEAT ? FEAT_GROUP : 0);
  constexpr int FEAT0 = GEOM ? MAP_GEOM : 0;      // first channel sum
  __shared__ float4 sA[MAP_CHUNK];
  __shared__ float4 sB[MAP_CHUNK];
  __shared__ float4 sF0[MAP_CHUNK];
  __shared__ float4 sF1[MAP_CHUNK];
  __shared__ float sSum[NSUM][MAP_CHUNK];
  __shared__ uint32_t sMax[4];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int c0 = (int)blockIdx.y * FEAT_GROUP;
  const int nch = min(FEAT_GROUP, C - c0);      // channels of this group that exist
  const MapPixel m = map_pixel(W, H, grid_x, tile_order, ranges);
  const bool inside = m.inside;
  const size_t pix = m.pix, HW = (size_t)W * H;
  const float pxf = (float)m.px, pyf = (float)m.py;
  const uint32_t last = map_last(m, n_contrib, inside);
  const uint32_t tmax = block_max_u32(last, sMax);
  float T = inside ? final_T[pix] : 0.0f;
  float g[FEAT_GROUP];
#pragma unroll
  for (int j = 0; j < FEAT_GROUP; ++j) g[j] = (inside && j < nch) ? dL_dmaps[(size_t)(c0 + j) * HW + pix] : 0.0f;
  float U = 0.0f;

  uint32_t hi = tmax;
  while (hi > 0) {
    const uint32_t lo = hi > (uint32_t)MAP_CHUNK ? hi - MAP_CHUNK : 0u;
    const uint32_t n = hi - lo;
    MapEntry e;
    if ((uint32_t)tid < n) {
      e = load_entry(rec, point_list[m.start + lo + tid]);
      float f[FEAT_GROUP];
      feat_load_row(F, C, c0, e.id, f);
      sA[tid] = e.lr.A;
      sB[tid] = e.lr.B;
      sF0[tid] = make_float4(f[0], f[1], f[2], f[3]);
      sF1[tid] = make_float4(f[4], f[5], f[6], f[7]);
    }
#pragma unroll
    for (int q = 0; q < NSUM; ++q) sSum[q][tid] = 0.0f;
    __syncthreads();
    for (uint32_t k = n; k-- > 0;) {
      const float4 b = sB[k];
      MapStep st = map_bwd_test(sA[k], b, pxf, pyf, lo + k < last);
      if (__builtin_amdgcn_ballot_w64(st.ok) == 0ull) continue;      // uniform over the wave
      map_bwd_advance(st, b, T);
      if (GEOM) {
        const float4 f0 = sF0[k], f1 = sF1[k];
        float cg = f0.x * g[0];
        cg = __builtin_fmaf(f0.y, g[1], cg);
        cg = __builtin_fmaf(f0.z, g[2], cg);
        cg = __builtin_fmaf(f0.w, g[3], cg);
        cg = __builtin_fmaf(f1.x, g[4], cg);
        cg = __builtin_fmaf(f1.y, g[5], cg);
        cg = __builtin_fmaf(f1.z, g[6], cg);
        cg = __builtin_fmaf(f1.w, g[7], cg);
        const float h = map_bwd_dalpha(st, T, cg, U);
        float v[MAP_GEOM];
        geom_terms(h, st.dx, st.dy, v);
        map_add_sums(v, sSum, k, lane);
      }
      if (FEAT) {
        const float w = st.am * T;
#pragma unroll
        for (int j = 0; j < FEAT_GROUP; ++j)
          if (j < nch) map_add_sum(w * g[j], &sSum[FEAT0 + j][k], lane);      // uniform over the workgroup
      }
    }
    __syncthreads();
    if ((uint32_t)tid < n) {
      if (GEOM) map_flush_acc<MAP_GEOM>(sSum, tid, e, acc);
      if (FEAT) {
        float* row = dL_dF + (size_t)e.id * (size_t)C + c0;
#pragma unroll
        for (int j = 0; j < FEAT_GROUP; ++j) {
          if (j < nch) {
            const float s = sSum[FEAT0 + j][tid];
            if ((__float_as_uint(s) << 1) != 0u) atomicAdd(row + j, s);
          }
        }
      }
    }
    __syncthreads();
    hi = lo;
  }
}

void launch_feature_maps_fwd(const MapFrame& f, const float* features, int C, float* out, hipStream_t s) {
  hipLaunchKernelGGL(feature_maps_fwd_kernel, dim3(f.tiles, (C + FEAT_GROUP - 1) / FEAT_GROUP), dim3(MAP_CHUNK), 0, s, f.W,
                     f.H, f.grid_x, f.tile_order, f.ranges, f.point_list, f.rec, f.n_contrib, features, C, out);
}

void launch_feature_maps_bwd(const MapFrame& f, const float* features, int C, const float* dL_dmaps, float* acc,
                             float* dL_dfeatures, hipStream_t s) {
  const dim3 grid(f.tiles, (C + FEAT_GROUP - 1) / FEAT_GROUP), block(MAP_CHUNK);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, s, f.W, f.H, f.grid_x, f.tile_order, f.ranges, f.point_list, f.rec,
                       f.n_contrib, f.final_T, features, C, dL_dmaps, acc, dL_dfeatures);
  };
  if (acc && dL_dfeatures) launch(feature_maps_bwd_kernel<true, true>);
  else if (acc) launch(feature_maps_bwd_kernel<true, false>);
  else if (dL_dfeatures) launch(feature_maps_bwd_kernel<false, true>);
}

}  // namespace gsr

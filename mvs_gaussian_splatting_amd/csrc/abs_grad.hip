// The absolute ("homodirectional") view-space gradient of AbsGS for a rendered frame: per Gaussian k,
//
//   abs_x[k] = 0.5 W sum_p | h_kp (cxx dx + cxy dy) |,   abs_y[k] = 0.5 H sum_p | h_kp (cxy dx + cyy dy) |,
//
// p over the pixels whose colour pass composited k (the entries of depth.hip, §7.9: the first n_contrib[p] entries of
// the tile's list that pass alpha >= 1/255), d = mean2D_k - p and h_kp = opacity_k G_kp dL/dalpha_kp of the COLOUR
// image.  The signed sum of the same terms, times -1, is GsrGrads.dL_dmeans2D: render_bwd adds a Gaussian's terms over
// a tile before it writes them, so the sign of a term is gone where its output starts, and the quantity needs a walk
// of its own.
//
// It is the walk the map backwards share (map_walk.h) with the Gaussian's colour as the three channels -- (r, g, b) of
// GeomRec, the clamped colour the forward composited -- and the background behind the last entry: the recurrence's U
// starts at bg . g, which is the colour backward's background term -T_final / (1 - alpha) (bg . g) once multiplied out.
// Grid, staging and reduction are those of features.hip's geometry-only backward with two sums per entry where that has
// six: across the wave with shuffles, across the four waves in LDS, and the lane that staged the entry issues at most
// two float atomic adds into the Gaussian's row (none when both sums are zero).  Nothing of the colour path is
// read-modified.  Atomics reorder: the result is reproducible to rounding, not bit for bit.
//
// Built with the flags of features.o.
#include "gsr_common.h"
#include "gsr_launch.h"
#include "map_walk.h"

namespace gsr {

__global__ __launch_bounds__(MAP_CHUNK) void abs_grad_bwd_kernel(int W, int H, int grid_x,
                                                                 const uint32_t* __restrict__ tile_order,
                                                                 const uint2* __restrict__ ranges,
                                                                 const uint32_t* __restrict__ point_list,
                                                                 const GeomRec* __restrict__ rec,
                                                                 const uint32_t* __restrict__ n_contrib,
                                                                 const float* __restrict__ final_T,
                                                                 const float* __restrict__ bg,
                                                                 const float* __restrict__ dL_dcolor,
                                                                 float* __restrict__ abs_means2D) {
  __shared__ float4 sA[MAP_CHUNK];
  __shared__ float4 sB[MAP_CHUNK];       // .z, .w: r, g
  __shared__ float4 sC[MAP_CHUNK];       // cxx, cxy, cyy, b
  __shared__ float sSum[2][MAP_CHUNK];
  __shared__ uint32_t sMax[4];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const MapPixel m = map_pixel(W, H, grid_x, tile_order, ranges);
  const bool inside = m.inside;      // a pixel of a partial tile outside the image takes no part: last = 0, g = 0
  const size_t pix = m.pix, HW = (size_t)W * H;
  const float pxf = (float)m.px, pyf = (float)m.py;
  const uint32_t last = map_last(m, n_contrib, inside);
  const uint32_t tmax = block_max_u32(last, sMax);
  float T = inside ? final_T[pix] : 0.0f;
  const float g0 = inside ? dL_dcolor[pix] : 0.0f;
  const float g1 = inside ? dL_dcolor[HW + pix] : 0.0f;
  const float g2 = inside ? dL_dcolor[2 * HW + pix] : 0.0f;
  float U = __builtin_fmaf(bg[2], g2, __builtin_fmaf(bg[1], g1, bg[0] * g0));      // the background, behind the last entry

  uint32_t hi = tmax;
  while (hi > 0) {
    const uint32_t lo = hi > (uint32_t)MAP_CHUNK ? hi - MAP_CHUNK : 0u;
    const uint32_t n = hi - lo;
    uint32_t id = 0u;
    if ((uint32_t)tid < n) {
      id = point_list[m.start + lo + tid];
      const MapEntry e = load_entry(rec, id);
      sA[tid] = e.lr.A;
      sB[tid] = make_float4(e.lr.B.x, e.lr.B.y, rec[id].r, rec[id].g);
      sC[tid] = make_float4(e.cxx, e.cxy, e.cyy, rec[id].b);
    }
    sSum[0][tid] = 0.0f;
    sSum[1][tid] = 0.0f;
    __syncthreads();
    for (uint32_t k = n; k-- > 0;) {
      const float4 b = sB[k];
      MapStep st = map_bwd_test(sA[k], b, pxf, pyf, lo + k < last);
      if (__builtin_amdgcn_ballot_w64(st.ok) == 0ull) continue;      // uniform over the wave
      map_bwd_advance(st, b, T);
      const float4 c = sC[k];
      const float cg = __builtin_fmaf(c.w, g2, __builtin_fmaf(b.w, g1, b.z * g0));
      const float h = map_bwd_dalpha(st, T, cg, U);
      map_add_sum(fabsf(h * __builtin_fmaf(c.y, st.dy, c.x * st.dx)), &sSum[0][k], lane);
      map_add_sum(fabsf(h * __builtin_fmaf(c.z, st.dy, c.y * st.dx)), &sSum[1][k], lane);
    }
    __syncthreads();
    if ((uint32_t)tid < n) {
      const float sx = sSum[0][tid], sy = sSum[1][tid];      // sums of magnitudes: >= 0
      float* row = abs_means2D + 3 * (size_t)id;
      if (sx != 0.0f) atomicAdd(row + 0, 0.5f * (float)W * sx);      // GsrGrads.dL_dmeans2D's scale: NDC units times 0.5 W, 0.5 H
      if (sy != 0.0f) atomicAdd(row + 1, 0.5f * (float)H * sy);
    }
    __syncthreads();
    hi = lo;
  }
}

void launch_abs_grad_bwd(const MapFrame& f, const float* bg, const float* dL_dcolor, float* abs_means2D, hipStream_t s) {
  hipLaunchKernelGGL(abs_grad_bwd_kernel, dim3(f.tiles), dim3(MAP_CHUNK), 0, s, f.W, f.H, f.grid_x, f.tile_order, f.ranges,
                     f.point_list, f.rec, f.n_contrib, f.final_T, bg, dL_dcolor, abs_means2D);
}

}  // namespace gsr

// Depth-distortion map of a rendered frame (the regulariser of 2DGS), with gradients.
//
//   dist = sum_i sum_{j<i} w_i w_j (m_i - m_j)^2,   w_i = alpha_i T_i,   m_i = m(z_i)
//   m(z) = z                                 mapping 0 ("linear")
//   m(z) = far / (far - near) (1 - near / z)  mapping 1 (the NDC depth 2DGS uses)
//
// over the list entries the colour pass composited at the pixel -- the entries of depth.hip (§7.9): the first
// n_contrib[pixel] entries of the tile's list whose alpha passes the 1/255 test, alpha evaluated and T updated by the
// walk the maps share (map_walk.h), so the decisions and the running T come out bit for bit.
// z_i is BinInfo::depth.  No background term; a pixel with zero or one contributor is exactly 0.
//
// In exact arithmetic dist = A M2 - M1^2 (A = sum w, M1 = sum w m, M2 = sum w m^2), but in float32 that subtraction cancels
// whenever the pixel's contributors lie in a thin slab -- the state the loss drives towards.  Both kernels therefore
// carry differences of m only.  Forward, per composited entry, with d = m_i - m_prev (0 at the first entry):
//     Q += d (2 S + d A);   S += d A;   dist += w_i Q;   A += w_i
// where S_i = sum_{j<i} w_j (m_i - m_j) and Q_i = sum_{j<i} w_j (m_i - m_j)^2; the identities hold for either sign of d.
//
// state [2,H,W], written by the forward for the backward (opaque to the caller), with cover = 1 - T_final:
//     state[0] = S_end / cover = m_last - mbar      (mbar = M1 / A; 0 without a contributor)
//     state[1] = dist / cover                       (0 without a contributor)
// Backward, back to front: r_k = m_k - mbar starts at state[0] and steps by r <- r - (m_next - m_k);
//     d dist / d w_k = E_k = A r_k^2 + dist / A,      d dist / d m_k = 2 w_k A r_k,
// and dL/dalpha_k is the recurrence of map_walk.h (map_bwd_dalpha) with g E_k as the entry's channel value.  Every
// quantity is of the order of the contributors' spread, never of m itself.
//
// Nothing of the colour path or of depth.hip is read-modified; the backward's sums go into a zeroed [P,8] accumulator in
// the layout aux_geom_bwd_kernel reads (word 6 is d z).  Nothing waits on another workgroup.
//
// Built with the flags of depth.o; the arithmetic that has to match the colour pass, and the recurrences, are explicit fma.
#include "gsr_common.h"
#include "gsr_launch.h"
#include "map_walk.h"

namespace gsr {

constexpr int DIST_SUMS = MAP_GEOM + 1;      // per-entry sums of the backward: the geometry sums and d z

// m(z) and m'(z) of a list entry's depth (scale = far / (far - near))
__device__ inline float2 dist_depth(float z, int mapping, float near, float scale) {
  float2 md;
  if (mapping == 0) {
    md = make_float2(z, 1.0f);
  } else {
    const float iz = 1.0f / z;
    md = make_float2(scale * (1.0f - near * iz), scale * near * iz * iz);
  }
  return md;
}

// ------------------------------------------------------------------------------------------------------------------
// Forward: one 256-lane workgroup per tile (the colour pass's tile order), one lane per pixel.  A round stages up to 256
// entries in LDS; every lane then walks the round's entries in list order up to ITS n_contrib.  No atomics: the map is
// the same bits from run to run.  A tile with an empty list writes zeros.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_CHUNK) void distortion_fwd_kernel(int W, int H, int grid_x,
                                                                   const uint32_t* __restrict__ tile_order,
                                                                   const uint2* __restrict__ ranges,
                                                                   const uint32_t* __restrict__ point_list,
                                                                   const GeomRec* __restrict__ rec,
                                                                   const BinInfo* __restrict__ bin,
                                                                   const uint32_t* __restrict__ n_contrib, int mapping,
                                                                   float near, float scale, float* __restrict__ dist,
                                                                   float* __restrict__ state) {
  __shared__ float4 sA[MAP_CHUNK];
  __shared__ float4 sB[MAP_CHUNK];
  __shared__ float sM[MAP_CHUNK];
  __shared__ uint32_t sMax[4];
  const int tid = threadIdx.x;
  const MapPixel m = map_pixel(W, H, grid_x, tile_order, ranges);
  const size_t pix = m.pix, HW = (size_t)W * H;
  const float pxf = (float)m.px, pyf = (float)m.py;
  const uint32_t last = map_last(m, n_contrib, m.inside);
  const uint32_t tmax = block_max_u32(last, sMax);

  float T = 1.0f, A = 0.0f, S = 0.0f, Q = 0.0f, D = 0.0f, mp = 0.0f;
  bool first = true;
  for (uint32_t base = 0; base < tmax; base += MAP_CHUNK) {
    const uint32_t n = min((uint32_t)MAP_CHUNK, tmax - base);
    if ((uint32_t)tid < n) {
      const MapEntry e = load_entry(rec, point_list[m.start + base + tid]);
      const float2 md = dist_depth(bin[e.id].depth, mapping, near, scale);
      sA[tid] = e.lr.A;
      sB[tid] = e.lr.B;
      sM[tid] = md.x;
    }
    __syncthreads();
    const uint32_t mine = last > base ? min(n, last - base) : 0u;
    for (uint32_t k = 0; k < mine; ++k) {
      const float4 a = sA[k], b = sB[k];
      const float alpha = map_alpha(a, b, pxf, pyf);
      if (alpha >= ALPHA_MIN) {
        const float mk = sM[k];
        const float w = alpha * T;
        const float d = first ? 0.0f : mk - mp;
        Q = __builtin_fmaf(d, __builtin_fmaf(d, A, 2.0f * S), Q);      // Q += d (2 S + d A), with the S and A of j < i
        S = __builtin_fmaf(d, A, S);
        D = __builtin_fmaf(w, Q, D);
        A += w;
        mp = mk;
        first = false;
        T = __builtin_fmaf(-alpha, T, T);      // T (1 - alpha), rounded once: the colour pass's update
      }
    }
    __syncthreads();
  }
  if (m.inside) {
    const float cover = 1.0f - T;      // the alpha map of depth.hip; the backward forms the same number from final_T
    const bool any = cover > 0.0f;
    dist[pix] = D;
    state[pix] = any ? S / cover : 0.0f;
    state[HW + pix] = any ? D / cover : 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Backward: same grid and staging, back to front from the pixel's final T (final_T of the frame).  With g the incoming
// gradient of the pixel, A = 1 - final_T and r_k = m_k - mbar (header comment), the entry's "channel value" is
//    c_k = g E_k = g (A r_k^2 + dist / A)
// in the recurrence of map_walk.h, and dL/dz_k = g 2 w_k A r_k m'(z_k).  Per entry the six geometry sums (geom_terms)
// and sum dL/dz over the tile's pixels go through map_add_sums and map_flush_acc into acc[P][8].
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_CHUNK) void distortion_bwd_kernel(int W, int H, int grid_x,
                                                                   const uint32_t* __restrict__ tile_order,
                                                                   const uint2* __restrict__ ranges,
                                                                   const uint32_t* __restrict__ point_list,
                                                                   const GeomRec* __restrict__ rec,
                                                                   const BinInfo* __restrict__ bin,
                                                                   const uint32_t* __restrict__ n_contrib,
                                                                   const float* __restrict__ final_T, int mapping,
                                                                   float near, float scale,
                                                                   const float* __restrict__ state,
                                                                   const float* __restrict__ dL_ddist,
                                                                   float* __restrict__ acc) {
  __shared__ float4 sA[MAP_CHUNK];
  __shared__ float4 sB[MAP_CHUNK];
  __shared__ float2 sM[MAP_CHUNK];      // m, m'
  __shared__ float sSum[DIST_SUMS][MAP_CHUNK];
  __shared__ uint32_t sMax[4];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const MapPixel m = map_pixel(W, H, grid_x, tile_order, ranges);
  const bool inside = m.inside;
  const size_t pix = m.pix, HW = (size_t)W * H;
  const float pxf = (float)m.px, pyf = (float)m.py;
  const uint32_t last = map_last(m, n_contrib, inside);
  const uint32_t tmax = block_max_u32(last, sMax);
  float T = inside ? final_T[pix] : 0.0f;
  const float A = inside ? 1.0f - T : 0.0f;
  const float g = inside ? dL_ddist[pix] : 0.0f;
  const float E0 = inside ? state[HW + pix] : 0.0f;      // dist / A
  float r = inside ? state[pix] : 0.0f;                  // m_k - mbar of the entry last visited
  float mn = 0.0f;                                       // its m
  bool seen = false;
  float U = 0.0f;

  uint32_t hi = tmax;
  while (hi > 0) {
    const uint32_t lo = hi > (uint32_t)MAP_CHUNK ? hi - MAP_CHUNK : 0u;
    const uint32_t n = hi - lo;
    MapEntry e;
    if ((uint32_t)tid < n) {
      e = load_entry(rec, point_list[m.start + lo + tid]);
      const float2 md = dist_depth(bin[e.id].depth, mapping, near, scale);
      sA[tid] = e.lr.A;
      sB[tid] = e.lr.B;
      sM[tid] = md;
    }
#pragma unroll
    for (int q = 0; q < DIST_SUMS; ++q) sSum[q][tid] = 0.0f;
    __syncthreads();
    for (uint32_t k = n; k-- > 0;) {
      const float4 b = sB[k];
      MapStep st = map_bwd_test(sA[k], b, pxf, pyf, lo + k < last);
      if (__builtin_amdgcn_ballot_w64(st.ok) == 0ull) continue;      // uniform over the wave
      const float2 mz = sM[k];
      map_bwd_advance(st, b, T);
      // a lane the entry does not reach keeps its r, as it keeps its T and U
      r -= (st.ok && seen) ? mn - mz.x : 0.0f;               // the first entry visited is the last composited: r = state[0]
      mn = st.ok ? mz.x : mn;
      seen = seen || st.ok;
      const float Ar = A * r;
      const float h = map_bwd_dalpha(st, T, g * __builtin_fmaf(Ar, r, E0), U);
      float v[DIST_SUMS];
      geom_terms(h, st.dx, st.dy, v);
      v[6] = st.am * T * (2.0f * g * Ar * mz.y);
      map_add_sums(v, sSum, k, lane);
    }
    __syncthreads();
    if ((uint32_t)tid < n) map_flush_acc<DIST_SUMS>(sSum, tid, e, acc);
    __syncthreads();
    hi = lo;
  }
}

void launch_distortion_fwd(const MapFrame& f, int mapping, float near, float far, float* dist, float* state, hipStream_t s) {
  const float scale = mapping ? far / (far - near) : 1.0f;
  hipLaunchKernelGGL(distortion_fwd_kernel, dim3(f.tiles), dim3(MAP_CHUNK), 0, s, f.W, f.H, f.grid_x, f.tile_order, f.ranges,
                     f.point_list, f.rec, f.bin, f.n_contrib, mapping, near, scale, dist, state);
}

void launch_distortion_bwd(const MapFrame& f, int mapping, float near, float far, const float* state, const float* dL_ddist,
                           float* acc, hipStream_t s) {
  const float scale = mapping ? far / (far - near) : 1.0f;
  hipLaunchKernelGGL(distortion_bwd_kernel, dim3(f.tiles), dim3(MAP_CHUNK), 0, s, f.W, f.H, f.grid_x, f.tile_order, f.ranges,
                     f.point_list, f.rec, f.bin, f.n_contrib, f.final_T, mapping, near, scale, state, dL_ddist, acc);
}

}  // namespace gsr

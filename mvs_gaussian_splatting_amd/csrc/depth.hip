// Depth, inverse-depth and accumulated-opacity maps of a rendered frame, with gradients.
//
//   depth = sum_i w_i z_i,   invdepth = sum_i w_i / z_i,   alpha = sum_i w_i = 1 - T_final,   w_i = alpha_i T_i
//
// over the list entries the colour pass composited at the pixel: entries [range.start, range.start + n_contrib[pixel])
// whose alpha passes the 1/255 test.  Inside that prefix every such entry also passed the colour pass's T test (the pixel
// was not saturated yet), so the prefix and the alpha test ARE the colour pass's decisions; alpha is evaluated with the
// colour pass's own functions (render_pair.h), so the tests and the running T come out bit for bit.  There is no
// background term.  z_i is BinInfo::depth, the view-space depth the lists are sorted by.
//
// Three kernels of their own; nothing of the colour path is read-modified: the forward reads the frame's saved state,
// the backward adds into a zeroed [P,8] accumulator of its own (never the colour path's gradient rows), and a
// per-Gaussian kernel takes the accumulator to the inputs.  Simple mappings (one lane per pixel, one LDS broadcast per
// list entry): these maps are an optional second output, not the flagship path.
//
// Built with -ffp-contract=off like preprocess.hip: aux_geom_bwd_kernel recomputes the projection and must get the
// values (and the guard-band decisions) of preprocess_fwd_kernel.  The compositing arithmetic that has to match the
// colour pass is written with explicit fma.
#include "gsr_common.h"
#include "gsr_launch.h"
#include "map_walk.h"
#include "preprocess_geom.h"

namespace gsr {

constexpr int AUX_SUMS = MAP_GEOM + 1;      // per-entry sums of the backward: the geometry sums and d z

// ------------------------------------------------------------------------------------------------------------------
// Forward: one 256-lane workgroup per tile (the colour pass's tile order: longest list first), one lane per pixel.
// A round stages up to 256 entries in LDS; every lane then walks the round's entries in list order up to ITS
// n_contrib.  No early-out of its own: how far a pixel walks was decided by the colour pass.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_CHUNK) void aux_maps_fwd_kernel(int W, int H, int grid_x,
                                                                 const uint32_t* __restrict__ tile_order,
                                                                 const uint2* __restrict__ ranges,
                                                                 const uint32_t* __restrict__ point_list,
                                                                 const GeomRec* __restrict__ rec,
                                                                 const BinInfo* __restrict__ bin,
                                                                 const uint32_t* __restrict__ n_contrib,
                                                                 float* __restrict__ out) {
  __shared__ float4 sA[MAP_CHUNK];
  __shared__ float4 sB[MAP_CHUNK];
  __shared__ float2 sZ[MAP_CHUNK];      // z, 1 / z
  __shared__ uint32_t sMax[4];
  const int tid = threadIdx.x;
  const MapPixel m = map_pixel(W, H, grid_x, tile_order, ranges);
  const size_t pix = m.pix, HW = (size_t)W * H;
  const float pxf = (float)m.px, pyf = (float)m.py;
  const uint32_t last = map_last(m, n_contrib, m.inside);
  const uint32_t tmax = block_max_u32(last, sMax);

  float T = 1.0f, D = 0.0f, I = 0.0f;
  for (uint32_t base = 0; base < tmax; base += MAP_CHUNK) {
    const uint32_t n = min((uint32_t)MAP_CHUNK, tmax - base);
    if ((uint32_t)tid < n) {
      const MapEntry e = load_entry(rec, point_list[m.start + base + tid]);
      const float z = bin[e.id].depth;
      sA[tid] = e.lr.A;
      sB[tid] = e.lr.B;
      sZ[tid] = make_float2(z, 1.0f / z);
    }
    __syncthreads();
    const uint32_t mine = last > base ? min(n, last - base) : 0u;
    for (uint32_t k = 0; k < mine; ++k) {
      const float4 a = sA[k], b = sB[k];
      const float alpha = map_alpha(a, b, pxf, pyf);
      if (alpha >= ALPHA_MIN) {
        const float2 z = sZ[k];
        const float w = alpha * T;
        D = __builtin_fmaf(z.x, w, D);
        I = __builtin_fmaf(z.y, w, I);
        T = __builtin_fmaf(-alpha, T, T);      // T (1 - alpha), rounded once: the colour pass's update
      }
    }
    __syncthreads();
  }
  if (m.inside) {
    out[pix] = D;
    out[HW + pix] = I;
    out[2 * HW + pix] = 1.0f - T;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Backward: same grid and staging, back to front from the pixel's final T (final_T of the frame: the forward above
// reproduces it bit for bit).  Upstream's recurrence with the channel values c_i = (z_i, 1 / z_i, 1) and no background:
// with g the incoming gradient of the pixel's three maps, U = (sum over the entries behind of (c . g) w) / T,
//    D = c_i . g - U,   dL/dalpha_i = T_i D,   U <- U + alpha_i D,
// and dL/dz_i = w_i (g_depth - g_invdepth / z_i^2).  Per entry the seven sums over the tile's pixels
//    sum h dx, sum h dy, sum h dx^2, sum h dx dy, sum h dy^2, sum h, sum dL/dz      (h = opacity G dL/dalpha, d = mean - pixel)
// are added across the wave with shuffles and across the four waves in LDS; the lane that staged the entry turns them into
// d mean2D (pixels), d conic, d opacity and d z and issues one float atomic add per quantity into acc[P][8].  A wave none
// of whose pixels the entry reaches skips the entry.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_CHUNK) void aux_maps_bwd_kernel(int W, int H, int grid_x,
                                                                 const uint32_t* __restrict__ tile_order,
                                                                 const uint2* __restrict__ ranges,
                                                                 const uint32_t* __restrict__ point_list,
                                                                 const GeomRec* __restrict__ rec,
                                                                 const BinInfo* __restrict__ bin,
                                                                 const uint32_t* __restrict__ n_contrib,
                                                                 const float* __restrict__ final_T,
                                                                 const float* __restrict__ dL_dmaps,
                                                                 float* __restrict__ acc) {
  __shared__ float4 sA[MAP_CHUNK];
  __shared__ float4 sB[MAP_CHUNK];
  __shared__ float2 sZ[MAP_CHUNK];
  __shared__ float sSum[AUX_SUMS][MAP_CHUNK];
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
  const float g0 = inside ? dL_dmaps[pix] : 0.0f, g1 = inside ? dL_dmaps[HW + pix] : 0.0f,
              g2 = inside ? dL_dmaps[2 * HW + pix] : 0.0f;
  float U = 0.0f;

  uint32_t hi = tmax;
  while (hi > 0) {
    const uint32_t lo = hi > (uint32_t)MAP_CHUNK ? hi - MAP_CHUNK : 0u;
    const uint32_t n = hi - lo;
    MapEntry e;
    if ((uint32_t)tid < n) {
      e = load_entry(rec, point_list[m.start + lo + tid]);
      const float z = bin[e.id].depth;
      sA[tid] = e.lr.A;
      sB[tid] = e.lr.B;
      sZ[tid] = make_float2(z, 1.0f / z);
    }
#pragma unroll
    for (int q = 0; q < AUX_SUMS; ++q) sSum[q][tid] = 0.0f;
    __syncthreads();
    for (uint32_t k = n; k-- > 0;) {
      const float4 b = sB[k];
      MapStep st = map_bwd_test(sA[k], b, pxf, pyf, lo + k < last);
      if (__builtin_amdgcn_ballot_w64(st.ok) == 0ull) continue;      // uniform over the wave
      const float2 z = sZ[k];
      map_bwd_advance(st, b, T);
      const float cg = __builtin_fmaf(z.x, g0, __builtin_fmaf(z.y, g1, g2));
      const float h = map_bwd_dalpha(st, T, cg, U);
      float v[AUX_SUMS];
      geom_terms(h, st.dx, st.dy, v);
      v[6] = st.am * T * (g0 - g1 * z.y * z.y);
      map_add_sums(v, sSum, k, lane);
    }
    __syncthreads();
    if ((uint32_t)tid < n) map_flush_acc<AUX_SUMS>(sSum, tid, e, acc);
    __syncthreads();
    hi = lo;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Per Gaussian (radii > 0 only): accumulator -> conic -> cov2D -> (J, W) -> cov3D / mean -> scales, rotations (or
// cov3D_precomp), d mean2D through the projection, d z through the view matrix's third column.  The steps and the
// guard-band masks are preprocess_bwd_kernel's (Appendix A.6 (i)-(iii), (v)); there is no colour and no SH here.
// Every output row is written in full.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PRE_BLOCK) void aux_geom_bwd_kernel(GsrParams p, const int32_t* __restrict__ radii,
                                                                 const float* __restrict__ acc, float* __restrict__ d_means3D,
                                                                 float* __restrict__ d_means2D, float* __restrict__ d_opacities,
                                                                 float* __restrict__ d_scales, float* __restrict__ d_rotations,
                                                                 float* __restrict__ d_cov3D) {
  const int idx = blockIdx.x * PRE_BLOCK + threadIdx.x;
  if (idx >= p.P) return;
  float dmean[3] = {0.f, 0.f, 0.f};
  float dm2x = 0.f, dm2y = 0.f, dop = 0.f;
  float dcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float dscale[3] = {0.f, 0.f, 0.f};
  float drot[4] = {0.f, 0.f, 0.f, 0.f};
  float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bool active = false;
  if (radii[idx] > 0) {
    const float4* r4 = reinterpret_cast<const float4*>(acc + 8 * (size_t)idx);
    const float4 u = r4[0], w = r4[1];
    a8[0] = u.x; a8[1] = u.y; a8[2] = u.z; a8[3] = u.w; a8[4] = w.x; a8[5] = w.y; a8[6] = w.z;
    uint32_t bits = 0u;
#pragma unroll
    for (int k = 0; k < 7; ++k) bits |= __float_as_uint(a8[k]);
    active = (bits << 1) != 0u;
  }
  if (active) {
    const float dcxx = a8[2], dcxy = a8[3], dcyy = a8[4], dz = a8[6];
    dop = a8[5];
    dm2x = 0.5f * (float)p.width * a8[0];       // the colour path's convention: NDC units scaled by 0.5 W, 0.5 H
    dm2y = 0.5f * (float)p.height * a8[1];

    Mat4 V, Mx;
    load_mat(p.viewmatrix, V);
    load_mat(p.projmatrix, Mx);
    const float px = p.means3D[3 * (size_t)idx + 0], py = p.means3D[3 * (size_t)idx + 1],
                pz = p.means3D[3 * (size_t)idx + 2];
    const float vx = V.m[0] * px + V.m[4] * py + V.m[8] * pz + V.m[12];
    const float vy = V.m[1] * px + V.m[5] * py + V.m[9] * pz + V.m[13];
    const float vz = V.m[2] * px + V.m[6] * py + V.m[10] * pz + V.m[14];

    float cov[6];
    float4 q4 = make_float4(1.f, 0.f, 0.f, 0.f);
    float sc[3] = {0.f, 0.f, 0.f};
    Activated act;
    act.qn = 1.0f;
    if (p.cov3D_precomp) {
#pragma unroll
      for (int k = 0; k < 6; ++k) cov[k] = p.cov3D_precomp[6 * (size_t)idx + k];
    } else {
      load_scale_rot(p, idx, act);
      q4 = act.q;
      sc[0] = act.sc[0]; sc[1] = act.sc[1]; sc[2] = act.sc[2];
      cov3d_from_scale_rot(sc[0], sc[1], sc[2], p.scale_modifier, q4.x, q4.y, q4.z, q4.w, cov);
    }
    const float fx = (float)p.width / (2.0f * p.tan_fovx), fy = (float)p.height / (2.0f * p.tan_fovy);
    const float limx = FOV_GUARD * p.tan_fovx, limy = FOV_GUARD * p.tan_fovy;
    Proj pr;
    project_cov(V, vx, vy, vz, cov, fx, fy, limx, limy, pr);

    // (i) conic -> cov2D (true-derivative convention for dcxy; 1e-7 as upstream)
    const float a = pr.a, b = pr.b, c = pr.c;
    const float den = a * c - b * b;
    const float k2 = 1.0f / (den * den + 0.0000001f);
    const float dL_da = k2 * (-c * c * dcxx + b * c * dcxy + (den - a * c) * dcyy);
    const float dL_dc = k2 * (-a * a * dcyy + a * b * dcxy + (den - a * c) * dcxx);
    const float dL_db = k2 * (2.0f * b * c * dcxx - (den + 2.0f * b * b) * dcxy + 2.0f * a * b * dcyy);

    // (ii) cov2D = A S A^T -> dS (6 unique) and dA
    const float* A0 = pr.A0;
    const float* A1 = pr.A1;
    auto dS = [&](int j, int k) { return dL_da * A0[j] * A0[k] + dL_db * A0[j] * A1[k] + dL_dc * A1[j] * A1[k]; };
    dcov[0] = dS(0, 0);
    dcov[3] = dS(1, 1);
    dcov[5] = dS(2, 2);
    dcov[1] = dS(0, 1) + dS(1, 0);
    dcov[2] = dS(0, 2) + dS(2, 0);
    dcov[4] = dS(1, 2) + dS(2, 1);
    const float S[3][3] = {{cov[0], cov[1], cov[2]}, {cov[1], cov[3], cov[4]}, {cov[2], cov[4], cov[5]}};
    float SA0[3], SA1[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      SA0[j] = S[j][0] * A0[0] + S[j][1] * A0[1] + S[j][2] * A0[2];
      SA1[j] = S[j][0] * A1[0] + S[j][1] * A1[1] + S[j][2] * A1[2];
    }
    float dA0[3], dA1[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      dA0[j] = 2.0f * dL_da * SA0[j] + dL_db * SA1[j];
      dA1[j] = 2.0f * dL_dc * SA1[j] + dL_db * SA0[j];
    }
    float dj00 = 0.f, dj02 = 0.f, dj11 = 0.f, dj12 = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      dj00 += dA0[j] * V.m[4 * j + 0];
      dj02 += dA0[j] * V.m[4 * j + 2];
      dj11 += dA1[j] * V.m[4 * j + 1];
      dj12 += dA1[j] * V.m[4 * j + 2];
    }
    const float tz = pr.tz, tz2 = tz * tz, tz3 = tz2 * tz;
    const float xm = (pr.txtz < -limx || pr.txtz > limx) ? 0.0f : 1.0f;
    const float ym = (pr.tytz < -limy || pr.tytz > limy) ? 0.0f : 1.0f;
    const float dtx = -fx / tz2 * dj02;
    const float dty = -fy / tz2 * dj12;
    const float dvx = xm * dtx;
    const float dvy = ym * dty;
    // the view-space depth is also the maps' z: its gradient joins the covariance path's
    const float dvz = -fx / tz2 * dj00 - fy / tz2 * dj11 + (2.0f * fx * pr.tx) / tz3 * dj02 +
                      (2.0f * fy * pr.ty) / tz3 * dj12 + dz;
#pragma unroll
    for (int i = 0; i < 3; ++i) dmean[i] = V.m[4 * i + 0] * dvx + V.m[4 * i + 1] * dvy + V.m[4 * i + 2] * dvz;

    // (iii) mean2D (NDC units) -> mean3D through p_hom / (w + 1e-7)
    {
      const float hx = Mx.m[0] * px + Mx.m[4] * py + Mx.m[8] * pz + Mx.m[12];
      const float hy = Mx.m[1] * px + Mx.m[5] * py + Mx.m[9] * pz + Mx.m[13];
      const float hw = Mx.m[3] * px + Mx.m[7] * py + Mx.m[11] * pz + Mx.m[15];
      const float m_w = 1.0f / (hw + 0.0000001f);
      const float mul1 = hx * m_w * m_w, mul2 = hy * m_w * m_w;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        dmean[i] += (Mx.m[4 * i + 0] * m_w - Mx.m[4 * i + 3] * mul1) * dm2x +
                    (Mx.m[4 * i + 1] * m_w - Mx.m[4 * i + 3] * mul2) * dm2y;
      }
    }

    // (v) cov3D -> scale, rotation
    if (!p.cov3D_precomp) {
      const float mod = p.scale_modifier;
      const float qr = q4.x, qx = q4.y, qy = q4.z, qz = q4.w;
      const float s0 = mod * sc[0], s1 = mod * sc[1], s2 = mod * sc[2];
      const float R[3][3] = {{1.0f - 2.0f * (qy * qy + qz * qz), 2.0f * (qx * qy - qr * qz), 2.0f * (qx * qz + qr * qy)},
                             {2.0f * (qx * qy + qr * qz), 1.0f - 2.0f * (qx * qx + qz * qz), 2.0f * (qy * qz - qr * qx)},
                             {2.0f * (qx * qz - qr * qy), 2.0f * (qy * qz + qr * qx), 1.0f - 2.0f * (qx * qx + qy * qy)}};
      const float sv[3] = {s0, s1, s2};
      const float Gm[3][3] = {{dcov[0], 0.5f * dcov[1], 0.5f * dcov[2]},
                              {0.5f * dcov[1], dcov[3], 0.5f * dcov[4]},
                              {0.5f * dcov[2], 0.5f * dcov[4], dcov[5]}};
      float dLm[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k)
          dLm[i][k] = 2.0f * (Gm[i][0] * R[0][k] * sv[k] + Gm[i][1] * R[1][k] * sv[k] + Gm[i][2] * R[2][k] * sv[k]);
      float dR[3][3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          sum += dLm[i][k] * R[i][k];
          dR[i][k] = dLm[i][k] * sv[k];
        }
        dscale[k] = sum * mod;
      }
      drot[0] = 2.0f * (qz * (dR[1][0] - dR[0][1]) + qy * (dR[0][2] - dR[2][0]) + qx * (dR[2][1] - dR[1][2]));
      drot[1] = 2.0f * (qy * (dR[0][1] + dR[1][0]) + qz * (dR[0][2] + dR[2][0]) + qr * (dR[2][1] - dR[1][2])) -
                4.0f * qx * (dR[1][1] + dR[2][2]);
      drot[2] = 2.0f * (qx * (dR[0][1] + dR[1][0]) + qr * (dR[0][2] - dR[2][0]) + qz * (dR[1][2] + dR[2][1])) -
                4.0f * qy * (dR[0][0] + dR[2][2]);
      drot[3] = 2.0f * (qr * (dR[1][0] - dR[0][1]) + qx * (dR[0][2] + dR[2][0]) + qy * (dR[1][2] + dR[2][1])) -
                4.0f * qz * (dR[0][0] + dR[1][1]);
      // the fused activations, back to the raw parameters
      if (p.act_flags & GSR_ACT_SCALE_EXP) {
#pragma unroll
        for (int k = 0; k < 3; ++k) dscale[k] *= sc[k];
      }
      if (p.act_flags & GSR_ACT_ROT_NORMALIZE) {
        const float dot = qr * drot[0] + qx * drot[1] + qy * drot[2] + qz * drot[3];
        drot[0] = (drot[0] - qr * dot) / act.qn;
        drot[1] = (drot[1] - qx * dot) / act.qn;
        drot[2] = (drot[2] - qy * dot) / act.qn;
        drot[3] = (drot[3] - qz * dot) / act.qn;
      }
    }
    if (p.act_flags & GSR_ACT_OPACITY_SIGMOID) {
      const float o = p.opacities[idx];
      const float sg = 1.0f / (1.0f + expf(-o));
      dop *= sg * (1.0f - sg);
    }
  }

#pragma unroll
  for (int i = 0; i < 3; ++i) d_means3D[3 * (size_t)idx + i] = dmean[i];
  d_means2D[3 * (size_t)idx + 0] = dm2x;
  d_means2D[3 * (size_t)idx + 1] = dm2y;
  d_means2D[3 * (size_t)idx + 2] = 0.0f;
  d_opacities[idx] = dop;
  if (p.cov3D_precomp) {
    if (d_cov3D)
#pragma unroll
      for (int i = 0; i < 6; ++i) d_cov3D[6 * (size_t)idx + i] = dcov[i];
  } else {
    if (d_scales)
#pragma unroll
      for (int i = 0; i < 3; ++i) d_scales[3 * (size_t)idx + i] = dscale[i];
    if (d_rotations)
#pragma unroll
      for (int i = 0; i < 4; ++i) d_rotations[4 * (size_t)idx + i] = drot[i];
  }
}

void launch_aux_maps_fwd(const MapFrame& f, float* out, hipStream_t s) {
  hipLaunchKernelGGL(aux_maps_fwd_kernel, dim3(f.tiles), dim3(MAP_CHUNK), 0, s, f.W, f.H, f.grid_x, f.tile_order, f.ranges,
                     f.point_list, f.rec, f.bin, f.n_contrib, out);
}

void launch_aux_maps_bwd(const MapFrame& f, const float* dL_dmaps, float* acc, hipStream_t s) {
  hipLaunchKernelGGL(aux_maps_bwd_kernel, dim3(f.tiles), dim3(MAP_CHUNK), 0, s, f.W, f.H, f.grid_x, f.tile_order, f.ranges,
                     f.point_list, f.rec, f.bin, f.n_contrib, f.final_T, dL_dmaps, acc);
}

void launch_aux_geom_bwd(const GsrParams& p, const int32_t* radii, const float* acc, const GsrAuxGrads& g, hipStream_t s) {
  const int nb = (p.P + PRE_BLOCK - 1) / PRE_BLOCK;
  if (nb > 0)
    hipLaunchKernelGGL(aux_geom_bwd_kernel, dim3(nb), dim3(PRE_BLOCK), 0, s, p, radii, acc, g.dL_dmeans3D, g.dL_dmeans2D,
                       g.dL_dopacities, g.dL_dscales, g.dL_drotations, g.dL_dcov3D);
}

}  // namespace gsr

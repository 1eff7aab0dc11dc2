// The fork's grow / learned-split branch of render() (gaussian_renderer/__init__.py:91-253): per frame, "virtual"
// Gaussians are appended to the model before it is rasterized, and their gradients are folded back onto their sources.
//
//   plan   : per Gaussian  g = accum / denom (NaN -> 0);  big = max(exp(scaling)) > percent_dense * extent
//            grow mode  sel = |g| >= thr          (:94-96)          split mode  sel = |g| >= thr & big   (:190-194)
//            block scans (densify.hip's shape) give every selected Gaussian its virtual row j; src[j] = i
//            counts = {G, #(sel & big)}: the second one is the grow + learned-split case the reference cannot run (:185)
//   expand : out[r] = in[r] for r < P, in[src[r - P]] for the virtual rows (every raw-parameter array, bit copies), then
//            grow   xyz[P+j] = xyz[i] + dir * max(exp(scaling[i])) * d                                    (:97-113)
//            split  xyz[i]  = xyz[i] + R s,  xyz[P+j] = R (-s) + xyz[i],  scaling = raw - log(k) on both  (:202-244)
//   fold   : g[i] += g[P+j] on every array (each source has exactly one virtual row: a gather, no atomics), then the
//            chain rule through the direction, the distance, the max-scale and the split offsets / scales
//
// The per-Gaussian arithmetic keeps the reference's float32 operation order (built with -ffp-contract=off).
#include "gsr_common.h"
#include "gsr_entry.h"
#include "gsr_launch.h"
#include "grow_common.h"
#include "row_plan.h"

namespace gsr {

constexpr int GR_BLOCK = PRE_BLOCK;
constexpr int GR_WAVES = GR_BLOCK / WAVE;

// index of the largest of three scales; ties go to the lowest index (torch.max's CPU tie-break, :108 / :190)
__device__ inline int argmax3(float a, float b, float c) {
  int k = 0;
  float m = a;
  if (b > m) { m = b; k = 1; }
  if (c > m) k = 2;
  return k;
}

// dL/d(raw quaternion) from dL/dR (row-major 3x3), through build_rotation's normalisation
__device__ inline void build_rotation_backward(const Rot& r, const float* __restrict__ dR, float* __restrict__ dq) {
  const float w = r.w, x = r.x, y = r.y, z = r.z;
  const float gw = 2.f * (-z * dR[1] + y * dR[2] + z * dR[3] - x * dR[5] - y * dR[6] + x * dR[7]);
  const float gx = 2.f * (y * dR[1] + z * dR[2] + y * dR[3] - 2.f * x * dR[4] - w * dR[5] + z * dR[6] + w * dR[7] -
                          2.f * x * dR[8]);
  const float gy = 2.f * (-2.f * y * dR[0] + x * dR[1] + w * dR[2] + x * dR[3] + z * dR[5] - w * dR[6] + z * dR[7] -
                          2.f * y * dR[8]);
  const float gz = 2.f * (-2.f * z * dR[0] - w * dR[1] + x * dR[2] + w * dR[3] - 2.f * z * dR[4] + y * dR[5] +
                          x * dR[6] + y * dR[7]);
  // q = r / |r|:  dL/dr = (dL/dq - q (q . dL/dq)) / |r|
  const float dot = w * gw + x * gx + y * gy + z * gz;
  dq[0] = (gw - w * dot) / r.norm;
  dq[1] = (gx - x * dot) / r.norm;
  dq[2] = (gy - y * dot) / r.norm;
  dq[3] = (gz - z * dot) / r.norm;
}

// ---- plan ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GR_BLOCK) void grow_plan_kernel(int P, const float* __restrict__ accum,
                                                              const float* __restrict__ denom,
                                                              const float* __restrict__ scaling, float thr, float pde,
                                                              int split_mode, uint8_t* __restrict__ flags,
                                                              uint32_t* __restrict__ block_counts, int stride) {
  const int i = blockIdx.x * GR_BLOCK + threadIdx.x;
  uint8_t f = 0;
  if (i < P) {
    float g = accum[i] / denom[i];
    if (g != g) g = 0.0f;
    const float mx = fmaxf(fmaxf(expf(scaling[3 * i]), expf(scaling[3 * i + 1])), expf(scaling[3 * i + 2]));
    const bool big = mx > pde;
    bool sel = fabsf(g) >= thr;
    if (split_mode) sel = sel && big;
    f = (sel ? 1 : 0) | ((sel && big) ? 2 : 0);
    flags[i] = f;
  }
  block_count_classes<2>(f, block_counts, stride);
}

__global__ __launch_bounds__(GR_BLOCK) void grow_positions_kernel(int P, const uint8_t* __restrict__ flags,
                                                                   const uint32_t* __restrict__ block_offs,
                                                                   int32_t* __restrict__ vidx, int32_t* __restrict__ src,
                                                                   uint8_t* __restrict__ selected) {
  const int i = blockIdx.x * GR_BLOCK + threadIdx.x;
  int32_t j[1];      // the rank among the selected (class 0) alone: the virtual row
  block_rank_classes<1>(i < P ? flags[i] : 0, block_offs, 0, j);
  if (i >= P) return;
  vidx[i] = j[0];
  selected[i] = j[0] >= 0 ? 1 : 0;
  if (j[0] >= 0) src[j[0]] = i;       // j < G <= P
}

// ---- expand -------------------------------------------------------------------------------------------------------
struct RowArrays {
  const float* in[6];
  float* out[6];
  int width[6];
};

// blockIdx.y picks the array; element-wise over the [P+G, width] output
__global__ __launch_bounds__(256) void grow_expand_rows_kernel(RowArrays a, int P, int G, const int32_t* __restrict__ src) {
  const int k = blockIdx.y;
  const int w = a.width[k];
  if (w == 0) return;
  const size_t total = (size_t)(P + G) * w, base = (size_t)P * w;
  const float* __restrict__ in = a.in[k];
  float* __restrict__ out = a.out[k];
  const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  // the P original rows are one contiguous copy: 16-byte accesses when both ends are 16-byte aligned
  const bool vec = (((uintptr_t)in | (uintptr_t)out) & 15u) == 0;
  const size_t n4 = vec ? base / 4 : 0;
  const float4* __restrict__ in4 = reinterpret_cast<const float4*>(in);
  float4* __restrict__ out4 = reinterpret_cast<float4*>(out);
  for (size_t e = t0; e < n4; e += stride) out4[e] = in4[e];
  for (size_t e = 4 * n4 + t0; e < total; e += stride) {
    if (e < base) {
      out[e] = in[e];
    } else {
      const size_t v = e - base;
      const uint32_t j = (uint32_t)(v / (size_t)w), c = (uint32_t)(v - (size_t)j * w);
      out[e] = in[(size_t)src[j] * w + c];
    }
  }
}

// One wave per virtual row: the argmax over num_dirs logits needs the whole row (any num_dirs)
__global__ __launch_bounds__(GR_BLOCK) void grow_expand_xyz_kernel(GsrGrow g, float* __restrict__ xyz_out) {
  const int j = blockIdx.x * GR_WAVES + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (j >= g.G) return;
  const int i = g.src[j];
  float dir[3];
  if (g.mode & GSR_GROW_DIR) {
    const int nd = g.num_dirs;
    const float* __restrict__ row = g.dirs_prob + (size_t)i * nd;
    float best;
    int bi;
    wave_argmax(row, nd, lane, best, bi);
    float sum = 0.0f;
    for (int n = lane; n < nd; n += WAVE) sum += expf(row[n] - best);
    sum = wave_reduce_add_f32(sum);
    if (lane != 0) return;
    const float y = 1.0f / sum;          // softmax at the argmax: exp(0) / sum
    const float h = (1.0f - y) + y;      // y_hard - y_soft.detach() + y_soft (:364-365)
    dir[0] = h * g.dirs[3 * bi]; dir[1] = h * g.dirs[3 * bi + 1]; dir[2] = h * g.dirs[3 * bi + 2];
  } else {
    if (lane != 0) return;
    const float v0 = g.conti_dirs[3 * i], v1 = g.conti_dirs[3 * i + 1], v2 = g.conti_dirs[3 * i + 2];
    const float n = fmaxf(sqrtf(v0 * v0 + v1 * v1 + v2 * v2), 1e-12f);   // F.normalize (:103)
    dir[0] = v0 / n; dir[1] = v1 / n; dir[2] = v2 / n;
  }
  const float s = fmaxf(fmaxf(expf(g.scaling[3 * i]), expf(g.scaling[3 * i + 1])), expf(g.scaling[3 * i + 2]));
  const float d = (g.mode & GSR_GROW_DISTANCE) ? 2.0f * sigmoidf_(g.grow_dist[i]) : 1.0f;
  const size_t o = 3 * ((size_t)g.P + j);
#pragma unroll
  for (int c = 0; c < 3; ++c) xyz_out[o + c] = g.xyz[3 * i + c] + (dir[c] * s) * d;
}

// samples s of the split (:202-209 / :210-212) of virtual row j
__device__ inline void split_samples(const GsrGrow& g, int i, int j, float* stds, float* s, float* sd) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    stds[c] = expf(g.scaling[3 * i + c]);
    if (g.mode & GSR_SPLIT_DISTANCE) {
      sd[c] = 2.2f * sigmoidf_(g.split_distance[3 * i + c]);
      s[c] = stds[c] * sd[c];
    } else {
      sd[c] = 0.0f;
      s[c] = 0.0f + stds[c] * g.noise[3 * (size_t)j + c];     // torch.normal(mean=0, std=stds)
    }
  }
}

__device__ inline float split_k(const GsrGrow& g, int i) {
  return (g.mode & GSR_SPLIT_SCALE) ? (0.6f * sigmoidf_(g.split_scale[i]) + 0.5f) * 2.0f : 1.6f;
}

__global__ __launch_bounds__(256) void grow_expand_split_kernel(GsrGrow g, float* __restrict__ xyz_out,
                                                                float* __restrict__ scaling_out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= g.G) return;
  const int i = g.src[j];
  Rot r;
  build_rotation(g.rotation + 4 * (size_t)i, r);
  float stds[3], s[3], sd[3];
  split_samples(g, i, j, stds, s, sd);
  const float lk = logf(split_k(g, i));
  const size_t o = 3 * ((size_t)g.P + j);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* R = r.R + 3 * c;
    const float p = g.xyz[3 * i + c];
    xyz_out[3 * (size_t)i + c] = p + ((R[0] * s[0] + R[1] * s[1]) + R[2] * s[2]);
    xyz_out[o + c] = ((R[0] * -s[0] + R[1] * -s[1]) + R[2] * -s[2]) + p;
    const float ls = g.scaling[3 * i + c] - lk;
    scaling_out[3 * (size_t)i + c] = ls;
    scaling_out[o + c] = ls;
  }
}

// ---- fold ---------------------------------------------------------------------------------------------------------
struct FoldArrays {
  const float* in[7];
  float* out[7];
  int width[7];
};

// out[i] = in[i] (+ in[P + vidx[i]]) element-wise over [P, width]
__global__ __launch_bounds__(256) void grow_fold_rows_kernel(FoldArrays a, int P, const int32_t* __restrict__ vidx) {
  const int k = blockIdx.y;
  const int w = a.width[k];
  if (w == 0) return;
  const size_t total = (size_t)P * w;
  const float* __restrict__ in = a.in[k];
  float* __restrict__ out = a.out[k];
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const uint32_t i = (uint32_t)(e / (size_t)w), c = (uint32_t)(e - (size_t)i * w);
    const int32_t j = vidx[i];
    out[e] = j < 0 ? in[e] : in[e] + in[((size_t)P + j) * w + c];
  }
}

// t = dir * s;  new = xyz + t * dist:  dL/ds onto the lowest-index maximum scale (then exp'), dL/d(dist) through 2 sigmoid
__device__ inline void grow_shift_terms(const GsrGrow& g, const GsrGrowGrads& d, int i, const float* gn, const float* dir,
                                        float s, int am, float dist, float sg) {
  float gs = 0.0f, gdist = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    gs += (gn[c] * dist) * dir[c];
    gdist += gn[c] * (dir[c] * s);
  }
  d.out[5][3 * (size_t)i + am] += gs * s;
  if (g.mode & GSR_GROW_DISTANCE) d.d_grow_dist[i] = (gdist * 2.0f) * ((1.0f - sg) * sg);
}

// One thread per virtual row: the chain rule of the grown / split rows onto their source's parameters
__global__ __launch_bounds__(256) void grow_fold_chain_kernel(GsrGrow g, GsrGrowGrads d) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= g.G) return;
  const int i = g.src[j];
  const size_t o = 3 * ((size_t)g.P + j);
  if (g.mode & GSR_GROW_DIR) return;        // not launched for it: grow_fold_dirs_kernel holds the logit row
  if (g.mode & GSR_GROW_CONTINUOUS) {
    const float e0 = expf(g.scaling[3 * i]), e1 = expf(g.scaling[3 * i + 1]), e2 = expf(g.scaling[3 * i + 2]);
    const int am = argmax3(e0, e1, e2);
    const float s = am == 0 ? e0 : (am == 1 ? e1 : e2);
    const float sg = (g.mode & GSR_GROW_DISTANCE) ? sigmoidf_(g.grow_dist[i]) : 0.0f;
    const float dist = (g.mode & GSR_GROW_DISTANCE) ? 2.0f * sg : 1.0f;
    const float gn[3] = {d.in[0][o], d.in[0][o + 1], d.in[0][o + 2]};
    // continuous directions only: grow_dir rows are folded by grow_fold_dirs_kernel (it holds the whole logit row)
    const float v0 = g.conti_dirs[3 * i], v1 = g.conti_dirs[3 * i + 1], v2 = g.conti_dirs[3 * i + 2];
    const float nrm = sqrtf(v0 * v0 + v1 * v1 + v2 * v2);
    const float n = fmaxf(nrm, 1e-12f);
    const float dir[3] = {v0 / n, v1 / n, v2 / n};
    // dL/d(dir) = g_new * d * s;  normalize backward: (gd - v (v . gd) / n^2) / n  (no norm term below eps)
    float gd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) gd[c] = (gn[c] * dist) * s;
    if (nrm > 1e-12f) {
      const float vg = (v0 * gd[0] + v1 * gd[1]) + v2 * gd[2];
      d.d_conti_dirs[3 * i] = (gd[0] - v0 * (vg / (n * n))) / n;
      d.d_conti_dirs[3 * i + 1] = (gd[1] - v1 * (vg / (n * n))) / n;
      d.d_conti_dirs[3 * i + 2] = (gd[2] - v2 * (vg / (n * n))) / n;
    } else {
      d.d_conti_dirs[3 * i] = gd[0] / n; d.d_conti_dirs[3 * i + 1] = gd[1] / n; d.d_conti_dirs[3 * i + 2] = gd[2] / n;
    }
    grow_shift_terms(g, d, i, gn, dir, s, am, dist, sg);
    return;
  }
  // learned split: xyz[i] + R s and R (-s) + xyz[i];  scaling raw - log(k) on both rows
  Rot r;
  build_rotation(g.rotation + 4 * (size_t)i, r);
  float stds[3], s[3], sd[3];
  split_samples(g, i, j, stds, s, sd);
  const size_t oi = 3 * (size_t)i;
  const float gu[3] = {d.in[0][oi] - d.in[0][o], d.in[0][oi + 1] - d.in[0][o + 1], d.in[0][oi + 2] - d.in[0][o + 2]};
  float dR[9], gsmp[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
#pragma unroll
    for (int n = 0; n < 3; ++n) dR[3 * m + n] = gu[m] * s[n];
  }
#pragma unroll
  for (int n = 0; n < 3; ++n) gsmp[n] = (r.R[n] * gu[0] + r.R[3 + n] * gu[1]) + r.R[6 + n] * gu[2];
  float dq[4];
  build_rotation_backward(r, dR, dq);
#pragma unroll
  for (int c = 0; c < 4; ++c) d.out[6][4 * (size_t)i + c] += dq[c];
  if (g.mode & GSR_SPLIT_DISTANCE) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      d.out[5][oi + c] += (gsmp[c] * sd[c]) * stds[c];
        const float sg = sigmoidf_(g.split_distance[oi + c]);
      d.d_split_distance[oi + c] = ((gsmp[c] * stds[c]) * 2.2f) * ((1.0f - sg) * sg);
    }
  }
  if (g.mode & GSR_SPLIT_SCALE) {
    // raw_out = raw - log(k):  dL/dk = -(sum of dL/draw_out over both rows) / k;  k = 2 (0.6 sigmoid(x) + 0.5)
    const float k = split_k(g, i);
    float t = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) t += d.in[5][oi + c] + d.in[5][o + c];
    const float sg = sigmoidf_(g.split_scale[i]);
    d.d_split_scale[i] = ((-t / k) * 2.0f * 0.6f) * ((1.0f - sg) * sg);
  }
}

// dirs_prob gradient of the selected rows (the caller zeroed the dense [P, num_dirs] tensor): for source i of virtual
// row j, the softmax backward of dL/d(one-hot) = dirs @ dL/d(dir)  (straight-through: y_hard - y_soft.detach() + y_soft,
// :360-366), and the max-scale / distance terms of the grown position.  One wave per virtual row.
__global__ __launch_bounds__(GR_BLOCK) void grow_fold_dirs_kernel(GsrGrow g, GsrGrowGrads d) {
  const int j = blockIdx.x * GR_WAVES + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (j >= g.G) return;
  const int i = g.src[j];
  const int nd = g.num_dirs;
  float* __restrict__ out = d.d_dirs_prob + (size_t)i * nd;
  const float* __restrict__ row = g.dirs_prob + (size_t)i * nd;
  const size_t o = 3 * ((size_t)g.P + j);
  const float e0 = expf(g.scaling[3 * i]), e1 = expf(g.scaling[3 * i + 1]), e2 = expf(g.scaling[3 * i + 2]);
  const int am = argmax3(e0, e1, e2);
  const float s = am == 0 ? e0 : (am == 1 ? e1 : e2);
  const float sg = (g.mode & GSR_GROW_DISTANCE) ? sigmoidf_(g.grow_dist[i]) : 0.0f;
  const float dist = (g.mode & GSR_GROW_DISTANCE) ? 2.0f * sg : 1.0f;
  const float gn[3] = {d.in[0][o], d.in[0][o + 1], d.in[0][o + 2]};
  const float gd0 = (gn[0] * dist) * s, gd1 = (gn[1] * dist) * s, gd2 = (gn[2] * dist) * s;
  float m;
  int bi;
  wave_argmax(row, nd, lane, m, bi);
  float sum = 0.0f;
  for (int n = lane; n < nd; n += WAVE) sum += expf(row[n] - m);
  sum = wave_reduce_add_f32(sum);
  // sum_n y_n * gh_n with gh_n = dirs[n] . dL/d(dir)
  float dot = 0.0f;
  for (int n = lane; n < nd; n += WAVE) {
    const float gh = (g.dirs[3 * n] * gd0 + g.dirs[3 * n + 1] * gd1) + g.dirs[3 * n + 2] * gd2;
    dot += (expf(row[n] - m) / sum) * gh;
  }
  dot = wave_reduce_add_f32(dot);
  for (int n = lane; n < nd; n += WAVE) {
    const float gh = (g.dirs[3 * n] * gd0 + g.dirs[3 * n + 1] * gd1) + g.dirs[3 * n + 2] * gd2;
    out[n] = (expf(row[n] - m) / sum) * (gh - dot);
  }
  if (lane == 0) {
    const float y = 1.0f / sum, h = (1.0f - y) + y;
    const float dir[3] = {h * g.dirs[3 * bi], h * g.dirs[3 * bi + 1], h * g.dirs[3 * bi + 2]};
    grow_shift_terms(g, d, i, gn, dir, s, am, dist, sg);
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// the plan's workspace is the shared head alone: classes {selected, selected & big}
static void launch_grow_plan(int P, const float* accum, const float* denom, const float* scaling, float thr, float pde,
                             int split_mode, void* ws, int32_t* vidx, int32_t* src, uint8_t* selected, hipStream_t s) {
  const RowPlanLayout L(P, 2);
  hipLaunchKernelGGL(grow_plan_kernel, dim3(L.nblocks), dim3(GR_BLOCK), 0, s, P, accum, denom, scaling, thr, pde,
                     split_mode, L.flags_of(ws), L.block_counts_of(ws), L.stride);
  launch_class_scans(L, ws, s);
  hipLaunchKernelGGL(grow_positions_kernel, dim3(L.nblocks), dim3(GR_BLOCK), 0, s, P, L.flags_of(ws),
                     L.block_offs_of(ws), vidx, src, selected);
}

static unsigned row_grid(size_t total) {
  size_t b = (total + 255) / 256;
  if (b > 8192) b = 8192;
  return (unsigned)(b < 1 ? 1 : b);
}

static void launch_grow_expand(const GsrGrow& g, float* const out[6], hipStream_t s) {
  RowArrays a;
  const float* in[6] = {g.xyz, g.f_dc, g.f_rest, g.opacity, g.scaling, g.rotation};
  const int width[6] = {3, 3, g.n_rest, 1, 3, 4};
  size_t widest = 0;
  for (int k = 0; k < 6; ++k) {
    a.in[k] = in[k];
    a.out[k] = out[k];
    a.width[k] = (in[k] && out[k]) ? width[k] : 0;
    if ((size_t)a.width[k] > widest) widest = a.width[k];
  }
  const size_t rows = (size_t)g.P + g.G;
  if (rows > 0)
    hipLaunchKernelGGL(grow_expand_rows_kernel, dim3(row_grid(rows * widest), 6), dim3(256), 0, s, a, g.P, g.G, g.src);
  if (g.G == 0) return;
  if (g.mode & (GSR_GROW_DIR | GSR_GROW_CONTINUOUS))
    hipLaunchKernelGGL(grow_expand_xyz_kernel, dim3((g.G + GR_WAVES - 1) / GR_WAVES), dim3(GR_BLOCK), 0, s, g, out[0]);
  else
    hipLaunchKernelGGL(grow_expand_split_kernel, dim3((g.G + 255) / 256), dim3(256), 0, s, g, out[0], out[4]);
}

static void launch_grow_fold(const GsrGrow& g, const GsrGrowGrads& d, hipStream_t s) {
  FoldArrays a;
  const int width[7] = {3, 3, 3, g.n_rest, 1, 3, 4};
  size_t widest = 0;
  for (int k = 0; k < 7; ++k) {
    a.in[k] = d.in[k];
    a.out[k] = d.out[k];
    a.width[k] = (d.in[k] && d.out[k]) ? width[k] : 0;
    if ((size_t)a.width[k] > widest) widest = a.width[k];
  }
  // GsrGrowGrads order: xyz, means2D, f_dc, f_rest, opacity, scaling, rotation
  if (g.P > 0)
    hipLaunchKernelGGL(grow_fold_rows_kernel, dim3(row_grid((size_t)g.P * widest), 7), dim3(256), 0, s, a, g.P, g.vidx);
  if ((g.mode & GSR_GROW_DIR) && g.G > 0)
    hipLaunchKernelGGL(grow_fold_dirs_kernel, dim3((g.G + GR_WAVES - 1) / GR_WAVES), dim3(GR_BLOCK), 0, s, g, d);
  // grow_dir rows are folded whole by grow_fold_dirs_kernel; the chain kernel serves continuous directions and splits
  if (g.G > 0 && !(g.mode & GSR_GROW_DIR)) hipLaunchKernelGGL(grow_fold_chain_kernel, dim3((g.G + 255) / 256), dim3(256), 0, s, g, d);
}

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_grow_workspace_bytes(int32_t P) { return P < 0 ? 0 : RowPlanLayout(P, 2).bytes; }
int gsr_grow_plan(int32_t P, const float* xyz_gradient_accum, const float* denom, const float* scaling_raw,
                  float grad_threshold, float percent_dense_extent, int32_t mode, void* workspace, size_t workspace_bytes,
                  int32_t* vidx, int32_t* src, uint8_t* selected, uint32_t counts_host[2], void* stream) {
  if (P < 0) return fail(GSR_E_BADARG, "P < 0");
  if (!counts_host) return fail(GSR_E_BADARG, "NULL counts_host");
  counts_host[0] = counts_host[1] = 0;
  if (P == 0) return 0;
  if (!xyz_gradient_accum || !denom || !scaling_raw || !workspace || !vidx || !src || !selected)
    return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({workspace}, 255u)) return fail(GSR_E_ALIGN, "workspace must be 256-byte aligned");
  const RowPlanLayout L(P, 2);
  if (workspace_bytes < L.bytes) return fail(GSR_E_CAPACITY, "grow workspace too small");
  const int grow = (mode & (GSR_GROW_DIR | GSR_GROW_CONTINUOUS)) != 0;
  if (!grow && !(mode & (GSR_SPLIT_DISTANCE | GSR_SPLIT_SCALE))) return fail(GSR_E_BADARG, "mode selects no branch");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_grow_plan(P, xyz_gradient_accum, denom, scaling_raw, grad_threshold, percent_dense_extent, grow ? 0 : 1,
                   workspace, vidx, src, selected, s);
  if (int rc = check(false, s, "grow_plan")) return rc;
  return read_class_totals(L, workspace, counts_host, s);
}

static int grow_validate(const GsrGrow* g) {
  if (!g) return fail(GSR_E_BADARG, "NULL GsrGrow");
  if (g->P < 0 || g->G < 0 || g->G > g->P) return fail(GSR_E_BADARG, "bad P / G");
  if (g->n_rest != 0 && g->n_rest != 45) return fail(GSR_E_BADARG, "n_rest must be 0 or 45");
  if (g->P > 0 && (!g->xyz || !g->f_dc || !g->opacity || !g->scaling || !g->rotation || (g->n_rest && !g->f_rest)))
    return fail(GSR_E_BADARG, "NULL model tensor");
  const int grow = (g->mode & (GSR_GROW_DIR | GSR_GROW_CONTINUOUS)) != 0;
  if ((g->mode & GSR_GROW_DIR) && (g->mode & GSR_GROW_CONTINUOUS))
    return fail(GSR_E_BADARG, "GSR_GROW_DIR and GSR_GROW_CONTINUOUS are exclusive");
  if (!grow && !(g->mode & (GSR_SPLIT_DISTANCE | GSR_SPLIT_SCALE))) return fail(GSR_E_BADARG, "mode selects no branch");
  if (g->P == 0) return 0;
  if (!g->vidx || (g->G > 0 && !g->src)) return fail(GSR_E_BADARG, "NULL vidx / src");
  if ((g->mode & GSR_GROW_DIR) && (!g->dirs_prob || !g->dirs || g->num_dirs <= 0))
    return fail(GSR_E_BADARG, "GSR_GROW_DIR needs dirs_prob, dirs and num_dirs > 0");
  if ((g->mode & GSR_GROW_CONTINUOUS) && !g->conti_dirs) return fail(GSR_E_BADARG, "NULL conti_dirs");
  if (grow && (g->mode & GSR_GROW_DISTANCE) && !g->grow_dist) return fail(GSR_E_BADARG, "NULL grow_dist");
  if (!grow && (g->mode & GSR_SPLIT_DISTANCE) && !g->split_distance) return fail(GSR_E_BADARG, "NULL split_distance");
  if (!grow && (g->mode & GSR_SPLIT_SCALE) && !g->split_scale) return fail(GSR_E_BADARG, "NULL split_scale");
  if (!grow && !(g->mode & GSR_SPLIT_DISTANCE) && g->G > 0 && !g->noise) return fail(GSR_E_BADARG, "NULL noise");
  return 0;
}

int gsr_grow_expand(const GsrGrow* g, float* xyz_out, float* f_dc_out, float* f_rest_out, float* opacity_out,
                    float* scaling_out, float* rotation_out, void* stream) {
  if (int rc = grow_validate(g)) return rc;
  if (g->P == 0) return 0;
  if (!xyz_out || !f_dc_out || !opacity_out || !scaling_out || !rotation_out || (g->n_rest && !f_rest_out))
    return fail(GSR_E_BADARG, "NULL output");
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* const out[6] = {xyz_out, f_dc_out, f_rest_out, opacity_out, scaling_out, rotation_out};
  launch_grow_expand(*g, out, s);
  return check(false, s, "grow_expand");
}

int gsr_grow_fold(const GsrGrow* g, const GsrGrowGrads* grads, void* stream) {
  if (int rc = grow_validate(g)) return rc;
  if (!grads) return fail(GSR_E_BADARG, "NULL grads");
  if (g->P == 0) return 0;
  for (int k = 0; k < 7; ++k) {
    if (k == 3 && !g->n_rest) continue;
    if (!grads->in[k] || !grads->out[k]) return fail(GSR_E_BADARG, "NULL gradient array");
  }
  const int grow = (g->mode & (GSR_GROW_DIR | GSR_GROW_CONTINUOUS)) != 0;
  if (((g->mode & GSR_GROW_DIR) && !grads->d_dirs_prob) || ((g->mode & GSR_GROW_CONTINUOUS) && !grads->d_conti_dirs) ||
      (grow && (g->mode & GSR_GROW_DISTANCE) && !grads->d_grow_dist) ||
      (!grow && (g->mode & GSR_SPLIT_DISTANCE) && !grads->d_split_distance) ||
      (!grow && (g->mode & GSR_SPLIT_SCALE) && !grads->d_split_scale))
    return fail(GSR_E_BADARG, "NULL gradient of a learned tensor of the mode");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_grow_fold(*g, *grads, s);
  return check(false, s, "grow_fold");
}

}  // extern "C"

// Load-time image ingest (include/gsr.h, ABI v19): what the reference does on the host for every image of a scene,
// between the file decode and the [3,H,W] float target the loss reads.
//
//   * composite_u8_kernel: the Blender reader's alpha composite (scene/dataset_readers.py:204-210) in float64,
//     n = v / 255.0, arr = n_rgb * n_a + bg * (1 - n_a), arr * 255.0 truncated toward zero, low eight bits.
//   * resize_pass_kernel: one pass (horizontal or vertical) of Pillow's 8-bit bicubic Image.resize: integer taps from
//     a host-built table, acc = 2^21 + sum pixel * tap, out = clamp(acc >> 22, 0, 255).
//   * to_float_chw_kernel: PILtoTorch + Camera.__init__ (utils/general_utils.py:21-27, scene/cameras.py:39-46):
//     float(v) / 255.0f, clamp to [0,1], times float(a) / 255.0f when there is an alpha channel; HWC -> CHW.
//
// Built with -ffp-contract=off, and the float64 / float32 steps are written with the round-to-nearest intrinsics: every
// operation is rounded on its own, as numpy and torch do on the host.  One thread per output pixel; every kernel is a
// stream of bytes in and out, bound by memory.
#include "gsr_common.h"
#include "gsr_entry.h"

namespace gsr {

namespace {

constexpr int IMG_THREADS = 256;
constexpr int RESIZE_PRECISION_BITS = 32 - 8 - 2;      // Pillow's PRECISION_BITS for 8-bit channels

__global__ __launch_bounds__(IMG_THREADS) void composite_u8_kernel(const uint8_t* __restrict__ rgba, size_t pixels,
                                                                   double bg0, double bg1, double bg2,
                                                                   uint8_t* __restrict__ rgb) {
  const size_t i = (size_t)blockIdx.x * IMG_THREADS + threadIdx.x;
  if (i >= pixels) return;
  const uchar4 v = reinterpret_cast<const uchar4*>(rgba)[i];
  const double na = __ddiv_rn((double)v.w, 255.0);
  const double rest = __dsub_rn(1.0, na);
  const double bg[3] = {bg0, bg1, bg2};
  const uint8_t in[3] = {v.x, v.y, v.z};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double n = __ddiv_rn((double)in[c], 255.0);
    const double arr = __dadd_rn(__dmul_rn(n, na), __dmul_rn(bg[c], rest));
    const double scaled = __dmul_rn(arr, 255.0);
    // numpy's float64 -> int8 cast: toward zero, then the low byte; the int8 bytes are then read as uint8.  |scaled|
    // stays far inside int32 for any background a caller can mean (the API bounds it)
    rgb[3 * i + c] = (uint8_t)((int32_t)scaled & 0xff);
  }
}

// One pass over `n_out` output pixels.  VERTICAL = false: in [rows, in_len, C] -> out [rows, out_len, C], taps along a
// row.  VERTICAL = true: in [in_len, cols, C] -> out [out_len, cols, C], taps down a column; neighbouring threads read
// neighbouring pixels of the same input row, so both passes are coalesced.
template <int C, bool VERTICAL>
__global__ __launch_bounds__(IMG_THREADS) void resize_pass_kernel(const uint8_t* __restrict__ in, int in_len, int out_len,
                                                                  int other, const int32_t* __restrict__ bounds,
                                                                  const int32_t* __restrict__ taps, int ksize,
                                                                  uint8_t* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * IMG_THREADS + threadIdx.x;
  const size_t n_out = (size_t)out_len * (size_t)other;
  if (idx >= n_out) return;
  // horizontal: idx = row * out_len + o; vertical: idx = o * cols + col
  const int o = VERTICAL ? (int)(idx / (size_t)other) : (int)(idx % (size_t)out_len);
  const size_t line = VERTICAL ? idx % (size_t)other : idx / (size_t)out_len;
  int first = bounds[2 * o], count = bounds[2 * o + 1];
  // the table comes from the host: keep every read inside the image whatever it holds
  first = min(max(first, 0), in_len);
  count = min(min(max(count, 0), ksize), in_len - first);
  const int32_t* __restrict__ k = taps + (size_t)o * (size_t)ksize;
  const size_t step = VERTICAL ? (size_t)other * C : (size_t)C;
  const uint8_t* __restrict__ p = VERTICAL ? in + ((size_t)first * (size_t)other + line) * C
                                           : in + (line * (size_t)in_len + (size_t)first) * C;
  int32_t acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 1 << (RESIZE_PRECISION_BITS - 1);
  for (int j = 0; j < count; ++j) {
    const int32_t w = k[j];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] += (int32_t)p[c] * w;
    p += step;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) out[idx * C + c] = (uint8_t)min(max(acc[c] >> RESIZE_PRECISION_BITS, 0), 255);
}

template <int C>
__global__ __launch_bounds__(IMG_THREADS) void to_float_chw_kernel(const uint8_t* __restrict__ in, size_t pixels,
                                                                   float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * IMG_THREADS + threadIdx.x;
  if (i >= pixels) return;
  uint8_t v[C];
  if constexpr (C == 4) {
    const uchar4 q = reinterpret_cast<const uchar4*>(in)[i];
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = in[C * i + c];
  }
  float mask = 1.0f;
  if constexpr (C == 4) mask = __fdiv_rn((float)v[3], 255.0f);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float x = fminf(fmaxf(__fdiv_rn((float)v[c], 255.0f), 0.0f), 1.0f);
    out[(size_t)c * pixels + i] = __fmul_rn(x, mask);
  }
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + IMG_THREADS - 1) / IMG_THREADS); }

template <int C>
void resize_pass(bool vertical, const uint8_t* in, int in_len, int out_len, int other, const int32_t* bounds,
                 const int32_t* taps, int ksize, uint8_t* out, hipStream_t s) {
  const size_t n = (size_t)out_len * (size_t)other;
  if (vertical)
    resize_pass_kernel<C, true><<<blocks_for(n), IMG_THREADS, 0, s>>>(in, in_len, out_len, other, bounds, taps, ksize, out);
  else
    resize_pass_kernel<C, false><<<blocks_for(n), IMG_THREADS, 0, s>>>(in, in_len, out_len, other, bounds, taps, ksize, out);
}

// one resize pass per call; bounds / taps: include/gsr.h
void launch_image_resize_pass(bool vertical, int C, const uint8_t* in, int in_len, int out_len, int other,
                              const int32_t* bounds, const int32_t* taps, int ksize, uint8_t* out, hipStream_t s) {
  if (C == 3) resize_pass<3>(vertical, in, in_len, out_len, other, bounds, taps, ksize, out, s);
  else resize_pass<1>(vertical, in, in_len, out_len, other, bounds, taps, ksize, out, s);
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

int gsr_image_composite_u8(const uint8_t* rgba, int32_t H, int32_t W, double bg_r, double bg_g, double bg_b,
                           uint8_t* rgb, void* stream) {
  if (!rgba || !rgb) return fail(GSR_E_BADARG, "NULL image");
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "bad image shape");
  const double bg[3] = {bg_r, bg_g, bg_b};
  for (double b : bg)
    if (!(b >= 0.0 && b <= 1.0)) return fail(GSR_E_BADARG, "background must lie in [0, 1]");
  if (!aligned({rgba}, 3u)) return fail(GSR_E_ALIGN, "the RGBA image must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t pixels = (size_t)H * (size_t)W;
  composite_u8_kernel<<<blocks_for(pixels), IMG_THREADS, 0, s>>>(rgba, pixels, bg_r, bg_g, bg_b, rgb);
  return check(false, s, "image_composite_u8");
}
int gsr_image_resize_u8(const uint8_t* src, int32_t C, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                        const int32_t* h_bounds, const int32_t* h_taps, int32_t h_ksize, const int32_t* v_bounds,
                        const int32_t* v_taps, int32_t v_ksize, uint8_t* tmp, uint8_t* dst, void* stream) {
  if (!src || !dst) return fail(GSR_E_BADARG, "NULL image");
  if (C != 1 && C != 3) return fail(GSR_E_BADARG, "resize takes 1 or 3 channels");
  if (!image_shape_ok(in_h, in_w) || !image_shape_ok(out_h, out_w) || !image_shape_ok(in_h, out_w))
    return fail(GSR_E_BADARG, "bad image shape");
  const bool horiz = out_w != in_w, vert = out_h != in_h;
  if (horiz && (!h_bounds || !h_taps || h_ksize <= 0)) return fail(GSR_E_BADARG, "horizontal pass needs its tap table");
  if (vert && (!v_bounds || !v_taps || v_ksize <= 0)) return fail(GSR_E_BADARG, "vertical pass needs its tap table");
  if (horiz && vert && !tmp) return fail(GSR_E_BADARG, "two passes need the intermediate image");
  if (!aligned({h_bounds, h_taps, v_bounds, v_taps}, 3u)) return fail(GSR_E_ALIGN, "tap tables must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!horiz && !vert) {
    GSR_HIP(hipMemcpyAsync(dst, src, (size_t)in_h * (size_t)in_w * (size_t)C, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  const uint8_t* mid = src;
  if (horiz) {
    uint8_t* out = vert ? tmp : dst;
    launch_image_resize_pass(false, C, src, in_w, out_w, in_h, h_bounds, h_taps, h_ksize, out, s);
    mid = out;
  }
  if (vert) launch_image_resize_pass(true, C, mid, in_h, out_h, out_w, v_bounds, v_taps, v_ksize, dst, s);
  return check(false, s, "image_resize_u8");
}
int gsr_image_to_float_chw(const uint8_t* src, int32_t C, int32_t H, int32_t W, float* dst, void* stream) {
  if (!src || !dst) return fail(GSR_E_BADARG, "NULL image");
  if (C != 3 && C != 4) return fail(GSR_E_BADARG, "the float target needs a 3- or 4-channel image");
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "bad image shape");
  if (!aligned({dst}, 3u) || (C == 4 && !aligned({src}, 3u)))
    return fail(GSR_E_ALIGN, "the float image and a 4-channel source must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t pixels = (size_t)H * (size_t)W;
  if (C == 4) to_float_chw_kernel<4><<<blocks_for(pixels), IMG_THREADS, 0, s>>>(src, pixels, dst);
  else to_float_chw_kernel<3><<<blocks_for(pixels), IMG_THREADS, 0, s>>>(src, pixels, dst);
  return check(false, s, "image_to_float_chw");
}

}  // extern "C"

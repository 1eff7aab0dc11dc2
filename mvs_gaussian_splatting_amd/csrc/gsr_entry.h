// What an extern "C" entry point (include/gsr.h) needs besides its kernels: the calling thread's error state and the
// argument checks that several files share.  Every file that defines gsr_* functions includes it; the error string
// itself is one thread_local object in gsr_api.hip, reached only through fail / hip_fail.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>

namespace gsr {

// make msg / "<where>: <HIP's error string>" the thread's gsr_last_error() and return code / (int)e
int fail(int code, const char* msg);
int hip_fail(hipError_t e, const char* where);
#define GSR_HIP(expr)                                        \
  do {                                                       \
    hipError_t _e = (expr);                                  \
    if (_e != hipSuccess) return hip_fail(_e, #expr);        \
  } while (0)

// after a batch of launches: surface launch errors; in debug mode (GsrParams::debug) also synchronise
inline int check(bool debug, hipStream_t s, const char* where) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, where);
  if (debug) {
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, where);
  }
  return 0;
}

// every pointer (NULL included) has the bits of mask clear
inline bool aligned(std::initializer_list<const void*> ptrs, uintptr_t mask) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  return (bits & mask) == 0;
}

// the [H,W] images that image ingest, exposure, TSDF views and the normal loss accept: at most 2^28 pixels
inline bool image_shape_ok(int32_t H, int32_t W) { return H > 0 && W > 0 && (int64_t)H * (int64_t)W <= (int64_t)1 << 28; }

}  // namespace gsr

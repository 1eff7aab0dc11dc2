// The row plan that densify.hip, densify_fork.hip and grow.hip share: every Gaussian gets a byte of class flags (bit c:
// "row i is in class c"), and each class is ranked in row order --
//
//   plan kernel      : the file's own classification, then block_count_classes: members of each class per block
//   class scans      : launch_class_scans: block counts -> exclusive block offsets and the grand totals
//   positions kernel : block_rank_classes: the global rank of every row in each class; the file's own writes
//   read-back        : read_class_totals: the totals, on the host
//
// Integer code only (no floating-point expression lives here), so every file compiles it under its own contraction
// setting.  All three files run it in PRE_BLOCK-thread blocks, one row per thread.
#pragma once
#include "gsr_common.h"
#include "gsr_entry.h"
#include "gsr_launch.h"

namespace gsr {

// The head of a plan workspace: flags | block_counts | block_offs | totals, each 256-byte aligned.  The nc counter arrays
// (and their offsets) lie `stride` = scan_array_stride(nblocks) words apart, which launch_scan_block_sums needs of arrays
// carved out of one buffer.  `bytes` is 256-aligned: a file's own arrays (pos, sel_src) start there.
struct RowPlanLayout {
  size_t flags, block_counts, block_offs, totals, bytes, rows;      // rows = max(P, 1)
  int nc, nblocks, stride;
  RowPlanLayout(int P, int nc_) : nc(nc_) {
    nblocks = (P + PRE_BLOCK - 1) / PRE_BLOCK;
    if (nblocks < 1) nblocks = 1;
    stride = scan_array_stride(nblocks);
    rows = (size_t)(P > 0 ? P : 1);
    size_t o = 0;
    flags = o;        o = align_up(o + rows, 256);
    block_counts = o; o = align_up(o + 4 * (size_t)nc * stride, 256);
    block_offs = o;   o = align_up(o + 4 * (size_t)nc * stride, 256);
    totals = o;       o = align_up(o + 64, 256);
    bytes = o;
  }
  template <typename T>
  static T* at(const void* ws, size_t off) { return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(ws) + off); }
  uint8_t* flags_of(const void* ws) const { return at<uint8_t>(ws, flags); }
  uint32_t* block_counts_of(const void* ws) const { return at<uint32_t>(ws, block_counts); }
  uint32_t* block_offs_of(const void* ws) const { return at<uint32_t>(ws, block_offs); }
  uint32_t* totals_of(const void* ws) const { return at<uint32_t>(ws, totals); }
};

// The end of a plan kernel: block_counts[c * stride + block] = rows of this block with bit c of f set.  Every thread of the
// block calls it (rows i >= P with f = 0): it holds two __syncthreads().
template <int NC>
__device__ inline void block_count_classes(uint8_t f, uint32_t* __restrict__ block_counts, int stride) {
  __shared__ uint32_t cnt[NC];
  if (threadIdx.x < NC) cnt[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int b = 0; b < NC; ++b) {
    const uint64_t m = __builtin_amdgcn_ballot_w64((f >> b) & 1);
    if ((threadIdx.x & (WAVE - 1)) == 0 && m) atomicAdd(&cnt[b], (uint32_t)__builtin_popcountll(m));
  }
  __syncthreads();
  if (threadIdx.x < NC) block_counts[(size_t)threadIdx.x * stride + blockIdx.x] = cnt[threadIdx.x];
}

// The start of a positions kernel: rank[c] = the row's rank in class c over the whole array (block_offs holds the scanned
// block counts), or -1 when bit c of f is clear.  It holds a __syncthreads(), so every thread of the block must reach it,
// rows i >= P included (with f = 0); return on i >= P after it.
template <int NC>
__device__ inline void block_rank_classes(uint8_t f, const uint32_t* __restrict__ block_offs, int stride,
                                          int32_t rank[NC]) {
  __shared__ uint32_t wave_tot[NC][PRE_BLOCK / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  uint32_t in_wave[NC];
#pragma unroll
  for (int b = 0; b < NC; ++b) {
    const uint64_t m = __builtin_amdgcn_ballot_w64((f >> b) & 1);
    in_wave[b] = (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[b][wid] = (uint32_t)__builtin_popcountll(m);
  }
  __syncthreads();
#pragma unroll
  for (int b = 0; b < NC; ++b) {
    uint32_t base = block_offs[(size_t)b * stride + blockIdx.x];
    for (int w = 0; w < wid; ++w) base += wave_tot[b][w];
    rank[b] = ((f >> b) & 1) ? (int32_t)(base + in_wave[b]) : -1;
  }
}

// Scans the nc block-count arrays into block_offs and totals[0..nc), two arrays per launch (the last launch of an odd nc
// carries one).
inline void launch_class_scans(const RowPlanLayout& L, void* ws, hipStream_t s) {
  const uint32_t* c = L.block_counts_of(ws);
  uint32_t* o = L.block_offs_of(ws);
  uint32_t* t = L.totals_of(ws);
  const size_t st = (size_t)L.stride;
  for (int b = 0; b < L.nc; b += 2) {
    if (b + 1 < L.nc)
      launch_scan_block_sums(c + b * st, o + b * st, t + b, c + (b + 1) * st, o + (b + 1) * st, t + b + 1, L.nblocks, s);
    else
      launch_scan_block_sums(c + b * st, o + b * st, t + b, nullptr, nullptr, nullptr, L.nblocks, s);
  }
}

// counts_host[0..nc) = the class totals of the plan enqueued on s; waits for the stream
inline int read_class_totals(const RowPlanLayout& L, const void* ws, uint32_t* counts_host, hipStream_t s) {
  GSR_HIP(hipMemcpyAsync(counts_host, L.totals_of(ws), 4 * (size_t)L.nc, hipMemcpyDeviceToHost, s));
  GSR_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // namespace gsr

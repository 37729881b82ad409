// Stream compaction pieces shared by the removals (amdr_bm25_remove, bm25_update.hip; the token-store removal of
// rows_compact.hip scans its document lengths with compact_scan_i64_kernel): where a kept element goes is its rank among the
// kept ones, and a rank is
//   the exclusive scan of the per-tile counts (compact_scan_i64_kernel)  +  the exclusive scan of the keep flags inside
//   the element's tile (compact_tile_scan, in LDS).
// No atomics: every position is a sum of counts, so the result is deterministic.  The host forms (compact_scan_host,
// compact_tile_scan_host) compute the same values in plain C++ for the host check programs, which define
// AMDR_COMPACT_HOST_ONLY before they include this file: no kernel is declared then (a program built for the host alone
// has no device code object to register one with) and no HIP header is needed.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) && !defined(AMDR_COMPACT_HOST_ONLY)
#define AMDR_COMPACT_DEVICE 1
#include <hip/hip_runtime.h>
#endif

namespace amdr {

constexpr int kCompactScanThreads = 1024;  // compact_scan_i64_kernel: one block of this many threads
constexpr int kCompactScanPerThread = 4;   // consecutive values per thread and round

// out[0 .. n] = exclusive prefix sums of in[0 .. n-1]; out[n] is the total.  `out` holds n + 1 values.
inline void compact_scan_host(const long long* in, long n, long long* out) {
  long long run = 0;
  for (long i = 0; i < n; ++i) {
    out[i] = run;
    run += in[i];
  }
  out[n] = run;
}

// rank[i] = number of set flags before i, for a tile of n flags; returns the tile's count.
inline int compact_tile_scan_host(const unsigned char* keep, int n, unsigned short* rank) {
  int run = 0;
  for (int i = 0; i < n; ++i) {
    rank[i] = (unsigned short)run;
    run += keep[i] ? 1 : 0;
  }
  return run;
}

#if defined(AMDR_COMPACT_DEVICE)

// Inclusive scan of one value per lane over the wave (64 lanes), by shuffles.
template <class T>
__device__ inline T compact_wave_inclusive(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(v, d, 64);
    if (lane >= d) v += up;
  }
  return v;
}

// Block-wide exclusive scan of one value per thread (THREADS a multiple of 64, at most 1024).  `wsum` is LDS room of
// THREADS / 64 + 1 values; every thread of the block calls this.  Returns the thread's exclusive prefix and sets *total
// to the block's sum.  Ends with a barrier, so `wsum` may be used again at once.
template <int THREADS, class T>
__device__ inline T compact_block_exclusive(T v, T* wsum, T* total) {
  static_assert(THREADS % 64 == 0 && THREADS <= 1024, "whole waves, at most 16 of them");
  constexpr int kWaves = THREADS / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T incl = compact_wave_inclusive(v);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    T run = 0;
    for (int w = 0; w < kWaves; ++w) {
      const T s = wsum[w];
      wsum[w] = run;
      run += s;
    }
    wsum[kWaves] = run;
  }
  __syncthreads();
  const T out = wsum[wave] + incl - v;
  *total = wsum[kWaves];
  __syncthreads();
  return out;
}

// The tile scan: thread tid of THREADS owns elements tid, tid + THREADS, ... of a tile of THREADS * PER elements (the
// coalesced layout of the kernels that read a tile) and passes their keep flags as bits of `keep_bits` (bit u = element
// u * THREADS + tid).  rank[u] becomes the number of kept elements before element u * THREADS + tid in the tile; returns
// the tile's count.  `lds` holds THREADS * PER + THREADS / 64 + 1 ints.
template <int THREADS, int PER>
__device__ inline int compact_tile_scan(unsigned keep_bits, int* lds, int* rank) {
  static_assert(PER <= 32, "one bit per element");
  const int tid = threadIdx.x;
  // a thread scans PER CONSECUTIVE elements, so the flags change hands through LDS: written in the owners' layout, read
  // back in the scanners'
#pragma unroll
  for (int u = 0; u < PER; ++u) lds[u * THREADS + tid] = (int)((keep_bits >> u) & 1u);
  __syncthreads();
  int mine = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) mine += lds[tid * PER + j];
  int total;
  const int before = compact_block_exclusive<THREADS, int>(mine, lds + THREADS * PER, &total);
  int run = before;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int f = lds[tid * PER + j];
    lds[tid * PER + j] = run;
    run += f;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < PER; ++u) rank[u] = lds[u * THREADS + tid];
  __syncthreads();
  return total;
}

// out[0 .. n] = exclusive prefix sums of in[0 .. n-1], out[n] the total: ONE block of kCompactScanThreads threads walks the
// array in rounds of kCompactScanThreads * kCompactScanPerThread values and carries the running sum.  Meant for the short
// arrays of a compaction (one value per tile, one per term), not for the elements themselves.  in and out may not overlap.
// Internal linkage: every translation unit that includes this header gets a kernel of its own, and two of them link.
static __global__ __launch_bounds__(kCompactScanThreads) void compact_scan_i64_kernel(const long long* __restrict__ in, long n,
                                                                                      long long* __restrict__ out) {
  __shared__ long long wsum[kCompactScanThreads / 64 + 1];
  constexpr long kRound = (long)kCompactScanThreads * kCompactScanPerThread;
  long long carry = 0;
  for (long base = 0; base < n; base += kRound) {
    const long i0 = base + (long)threadIdx.x * kCompactScanPerThread;
    long long v[kCompactScanPerThread];
    long long mine = 0;
#pragma unroll
    for (int j = 0; j < kCompactScanPerThread; ++j) {
      v[j] = i0 + j < n ? in[i0 + j] : 0;
      mine += v[j];
    }
    long long total;
    long long run = carry + compact_block_exclusive<kCompactScanThreads, long long>(mine, wsum, &total);
#pragma unroll
    for (int j = 0; j < kCompactScanPerThread; ++j) {
      if (i0 + j < n) out[i0 + j] = run;
      run += v[j];
    }
    carry += total;
  }
  if (threadIdx.x == 0) out[n] = carry;
}

#endif  // AMDR_COMPACT_DEVICE

}  // namespace amdr

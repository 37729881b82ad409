// Ordered row compaction of a resident matrix: the device half of amdr_dense_remove (dense.hip) and amdr_maxsim_remove
// (maxsim.hip).  The surviving rows close up in their old order into a NEW buffer (never in place); which old row a new
// row comes from is the rule of rows_compact.hpp, shared with the host check (check_rows_compact.cpp).
//
//   rows_compact_kernel      uniform rows of row_bytes (a multiple of 16; the dense matrix: 4 * d)
//   segments_len_kernel      new document j -> its length and the old row its rows start at        } the doc_ptr rebuild
//   compact_scan_i64_kernel  (compact.hpp) the exclusive scan of the lengths = the new doc_ptr     }
//   segments_compact_kernel  token rows of 512 B under the segmented map (the MaxSim store)
// and of the replaces (documents keep their ids; the rule is rows_compact.hpp's rs_*):
//   rows_scatter_kernel      staged rows written over rows replace_ids[i] of the dense matrix, in place
//   splice_len_kernel        document j -> its length afterwards and its signed source row        } + the same scan
//   segments_splice_kernel   token rows of 512 B, each from the old store or from the staged rows, into a new buffer
//
// Both copy kernels move 16-byte units.  A block owns a slab of kRcSlabUnits consecutive NEW units (whole rows: 32 KiB or
// a little less), first writes the old row of each of the slab's rows into LDS — every thread a run of consecutive rows:
// one binary search in the removal list, read from global memory, then the linear walk — and then copies: thread t moves
// units t, t + 256, ... of the slab, so a wave's 64 lanes load and store 1 KiB of consecutive bytes per instruction
// wherever a row is at least that long, and whole rows side by side where it is shorter (the destination is always
// consecutive).  A thread moves one unit at a time (rc_copy_slab says why).  The grid is capped at 8 blocks per CU and
// strides over the slabs.  No atomics, no ordering between blocks: every destination unit has one writer and its value
// depends on the inputs alone.
// Algorithmic traffic: every surviving byte read once and written once, plus the removal list (searched, so a fraction
// of it per slab) and, segmented, both doc_ptrs and 16 B of scratch per surviving document.
#include "rows_compact.hpp"

#include "common.hpp"
#include "compact.hpp"

namespace amdr {
namespace {

constexpr int kRcThreads = 256;
constexpr int kRcPerThread = 8;                          // units of a slab per thread
constexpr int kRcSlabUnits = kRcThreads * kRcPerThread;  // 16-byte units per slab
constexpr int kRcMaxBlocks = 256 * 8;
constexpr int kSegRowUnits = 32;                           // a token row: 128 x fp32 = 512 B
constexpr int kSegSlabRows = kRcSlabUnits / kSegRowUnits;  // 64 token rows per slab
constexpr int kSegRun = 4;                                 // consecutive rows whose source one thread finds

// The slab's copy: unit u of the slab belongs to its row u / units_per_row, whose old row is row_src[that]; the slab's
// first destination unit is dst0.  `units` <= kRcSlabUnits.  One unit per thread and step, each stored as soon as it has
// arrived, the loop not unrolled: measured on 4 M x 768 rows, this form copies at the rate of a plain grid-stride copy
// and of hipMemcpy device-to-device (5.1-5.2 TB/s), while issuing 2, 4 or 8 of a thread's loads ahead of their stores
// copies at 3.7, 3.5 and 3.5 TB/s — the memory-level parallelism comes from the eight resident blocks of a CU.
__device__ inline void rc_copy_slab(const uint4* __restrict__ src, uint4* __restrict__ dst, long long dst0, int units,
                                    int units_per_row, const long long* row_src) {
#pragma unroll 1
  for (int u = (int)threadIdx.x; u < units; u += kRcThreads) {
    const int row = u / units_per_row;
    dst[dst0 + u] = src[row_src[row] * units_per_row + (u - row * units_per_row)];
  }
}

__global__ __launch_bounds__(kRcThreads) void rows_compact_kernel(const uint4* __restrict__ src, long long n_new,
                                                                  int units_per_row, int rows_per_slab, long long slabs,
                                                                  const long long* __restrict__ remove_ids, long n_remove,
                                                                  uint4* __restrict__ dst) {
  __shared__ long long row_src[kRcSlabUnits];  // (a slab of 16-byte rows holds this many rows)
  const int per = (rows_per_slab + kRcThreads - 1) / kRcThreads;
  for (long long slab = blockIdx.x; slab < slabs; slab += gridDim.x) {
    const long long j0 = slab * rows_per_slab;
    const int rows = (int)(n_new - j0 < rows_per_slab ? n_new - j0 : rows_per_slab);
    const int a = (int)threadIdx.x * per;
    if (a < rows) rc_src_range(remove_ids, n_remove, j0 + a, rows - a < per ? rows - a : per, row_src + a);
    __syncthreads();
    rc_copy_slab(src, dst, j0 * units_per_row, rows * units_per_row, units_per_row, row_src);
    __syncthreads();
  }
}

// New document j of n_docs_new: its length and the old row its rows start at.
__global__ __launch_bounds__(256) void segments_len_kernel(const long long* __restrict__ doc_ptr, long n_docs_new,
                                                           const long long* __restrict__ remove_ids, long n_remove,
                                                           long long* __restrict__ len, long long* __restrict__ start) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_docs_new) return;
  rc_seg_entry(doc_ptr, rc_src(remove_ids, n_remove, j), &len[j], &start[j]);
}

__global__ __launch_bounds__(kRcThreads) void segments_compact_kernel(const uint4* __restrict__ src, long long rows_new,
                                                                      long long slabs, const long long* __restrict__ new_ptr,
                                                                      const long long* __restrict__ start, long n_docs_new,
                                                                      uint4* __restrict__ dst) {
  __shared__ long long row_src[kSegSlabRows];
  for (long long slab = blockIdx.x; slab < slabs; slab += gridDim.x) {
    const long long t0 = slab * kSegSlabRows;
    const int rows = (int)(rows_new - t0 < kSegSlabRows ? rows_new - t0 : kSegSlabRows);
    const int a = (int)threadIdx.x * kSegRun;
    if (a < rows) {
      long j = rc_seg_doc(new_ptr, n_docs_new, t0 + a);
      for (int i = 0; i < kSegRun && a + i < rows; ++i) {
        j = rc_seg_walk(new_ptr, n_docs_new, j, t0 + a + i);
        row_src[a + i] = rc_seg_src(new_ptr, start, j, t0 + a + i);
      }
    }
    __syncthreads();
    rc_copy_slab(src, dst, t0 * kSegRowUnits, rows * kSegRowUnits, kSegRowUnits, row_src);
    __syncthreads();
  }
}

// ---- replace: rows exchanged under unchanged ids (amdr_dense_replace, amdr_maxsim_replace) ----------------------------
// The dense form writes IN PLACE: staged row i goes to row replace_ids[i] of the matrix, nothing else moves.  Unit u of
// the staged rows (consecutive, so a wave loads 1 KiB per instruction) has one destination and one writer — the ids are
// strictly ascending — so there is nothing to order.  Traffic: every replaced byte read once and written once + 8 B an id.
__global__ __launch_bounds__(kRcThreads) void rows_scatter_kernel(const uint4* __restrict__ rows, long long units,
                                                                  int units_per_row,
                                                                  const long long* __restrict__ replace_ids,
                                                                  uint4* __restrict__ dst) {
  const long long step = (long long)gridDim.x * kRcThreads;
#pragma unroll 1
  for (long long u = (long long)blockIdx.x * kRcThreads + threadIdx.x; u < units; u += step) {
    const long long i = u / units_per_row;
    dst[replace_ids[i] * units_per_row + (u - i * units_per_row)] = rows[u];
  }
}

// Document j of n_docs (the count does not change): its length afterwards and the signed source row its rows start at.
__global__ __launch_bounds__(256) void splice_len_kernel(const long long* __restrict__ doc_ptr, long n_docs,
                                                         const long long* __restrict__ add_ptr,
                                                         const long long* __restrict__ replace_ids, long n_rep,
                                                         long long* __restrict__ len, long long* __restrict__ start) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_docs) return;
  rs_seg_entry(doc_ptr, add_ptr, replace_ids, n_rep, j, &len[j], &start[j]);
}

// The ordered splice of 512-byte token rows into a NEW buffer: segments_compact_kernel with two sources.  A slab's rows
// get their signed source row in LDS (rs_seg_src), then every unit is loaded from the old store or from the staged rows
// and stored to its consecutive destination, one unit per thread and step as in rc_copy_slab.
__global__ __launch_bounds__(kRcThreads) void segments_splice_kernel(const uint4* __restrict__ old_rows,
                                                                     const uint4* __restrict__ add_rows, long long rows_new,
                                                                     long long slabs, const long long* __restrict__ new_ptr,
                                                                     const long long* __restrict__ start, long n_docs,
                                                                     uint4* __restrict__ dst) {
  __shared__ long long row_src[kSegSlabRows];
  for (long long slab = blockIdx.x; slab < slabs; slab += gridDim.x) {
    const long long t0 = slab * kSegSlabRows;
    const int rows = (int)(rows_new - t0 < kSegSlabRows ? rows_new - t0 : kSegSlabRows);
    const int a = (int)threadIdx.x * kSegRun;
    if (a < rows) {
      long j = rc_seg_doc(new_ptr, n_docs, t0 + a);
      for (int i = 0; i < kSegRun && a + i < rows; ++i) {
        j = rc_seg_walk(new_ptr, n_docs, j, t0 + a + i);
        row_src[a + i] = rs_seg_src(new_ptr, start, j, t0 + a + i);
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int u = (int)threadIdx.x; u < rows * kSegRowUnits; u += kRcThreads) {
      const int row = u / kSegRowUnits;
      const long long s = row_src[row];
      const uint4* from = s >= 0 ? old_rows + s * kSegRowUnits : add_rows + ~s * kSegRowUnits;
      dst[t0 * kSegRowUnits + u] = from[u - row * kSegRowUnits];
    }
    __syncthreads();
  }
}

unsigned rc_grid(long long slabs) { return (unsigned)(slabs < kRcMaxBlocks ? slabs : kRcMaxBlocks); }

}  // namespace

int rows_compact_launch(const void* src, long long n_new, long row_bytes, const long long* remove_ids, long n_remove,
                        void* dst, hipStream_t st) {
  AMDR_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0 && row_bytes / 16 <= kRcSlabUnits,
               "rows_compact: row_bytes=%ld must be a multiple of 16, at most %d", row_bytes, kRcSlabUnits * 16);
  AMDR_REQUIRE(n_new >= 0 && n_remove >= 0, "rows_compact: bad sizes");
  if (n_new == 0) return AMDR_OK;
  AMDR_REQUIRE(src && dst && (remove_ids || n_remove == 0), "rows_compact: null");
  AMDR_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, "rows_compact: buffers must be 16-byte aligned");
  const int upr = (int)(row_bytes / 16), rows_per_slab = kRcSlabUnits / upr;
  const long long slabs = (n_new + rows_per_slab - 1) / rows_per_slab;
  hipLaunchKernelGGL(rows_compact_kernel, dim3(rc_grid(slabs)), dim3(kRcThreads), 0, st, (const uint4*)src, n_new, upr,
                     rows_per_slab, slabs, remove_ids, n_remove, (uint4*)dst);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

int segments_ptr_launch(const long long* doc_ptr, long n_docs_new, const long long* remove_ids, long n_remove,
                        long long* len, long long* start, long long* new_ptr, hipStream_t st) {
  AMDR_REQUIRE(n_docs_new >= 1 && n_remove >= 0, "segments_ptr: bad sizes");
  AMDR_REQUIRE(doc_ptr && len && start && new_ptr && (remove_ids || n_remove == 0), "segments_ptr: null");
  hipLaunchKernelGGL(segments_len_kernel, dim3((unsigned)((n_docs_new + 255) / 256)), dim3(256), 0, st, doc_ptr, n_docs_new,
                     remove_ids, n_remove, len, start);
  AMDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(compact_scan_i64_kernel, dim3(1), dim3(kCompactScanThreads), 0, st, len, n_docs_new, new_ptr);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

int segments_compact_launch(const void* src, long long rows_new, const long long* new_ptr, const long long* start,
                            long n_docs_new, void* dst, hipStream_t st) {
  AMDR_REQUIRE(rows_new >= 1 && n_docs_new >= 1, "segments_compact: bad sizes");
  AMDR_REQUIRE(src && dst && new_ptr && start, "segments_compact: null");
  AMDR_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, "segments_compact: buffers must be 16-byte aligned");
  const long long slabs = (rows_new + kSegSlabRows - 1) / kSegSlabRows;
  hipLaunchKernelGGL(segments_compact_kernel, dim3(rc_grid(slabs)), dim3(kRcThreads), 0, st, (const uint4*)src, rows_new,
                     slabs, new_ptr, start, n_docs_new, (uint4*)dst);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

int rows_scatter_launch(const void* rows, long long n_rep, long row_bytes, const long long* replace_ids, void* dst,
                        hipStream_t st) {
  AMDR_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0, "rows_scatter: row_bytes=%ld must be a multiple of 16", row_bytes);
  AMDR_REQUIRE(n_rep >= 1 && rows && replace_ids && dst, "rows_scatter: bad arguments");
  AMDR_REQUIRE((((uintptr_t)rows | (uintptr_t)dst) & 15) == 0, "rows_scatter: buffers must be 16-byte aligned");
  const int upr = (int)(row_bytes / 16);
  const long long units = n_rep * upr;
  hipLaunchKernelGGL(rows_scatter_kernel, dim3(rc_grid((units + kRcThreads - 1) / kRcThreads)), dim3(kRcThreads), 0, st,
                     (const uint4*)rows, units, upr, replace_ids, (uint4*)dst);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

int splice_ptr_launch(const long long* doc_ptr, long n_docs, const long long* add_ptr, const long long* replace_ids,
                      long n_rep, long long* len, long long* start, long long* new_ptr, hipStream_t st) {
  AMDR_REQUIRE(n_docs >= 1 && n_rep >= 1, "splice_ptr: bad sizes");
  AMDR_REQUIRE(doc_ptr && add_ptr && replace_ids && len && start && new_ptr, "splice_ptr: null");
  hipLaunchKernelGGL(splice_len_kernel, dim3((unsigned)((n_docs + 255) / 256)), dim3(256), 0, st, doc_ptr, n_docs, add_ptr,
                     replace_ids, n_rep, len, start);
  AMDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(compact_scan_i64_kernel, dim3(1), dim3(kCompactScanThreads), 0, st, len, n_docs, new_ptr);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

int segments_splice_launch(const void* old_rows, const void* add_rows, long long rows_new, const long long* new_ptr,
                           const long long* start, long n_docs, void* dst, hipStream_t st) {
  AMDR_REQUIRE(rows_new >= 1 && n_docs >= 1, "segments_splice: bad sizes");
  AMDR_REQUIRE(old_rows && add_rows && dst && new_ptr && start, "segments_splice: null");
  AMDR_REQUIRE((((uintptr_t)old_rows | (uintptr_t)add_rows | (uintptr_t)dst) & 15) == 0,
               "segments_splice: buffers must be 16-byte aligned");
  const long long slabs = (rows_new + kSegSlabRows - 1) / kSegSlabRows;
  hipLaunchKernelGGL(segments_splice_kernel, dim3(rc_grid(slabs)), dim3(kRcThreads), 0, st, (const uint4*)old_rows,
                     (const uint4*)add_rows, rows_new, slabs, new_ptr, start, n_docs, (uint4*)dst);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

}  // namespace amdr

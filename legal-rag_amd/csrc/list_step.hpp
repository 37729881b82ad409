// What the list resolvers on the BM25 handle share: term_scope.hip (term constraints), phrase_scope.hip (phrases, Nears),
// union_lists.hip (Prefix / OneOf), class_span.hip (PhraseOf / NearOf) and unit_span.hip (Within).  Each resolves ITEMS into
// ascending lists that lie back to back in one array (list_ptr [n + 1] | rows), in three launches without atomics:
//   count   the resolver's own kernel, one block per CELL (item x tile): the tile's keep count -> counts[cell], what the
//           write pass needs again parked in the cell's payload.
//   scan    compact_scan_i64_kernel over the counts: every cell's offset.
//   write   the resolver's own kernel: kept element -> rows[start + offsets[cell] + rank]; positions >= rows_cap are
//           dropped (status 2); thread 0 of an item's tile 0 writes the item's list_ptr entry (list_write_header).
// A call may CONTINUE an array: n_before lists stand before its own, start = list_ptr[n_before] is read on the device.
// Here: the workspace layout, the launch sequence, the device pieces of the write pass and of the candidate-tile kernels
// (phrase_scope.hip, class_span.hip, unit_span.hip), and the host twins' staging over bm25->tscope.  What an item is, its grid and its
// kernels stay with each resolver.
#pragma once
#include "bm25_handle.hpp"
#include "compact.hpp"
#include "phrase_rule.hpp"
#include "union_rule.hpp"

namespace amdr {

// ---- workspace ------------------------------------------------------------------------------------------------------------
constexpr size_t kListAlign = 256;
inline size_t list_align(size_t b) { return (b + kListAlign - 1) / kListAlign * kListAlign; }

// counts i64 [cells] | offsets i64 [cells + 1] | payload [cells x payload_per_cell bytes], each region aligned
struct ListWork {
  size_t off_counts, off_offsets, off_payload, total;
};
inline ListWork list_work(size_t cells, size_t payload_per_cell) {
  ListWork w;
  w.off_counts = 0;
  w.off_offsets = list_align(cells * sizeof(long long));
  w.off_payload = w.off_offsets + list_align((cells + 1) * sizeof(long long));
  w.total = w.off_payload + list_align(cells * payload_per_cell);
  return w;
}

// the workspace arguments of a "_device" entry against the plan's `need` (0 for an empty call)
inline int list_check_work(const char* who, const void* work_dev, int64_t work_bytes, size_t need) {
  AMDR_REQUIRE(work_bytes >= 0, "%s: work_bytes=%lld", who, (long long)work_bytes);
  AMDR_REQUIRE((size_t)work_bytes >= need && (need == 0 || work_dev), "%s: a workspace of %lld bytes, the plan asks for %zu", who,
               (long long)work_bytes, need);
  return AMDR_OK;
}

// ---- the launch sequence --------------------------------------------------------------------------------------------------
// count(counts, payload) and write(offsets, payload) enqueue the resolver's two kernels on `st`.  An empty call (n == 0)
// enqueues no kernel: it starts an empty array (list_ptr[0] = 0) or, behind n_before lists, leaves the array as it is.
template <class Count, class Write>
int list_launch(hipStream_t st, int64_t n, int64_t n_before, size_t cells, size_t payload_per_cell, long long* list_ptr,
                unsigned char* work, Count&& count, Write&& write) {
  if (n == 0) {
    if (n_before == 0) AMDR_HIP(hipMemsetAsync(list_ptr, 0, sizeof(long long), st));
    return AMDR_OK;
  }
  const ListWork w = list_work(cells, payload_per_cell);
  long long* counts = reinterpret_cast<long long*>(work + w.off_counts);
  long long* offsets = reinterpret_cast<long long*>(work + w.off_offsets);
  count(counts, work + w.off_payload);
  AMDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(compact_scan_i64_kernel, dim3(1), dim3(kCompactScanThreads), 0, st, (const long long*)counts, (long)cells,
                     offsets);
  AMDR_HIP(hipGetLastError());
  write((const long long*)offsets, (const unsigned char*)(work + w.off_payload));
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

// ---- device pieces --------------------------------------------------------------------------------------------------------
// Where the call's own rows begin.  (Entry n_before is not written by this launch unless n_before == 0, and then it is not
// read.)  list_ptr may be the array the kernel writes: no __restrict__ here.
__device__ __forceinline__ long long list_start(const long long* list_ptr, long long n_before) {
  return n_before > 0 ? list_ptr[n_before] : 0;
}

// Item p's list_ptr entry, by ONE thread of the item's tile 0: [begin, end) is the item's list in the unclamped array.
// Entry n_before + p + 1 is written clamped to rows_cap — entry 0 too by the item that starts an array — so a call
// writes the entries n_before + 1 .. n_before + n, and 0 .. n when n_before == 0.  Returns the item's status word, 0 or 2:
// a union stores it outright, a resolver whose count pass may have stored 1 only raises to it.
__device__ __forceinline__ int list_write_header(long long* list_ptr, long long n_before, long long p, long long begin,
                                                 long long end, long long rows_cap) {
  if (n_before == 0 && p == 0) list_ptr[0] = 0;
  list_ptr[n_before + p + 1] = un_clamp(end, rows_cap);
  return un_status(begin, end, rows_cap);
}

// LDS traffic between the lanes of ONE wave: the LDS unit serves a wave's operations in order, so only the compiler has
// to be kept from moving them.
__device__ __forceinline__ void list_wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The candidate-tile kernels (one candidate per thread, THREADS of them): the threads whose candidate passed phase 1
// (`all`) are compacted, in thread order, into surv[], and every keep flag is cleared.  Holds barriers: EVERY thread of
// the block calls it, under a block-uniform condition.  Returns the survivor count, block-uniform; ends with a barrier, so
// surv[] and kept[] may be used at once.
template <int THREADS>
__device__ __forceinline__ int list_compact_survivors(bool all, unsigned short* surv, unsigned char* kept, int* wsum) {
  kept[threadIdx.x] = 0;
  int n_surv;
  const int slot = compact_block_exclusive<THREADS, int>(all ? 1 : 0, wsum, &n_surv);
  if (all) surv[slot] = (unsigned short)threadIdx.x;
  __syncthreads();
  return n_surv;
}

// Behind phase 2: the block ranks its kept candidates, parks rank-or-minus-one per candidate in the cell's payload and
// writes the cell's keep count.  Begins with the barrier that ends phase 2 (kept[] was written by other waves): EVERY
// thread of the block calls it, under a block-uniform condition.
template <int THREADS>
__device__ __forceinline__ void list_rank_and_park(const unsigned char* kept, int* wsum, int* rank_cell, long long* count_cell) {
  __syncthreads();
  const int keep = kept[threadIdx.x];
  int total;
  const int rank = compact_block_exclusive<THREADS, int>(keep, wsum, &total);
  rank_cell[threadIdx.x] = keep ? rank : -1;
  if (threadIdx.x == 0) *count_cell = total;
}

// The write pass of those kernels: where the thread's candidate goes — first + its parked rank, first = start +
// offsets[cell] — or -1: not kept, or dropped at rows_cap.  (A list_ptr that breaks its promise cannot make the position
// negative.)  Holds no barrier.
__device__ __forceinline__ long long list_kept_at(const int* rank_cell, const long long* offsets, size_t cell, long long start,
                                                  long long rows_cap) {
  const int rank = rank_cell[threadIdx.x];
  if (rank < 0) return -1;
  const long long at = start + offsets[cell] + rank;
  return at >= 0 && at < rows_cap ? at : -1;
}

// ---- the host twins -------------------------------------------------------------------------------------------------------
// The resident index and token stream as the phrase rule reads them (phrase_scope.hip, class_span.hip).
inline PhIndex ph_index(const amdr_bm25* h) {
  const BmIndex& ix = h->ix;
  return PhIndex{ix.term_ptr, ix.post_doc, (long)ix.n_terms, (long)ix.n_docs, h->tok_ptr, h->tok};
}

// The staging of one host-pointer call over bm25->tscope (under bm25->mu): add() lays the regions out back to back — a
// region holds bytes + 1, aligned, so none is empty — and returns the region's offset; upload() grows the buffer and
// sends up every region that has a source; at<T>() is a region's device address, also as the workspace of a step.
struct ListStage {
  static constexpr int kMax = 16;
  size_t off[kMax], bytes[kMax], total = 0;
  const void* src[kMax];
  int n = 0;
  unsigned char* base = nullptr;
  size_t add(size_t b, const void* from = nullptr) {
    off[n] = total, bytes[n] = b, src[n] = from, ++n;
    total += list_align(b + 1);
    return off[n - 1];
  }
  int upload(amdr_bm25* bm25) {
    if (int rc = bm25->tscope.ensure(total)) return rc;
    base = bm25->tscope.as<unsigned char>();
    for (int i = 0; i < n; ++i)
      if (bytes[i] && src[i]) AMDR_HIP(hipMemcpyAsync(base + off[i], src[i], bytes[i], hipMemcpyHostToDevice, bm25->stream));
    return AMDR_OK;
  }
  template <class T>
  T* at(size_t o) const {
    return reinterpret_cast<T*>(base + o);
  }
};

// The end of a host twin, in two steps: the list pointers and the status words come back and the stream is synchronised;
// then only the rows the array names (`used`, <= rows_cap), of row_bytes each: 4 for documents, 8 for scope rows.
inline int list_fetch_heads(hipStream_t st, const long long* list_ptr_dev, int64_t n_ptr, void* out_list_ptr,
                            const int* status_dev, int64_t n_status, int32_t* out_status) {
  AMDR_HIP(hipMemcpyAsync(out_list_ptr, list_ptr_dev, (size_t)n_ptr * 8, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipMemcpyAsync(out_status, status_dev, (size_t)n_status * 4, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipStreamSynchronize(st));
  return AMDR_OK;
}
inline int list_fetch_rows(hipStream_t st, const void* rows_dev, size_t row_bytes, int64_t used, void* out_rows) {
  if (used > 0) {
    AMDR_HIP(hipMemcpyAsync(out_rows, rows_dev, (size_t)used * row_bytes, hipMemcpyDeviceToHost, st));
    AMDR_HIP(hipStreamSynchronize(st));
  }
  return AMDR_OK;
}
inline int list_fetch(hipStream_t st, int64_t n, const long long* list_ptr_dev, const int* status_dev, const void* rows_dev,
                      size_t row_bytes, int64_t* out_list_ptr, int32_t* out_status, void* out_rows) {
  if (int rc = list_fetch_heads(st, list_ptr_dev, n + 1, out_list_ptr, status_dev, n, out_status)) return rc;
  return list_fetch_rows(st, rows_dev, row_bytes, out_list_ptr[n], out_rows);
}

}  // namespace amdr

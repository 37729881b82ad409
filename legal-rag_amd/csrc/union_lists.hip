// Unions of posting lists: the root expander (sell!) and alternatives (buyer OR purchaser) resolved into ascending document
// lists on the device.
//
// No reference counterpart: the reference's BM25 channel scores bags of words (legalrag/retrieval/bm25_retriever.py:74-75)
// and has neither a stemmer nor a filter.  Here a union item — several term ids, union_rule.hpp — is resolved from the
// resident postings into ITS OWN ascending, de-duplicated document list, a virtual posting list, which
// amdr_term_scope_lists (term_scope.hip) reads as one more term, beside the lists of the phrases and the Nears
// (phrase_scope.hip).  It needs the postings only, not the token stream.
//
// The three launches of list_step.hpp, no global atomics, deterministic, nothing allocated; the grid is ONE-
// dimensional, n_items x tiles blocks of kUnThreads threads, cell = p * tiles + y (item p, tile y of kUnTile documents):
//   count   the block clears a bitmap of kUnTile bits in LDS; its waves take the item's terms round-robin; for a term the
//           wave finds the part of the posting list inside the tile (un_tile_range: two lower-bound searches on
//           wave-uniform operands, so they run on the scalar unit) and its lanes stride over that part and set bit
//           doc - tile base with an LDS atomic OR — idempotent and independent of order.  After a barrier the block
//           counts the set bits into counts[cell] and PARKS the bitmap in the workspace, 4 KiB per cell: the write pass
//           does not walk the postings again.
//   scan    compact_scan_i64_kernel over the counts: every cell's offset behind the array's start.
//   write   thread t reads its kUnPer consecutive words of the parked bitmap, the block scans their bit counts, and the
//           thread expands its bits, ascending, to docs[start + offsets[cell] + rank]; positions >= rows_cap are dropped.
//           The block of tile 0 writes the item's list_ptr entry, clamped to rows_cap, and its status: 0, or 2 (rows
//           dropped; there is no 1, a union has no driver to be too long).
// One list array.  The call CONTINUES the array a span step began on the same stream: list_ptr has n_before + n_items + 1
// entries of which the first n_before + 1 are written; start = list_ptr[n_before] is read ON THE DEVICE by the write pass
// (no host synchronise), the entries n_before + 1 .. are written, and the documents go behind `start`.  n_before = 0
// starts an array: start is 0 and the call writes list_ptr[0] itself.
// Every barrier sits under a block-uniform condition: the term loop holds none, and nothing returns before the last one.
// LDS: the bitmap (4 096 B) and the scan's wave sums.  Workspace per cell: two i64 and the 4 KiB bitmap.
#include "list_step.hpp"
#include "union_rule.hpp"

#include <mutex>

using namespace amdr;

namespace {

constexpr int kUnWaves = kUnThreads / 64;
static_assert(kUnThreads % 64 == 0, "whole waves");

// Workspace (list_work): a cell's payload is its parked bitmap u32 [kUnWords]
constexpr size_t kUnCellBytes = kUnWords * sizeof(unsigned);

__global__ __launch_bounds__(kUnThreads) void union_count_kernel(UnIndex I, const long long* __restrict__ item_ptr,
                                                                const int* __restrict__ item_terms, long long tiles,
                                                                long long* __restrict__ counts, uint4* __restrict__ parked) {
  __shared__ unsigned bits[kUnWords];
  __shared__ int wsum[kUnWaves + 1];
  const long long cell = blockIdx.x;
  const long long p = cell / tiles, tile = cell - p * tiles;
#pragma unroll
  for (int j = 0; j < kUnPer; ++j) bits[threadIdx.x * kUnPer + j] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (wave-uniform by construction: say so)
  const long long b = item_ptr[p], e = item_ptr[p + 1];
  for (long long j = b + wave; j < e; j += kUnWaves) {  // wave-uniform; no barrier inside
    const int t = __builtin_amdgcn_readfirstlane(item_terms[j]);
    long long lo, hi;
    if (!un_tile_range(I, t, tile, &lo, &hi)) continue;
    for (long long i = lo + lane; i < hi; i += 64) {
      const long long doc = I.post_doc[i];  // inside the tile: [lo, hi) is its part of an ascending list
      // (the mask changes no word of such a list; a list that breaks its promise cannot leave the bitmap)
      atomicOr(&bits[un_bit_word(doc, tile) & (kUnWords - 1)], un_bit_mask(doc));
    }
  }
  __syncthreads();
  uint4 w;
  w.x = bits[threadIdx.x * kUnPer + 0], w.y = bits[threadIdx.x * kUnPer + 1];
  w.z = bits[threadIdx.x * kUnPer + 2], w.w = bits[threadIdx.x * kUnPer + 3];
  parked[(size_t)cell * kUnThreads + threadIdx.x] = w;
  int total;
  (void)compact_block_exclusive<kUnThreads, int>(un_popcount(w.x) + un_popcount(w.y) + un_popcount(w.z) + un_popcount(w.w),
                                                 wsum, &total);
  if (threadIdx.x == 0) counts[cell] = total;
}

__global__ __launch_bounds__(kUnThreads) void union_write_kernel(long long tiles, long long n_before, long long rows_cap,
                                                                const long long* __restrict__ offsets,
                                                                const uint4* __restrict__ parked, long long* list_ptr,
                                                                int* __restrict__ docs, int* __restrict__ status) {
  __shared__ int wsum[kUnWaves + 1];
  const long long cell = blockIdx.x;
  const long long p = cell / tiles, tile = cell - p * tiles;
  const long long start = list_start(list_ptr, n_before);
  if (tile == 0 && threadIdx.x == 0)
    status[p] = list_write_header(list_ptr, n_before, p, start + offsets[p * tiles], start + offsets[(p + 1) * tiles], rows_cap);
  const uint4 w = parked[(size_t)cell * kUnThreads + threadIdx.x];
  const unsigned word[kUnPer] = {w.x, w.y, w.z, w.w};
  int mine = 0;
#pragma unroll
  for (int j = 0; j < kUnPer; ++j) mine += un_popcount(word[j]);
  int total;
  const int rank = compact_block_exclusive<kUnThreads, int>(mine, wsum, &total);
  long long at = start + offsets[cell] + rank;
#pragma unroll
  for (int j = 0; j < kUnPer; ++j) at += un_expand_word(word[j], tile, (int)threadIdx.x * kUnPer + j, at, rows_cap, docs);
}

struct UnOut {
  long long* list_ptr;
  int* docs;
  int* status;
};

int un_launch(const UnIndex& I, const long long* item_ptr, const int* item_terms, int64_t n_items, int64_t n_before,
              int64_t rows_cap, const UnOut& o, unsigned char* work, hipStream_t st) {
  const long long tiles = un_tiles(I.n_docs), cells = (long long)n_items * tiles;
  const dim3 grid((unsigned)cells);
  return list_launch(
      st, n_items, n_before, (size_t)cells, kUnCellBytes, o.list_ptr, work,
      [&](long long* counts, unsigned char* parked) {
        hipLaunchKernelGGL(union_count_kernel, grid, dim3(kUnThreads), 0, st, I, item_ptr, item_terms, tiles, counts,
                           (uint4*)parked);
      },
      [&](const long long* offsets, const unsigned char* parked) {
        hipLaunchKernelGGL(union_write_kernel, grid, dim3(kUnThreads), 0, st, tiles, (long long)n_before, (long long)rows_cap,
                           offsets, (const uint4*)parked, o.list_ptr, o.docs, o.status);
      });
}

// sizes every entry point refuses (nothing is enqueued); *cells: the cells of the launch
int un_check_sizes(const char* who, int64_t n_items, int64_t n_docs, int64_t n_before, int64_t rows_cap, long long* cells) {
  AMDR_REQUIRE(n_items >= 0 && n_docs >= 0 && n_before >= 0 && rows_cap >= 0, "%s: a negative size", who);
  AMDR_REQUIRE(un_cells(n_items, n_docs, cells), "%s: %lld items x %lld tiles of %d documents are more than the %lld cells of "
               "one launch", who, (long long)n_items, un_tiles(n_docs), kUnTile, kUnMaxCells);
  return AMDR_OK;
}

UnIndex un_index(const amdr_bm25* h) {
  const BmIndex& ix = h->ix;
  return UnIndex{ix.term_ptr, ix.post_doc, (long)ix.n_terms, (long)ix.n_docs};
}

}  // namespace

extern "C" {

int amdr_union_lists_plan(int64_t n_items, int64_t n_docs, int64_t* work_bytes) {
  AMDR_REQUIRE(work_bytes != nullptr, "union_lists_plan: null");
  long long cells = 0;
  int rc = un_check_sizes("union_lists_plan", n_items, n_docs, 0, 0, &cells);
  if (rc) return rc;
  *work_bytes = (int64_t)list_work((size_t)cells, kUnCellBytes).total;
  return AMDR_OK;
}

int amdr_union_lists_device(amdr_bm25_t* bm25, const int64_t* item_ptr_dev, const int32_t* item_terms_dev, int64_t n_items,
                            int64_t n_before, int64_t rows_cap, int64_t* list_ptr_dev, int32_t* docs_dev,
                            int32_t* out_status_dev, void* work_dev, int64_t work_bytes, void* stream) {
  static const char* const who = "union_lists";
  AMDR_REQUIRE(bm25 != nullptr, "%s: null handle", who);
  long long cells = 0;
  int rc = un_check_sizes(who, n_items, bm25->ix.n_docs, n_before, rows_cap, &cells);
  if (rc) return rc;
  AMDR_REQUIRE(list_ptr_dev != nullptr, "%s: null list_ptr", who);
  AMDR_REQUIRE(n_items == 0 || (item_ptr_dev && item_terms_dev && out_status_dev), "%s: null operand", who);
  AMDR_REQUIRE(rows_cap == 0 || docs_dev, "%s: null docs", who);
  const size_t need = n_items ? list_work((size_t)cells, kUnCellBytes).total : 0;
  if ((rc = list_check_work(who, work_dev, work_bytes, need))) return rc;
  AMDR_HIP(hipSetDevice(bm25->device));
  const UnOut o{(long long*)list_ptr_dev, docs_dev, out_status_dev};
  return un_launch(un_index(bm25), (const long long*)item_ptr_dev, item_terms_dev, n_items, n_before, rows_cap, o,
                   static_cast<unsigned char*>(work_dev), (hipStream_t)stream);
}

int amdr_union_lists(amdr_bm25_t* bm25, const int64_t* item_ptr, const int32_t* item_terms, int64_t n_items, int64_t rows_cap,
                     int64_t* out_list_ptr, int32_t* out_docs, int32_t* out_status) {
  static const char* const who = "union_lists";
  AMDR_REQUIRE(bm25 != nullptr, "%s: null handle", who);
  AMDR_REQUIRE(n_items >= 0 && rows_cap >= 0, "%s: a negative size", who);
  AMDR_REQUIRE(out_list_ptr != nullptr, "%s: null out_list_ptr", who);
  AMDR_REQUIRE(n_items == 0 || out_status, "%s: null out_status", who);
  AMDR_REQUIRE(rows_cap == 0 || out_docs, "%s: null out_docs", who);
  std::lock_guard<std::mutex> g(bm25->mu);
  long long cells = 0;
  int rc = un_check_sizes(who, n_items, bm25->ix.n_docs, 0, rows_cap, &cells);
  if (rc) return rc;
  const int bad = un_validate(item_ptr, item_terms, n_items);
  AMDR_REQUIRE(bad == kUnValid, "%s: %s", who, un_error_text(bad));
  if (n_items == 0) {
    out_list_ptr[0] = 0;
    return AMDR_OK;
  }
  AMDR_HIP(hipSetDevice(bm25->device));
  // The staging buffer: the item arrays, the outputs, the workspace.
  ListStage s;
  const size_t a_ptr = s.add((size_t)(n_items + 1) * 8, item_ptr), a_terms = s.add((size_t)item_ptr[n_items] * 4, item_terms);
  const size_t a_list_ptr = s.add((size_t)(n_items + 1) * 8), a_docs = s.add((size_t)rows_cap * 4);
  const size_t a_status = s.add((size_t)n_items * 4);
  const size_t a_work = s.add(list_work((size_t)cells, kUnCellBytes).total);
  if ((rc = s.upload(bm25))) return rc;
  const UnOut o{s.at<long long>(a_list_ptr), s.at<int>(a_docs), s.at<int>(a_status)};
  hipStream_t st = bm25->stream;
  if ((rc = un_launch(un_index(bm25), s.at<long long>(a_ptr), s.at<int>(a_terms), n_items, 0, rows_cap, o,
                      s.at<unsigned char>(a_work), st)))
    return rc;
  // (used <= rows_cap: only the documents the lists name come back)
  return list_fetch(st, n_items, o.list_ptr, o.status, o.docs, 4, out_list_ptr, out_status, out_docs);
}

}  // extern "C"

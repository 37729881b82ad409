// Required and excluded terms: Boolean term constraints resolved into a scope table on the device.
//
// No reference counterpart: the reference's BM25 channel only prefers a query's terms (legalrag/retrieval/
// bm25_retriever.py:74-75 scores and sorts the whole corpus) and HybridRetriever.search has no filter argument; a caller
// who wants "articles that contain seller and goods but not buyer" over-fetches and filters on the host.  Here the step
// from term constraints to the ascending row lists the scoped kernels take (scope.hip) runs on the resident term-major
// postings (BmIndex::term_ptr / post_doc), without a host synchronise: the table it writes is handed unchanged to
// amdr_scope_*_search_device and amdr_hybrid_scope_device on the same stream.  The rule — what a group and a constraint
// are, which list drives a constraint — is term_scope_rule.hpp's, shared with the host check.  A call may bring VIRTUAL
// posting lists (amdr_term_scope_lists*: the phrase lists of phrase_scope.hip, written just before on the same stream):
// term id n_terms + p names the p-th of them wherever a term id may stand.
//
// Three launches, no atomics, deterministic; grid = (x = constraint, y = tile of kTsTile candidates of its driver):
//   count   a block evaluates its tile's candidates (thread t takes candidates t, t + 256, ...: the driver loads are
//           coalesced; the binary searches behind them diverge by nature), parks the keep bits and writes its keep count
//           to counts[c][tile]; a driver longer than cand_max: zero counts and status[c] = 1.
//   scan    compact_scan_i64_kernel over the flattened [n_cons x tiles] counts: every tile's write offset, and with it
//           scope_ptr[c] = the offset of tile 0 of c.
//   write   compact_tile_scan inside the tile; kept candidate -> rows[offset + rank]; positions >= rows_cap are dropped
//           and their constraints get status[c] = 2; scope_ptr is written clamped to rows_cap.
// The constraint is the grid's x in every call (x holds 2^31 - 1 blocks, y 65 535): a batch may carry more than 65 535
// constraints, and cand_max <= 65 535 tiles is far past any resident index.
// Every barrier sits under a block-uniform condition: the driver is computed by one thread and read from LDS by all.
#include "list_step.hpp"
#include "term_scope_rule.hpp"

#include <mutex>

using namespace amdr;

namespace {

constexpr int kTsThreads = 256;
constexpr int kTsPer = kTsTile / kTsThreads;  // candidates per thread
static_assert(kTsPer * kTsThreads == kTsTile && kTsPer <= 32, "one keep bit per candidate of a thread");

// Workspace (list_work): a cell is a tile of a constraint, its payload the keep bits u32 [256]
constexpr size_t kTsCellBytes = kTsThreads * sizeof(unsigned);
size_t ts_cells(int64_t n_cons, int64_t cand_max) { return (size_t)n_cons * (size_t)ts_tiles(cand_max); }

// the block's driver: computed by thread 0, read by all (ends with a barrier)
__device__ __forceinline__ TsDriver ts_block_driver(const TsIndex& I, const TsCons& C, long c, TsDriver* slot) {
  if (threadIdx.x == 0) *slot = ts_driver(I, C, c);
  __syncthreads();
  return *slot;
}

__global__ __launch_bounds__(kTsThreads) void term_scope_count_kernel(TsIndex I, TsCons C, long long cand_max,
                                                                     long long* __restrict__ counts,
                                                                     unsigned* __restrict__ bits, int* __restrict__ status) {
  __shared__ TsDriver drv;
  __shared__ int wsum[kTsThreads / 64 + 1];
  const long c = blockIdx.x;
  const long long tile = blockIdx.y, tiles = gridDim.y;
  const size_t cell = (size_t)c * tiles + tile;
  const TsDriver D = ts_block_driver(I, C, c, &drv);
  const bool over = D.len > cand_max;
  if (tile == 0 && threadIdx.x == 0) status[c] = over ? kTsCandOverflow : kTsOk;
  const long long i0 = tile * kTsTile;
  if (over || i0 >= D.len) {  // block-uniform
    if (threadIdx.x == 0) counts[cell] = 0;
    return;
  }
  unsigned keep = 0;
#pragma unroll
  for (int u = 0; u < kTsPer; ++u) {
    const long long i = i0 + (long long)u * kTsThreads + threadIdx.x;
    if (i < D.len && ts_qualifies(I, C, c, D, ts_candidate(I, C, D, i))) keep |= 1u << u;
  }
  bits[cell * kTsThreads + threadIdx.x] = keep;
  int total;
  (void)compact_block_exclusive<kTsThreads, int>(__popc(keep), wsum, &total);
  if (threadIdx.x == 0) counts[cell] = total;
}

__global__ __launch_bounds__(kTsThreads) void term_scope_write_kernel(TsIndex I, TsCons C, long long cand_max,
                                                                     long long rows_cap,
                                                                     const long long* __restrict__ offsets,
                                                                     const unsigned* __restrict__ bits,
                                                                     long long* __restrict__ scope_ptr,
                                                                     long long* __restrict__ rows, int* __restrict__ status) {
  __shared__ TsDriver drv;
  __shared__ int lds[kTsThreads * kTsPer + kTsThreads / 64 + 1];
  const long c = blockIdx.x;
  const long long tile = blockIdx.y, tiles = gridDim.y;
  const size_t cell = (size_t)c * tiles + tile;
  if (tile == 0 && threadIdx.x == 0) {
    const int s = list_write_header(scope_ptr, 0, c, offsets[(size_t)c * tiles], offsets[(size_t)(c + 1) * tiles], rows_cap);
    if (s != kTsOk) status[c] = s;  // (a constraint over cand_max has no row: its 1 stays)
  }
  const TsDriver D = ts_block_driver(I, C, c, &drv);
  const long long i0 = tile * kTsTile;
  if (D.len > cand_max || i0 >= D.len) return;  // block-uniform
  const unsigned keep = bits[cell * kTsThreads + threadIdx.x];
  int rank[kTsPer];
  (void)compact_tile_scan<kTsThreads, kTsPer>(keep, lds, rank);
  const long long off = offsets[cell];
#pragma unroll
  for (int u = 0; u < kTsPer; ++u) {
    if (!((keep >> u) & 1u)) continue;
    const long long i = i0 + (long long)u * kTsThreads + threadIdx.x;  // (a kept candidate lies inside the driver)
    const long long at = off + rank[u];
    if (at < rows_cap) rows[at] = ts_candidate(I, C, D, i);
  }
}

struct TsOut {
  long long* scope_ptr;
  long long* rows;
  int* status;
};

int ts_launch(const TsIndex& I, const TsCons& C, int64_t n_cons, int64_t cand_max, int64_t rows_cap, const TsOut& o,
              unsigned char* work, hipStream_t st) {
  const dim3 grid((unsigned)n_cons, (unsigned)ts_tiles(cand_max));
  return list_launch(
      st, n_cons, 0, ts_cells(n_cons, cand_max), kTsCellBytes, o.scope_ptr, work,
      [&](long long* counts, unsigned char* bits) {
        hipLaunchKernelGGL(term_scope_count_kernel, grid, dim3(kTsThreads), 0, st, I, C, (long long)cand_max, counts,
                           (unsigned*)bits, o.status);
      },
      [&](const long long* offsets, const unsigned char* bits) {
        hipLaunchKernelGGL(term_scope_write_kernel, grid, dim3(kTsThreads), 0, st, I, C, (long long)cand_max, (long long)rows_cap,
                           offsets, (const unsigned*)bits, o.scope_ptr, o.rows, o.status);
      });
}

// sizes both entry points refuse (nothing is enqueued)
int ts_check_sizes(const char* who, int64_t n_base, int64_t n_cons, int64_t n_groups, int64_t cand_max, int64_t rows_cap) {
  AMDR_REQUIRE(n_base >= 0 && n_cons >= 0 && n_groups >= 0 && cand_max >= 0 && rows_cap >= 0, "%s: a negative size", who);
  AMDR_REQUIRE(n_cons <= INT32_MAX && n_base <= INT32_MAX, "%s: more than 2^31 - 1 constraints or base scopes", who);
  AMDR_REQUIRE(ts_tiles(cand_max) <= kGridYMax, "%s: cand_max=%lld beyond %d tiles of %d candidates", who,
               (long long)cand_max, kGridYMax, kTsTile);
  return AMDR_OK;
}

}  // namespace

extern "C" {

int amdr_term_scope_plan(int64_t n_cons, int64_t cand_max, int64_t* work_bytes) {
  AMDR_REQUIRE(work_bytes != nullptr, "term_scope_plan: null");
  int rc = ts_check_sizes("term_scope_plan", 0, n_cons, 0, cand_max, 0);
  if (rc) return rc;
  *work_bytes = (int64_t)list_work(ts_cells(n_cons, cand_max), kTsCellBytes).total;
  return AMDR_OK;
}

int amdr_term_scope_lists_device(amdr_bm25_t* bm25, const int64_t* grp_ptr_dev, const int32_t* grp_kind_dev,
                                 const int64_t* grp_term_ptr_dev, const int32_t* grp_terms_dev, const int64_t* base_ptr_dev,
                                 const int64_t* base_rows_dev, const int32_t* cons_base_dev, const int64_t* x_ptr_dev,
                                 const int32_t* x_doc_dev, int64_t n_x, int64_t n_base, int64_t n_cons, int64_t n_groups,
                                 int64_t cand_max, int64_t rows_cap, int64_t* out_scope_ptr_dev, int64_t* out_rows_dev,
                                 int32_t* out_status_dev, void* work_dev, int64_t work_bytes, void* stream) {
  AMDR_REQUIRE(bm25 != nullptr, "term_scope: null handle");
  int rc = ts_check_sizes("term_scope", n_base, n_cons, n_groups, cand_max, rows_cap);
  if (rc) return rc;
  AMDR_REQUIRE(n_x >= 0 && n_x <= INT32_MAX, "term_scope: n_x=%lld", (long long)n_x);
  AMDR_REQUIRE(n_x == 0 || (x_ptr_dev && x_doc_dev), "term_scope: null virtual lists");
  AMDR_REQUIRE(out_scope_ptr_dev != nullptr, "term_scope: null out_scope_ptr");
  AMDR_REQUIRE(n_cons == 0 || (grp_ptr_dev && grp_term_ptr_dev && cons_base_dev && out_status_dev), "term_scope: null operand");
  AMDR_REQUIRE(n_groups == 0 || (grp_kind_dev && grp_terms_dev), "term_scope: null group arrays");
  AMDR_REQUIRE(n_base == 0 || base_ptr_dev, "term_scope: null base_ptr");
  AMDR_REQUIRE(rows_cap == 0 || out_rows_dev, "term_scope: null out_rows");
  const size_t need = n_cons ? list_work(ts_cells(n_cons, cand_max), kTsCellBytes).total : 0;
  if ((rc = list_check_work("term_scope", work_dev, work_bytes, need))) return rc;
  AMDR_HIP(hipSetDevice(bm25->device));
  const BmIndex& ix = bm25->ix;
  const TsIndex I{ix.term_ptr, ix.post_doc, (long)ix.n_terms, (long)ix.n_docs, (const long long*)x_ptr_dev, x_doc_dev, (long)n_x};
  const TsCons C{(const long long*)grp_ptr_dev, grp_kind_dev, (const long long*)grp_term_ptr_dev, grp_terms_dev,
                 (const long long*)base_ptr_dev, (const long long*)base_rows_dev, cons_base_dev, (int)n_base};
  const TsOut o{(long long*)out_scope_ptr_dev, (long long*)out_rows_dev, out_status_dev};
  return ts_launch(I, C, n_cons, cand_max, rows_cap, o, static_cast<unsigned char*>(work_dev), (hipStream_t)stream);
}

int amdr_term_scope_device(amdr_bm25_t* bm25, const int64_t* grp_ptr_dev, const int32_t* grp_kind_dev,
                           const int64_t* grp_term_ptr_dev, const int32_t* grp_terms_dev, const int64_t* base_ptr_dev,
                           const int64_t* base_rows_dev, const int32_t* cons_base_dev, int64_t n_base, int64_t n_cons,
                           int64_t n_groups, int64_t cand_max, int64_t rows_cap, int64_t* out_scope_ptr_dev,
                           int64_t* out_rows_dev, int32_t* out_status_dev, void* work_dev, int64_t work_bytes, void* stream) {
  return amdr_term_scope_lists_device(bm25, grp_ptr_dev, grp_kind_dev, grp_term_ptr_dev, grp_terms_dev, base_ptr_dev,
                                      base_rows_dev, cons_base_dev, nullptr, nullptr, 0, n_base, n_cons, n_groups, cand_max,
                                      rows_cap, out_scope_ptr_dev, out_rows_dev, out_status_dev, work_dev, work_bytes, stream);
}

int amdr_term_scope_lists(amdr_bm25_t* bm25, const int64_t* grp_ptr, const int32_t* grp_kind, const int64_t* grp_term_ptr,
                          const int32_t* grp_terms, const int64_t* base_ptr, const int64_t* base_rows,
                          const int32_t* cons_base, const int64_t* x_ptr, const int32_t* x_doc, int64_t n_x, int64_t n_base,
                          int64_t n_cons, int64_t n_groups, int64_t cand_max, int64_t rows_cap, int64_t* out_scope_ptr,
                          int64_t* out_rows, int32_t* out_status) {
  AMDR_REQUIRE(bm25 != nullptr, "term_scope: null handle");
  int rc = ts_check_sizes("term_scope", n_base, n_cons, n_groups, cand_max, rows_cap);
  if (rc) return rc;
  AMDR_REQUIRE(out_scope_ptr != nullptr, "term_scope: null out_scope_ptr");
  AMDR_REQUIRE(n_cons == 0 || out_status, "term_scope: null out_status");
  AMDR_REQUIRE(rows_cap == 0 || out_rows, "term_scope: null out_rows");
  std::lock_guard<std::mutex> g(bm25->mu);
  const int bad = ts_validate(grp_ptr, grp_kind, grp_term_ptr, base_ptr, base_rows, cons_base, n_base, n_cons, n_groups,
                              bm25->ix.n_docs);
  AMDR_REQUIRE(bad == kTsValid, "term_scope: %s", ts_error_text(bad));
  AMDR_REQUIRE(n_x <= INT32_MAX, "term_scope: n_x=%lld", (long long)n_x);
  const int bad_x = ts_validate_lists(x_ptr, x_doc, n_x, bm25->ix.n_docs);
  AMDR_REQUIRE(bad_x == kTsValid, "term_scope: %s", ts_error_text(bad_x));
  const int64_t n_x_docs = n_x ? x_ptr[n_x] : 0;
  const int64_t n_terms_all = grp_term_ptr[n_groups], n_base_rows = n_base ? base_ptr[n_base] : 0;
  AMDR_REQUIRE(n_terms_all == 0 || grp_terms, "term_scope: null grp_terms");
  if (n_cons == 0) {
    out_scope_ptr[0] = 0;
    return AMDR_OK;
  }
  AMDR_HIP(hipSetDevice(bm25->device));
  // The staging buffer: the seven operand arrays and the two of the virtual lists, the outputs, the workspace.
  ListStage s;
  const size_t a_grp_ptr = s.add((size_t)(n_cons + 1) * 8, grp_ptr), a_grp_kind = s.add((size_t)n_groups * 4, grp_kind);
  const size_t a_grp_term_ptr = s.add((size_t)(n_groups + 1) * 8, grp_term_ptr);
  const size_t a_grp_terms = s.add((size_t)n_terms_all * 4, grp_terms);
  const size_t a_base_ptr = s.add((size_t)(n_base + 1) * 8, base_ptr), a_base_rows = s.add((size_t)n_base_rows * 8, base_rows);
  const size_t a_cons_base = s.add((size_t)n_cons * 4, cons_base);
  const size_t a_x_ptr = s.add(n_x ? (size_t)(n_x + 1) * 8 : 0, x_ptr), a_x_doc = s.add((size_t)n_x_docs * 4, x_doc);
  const size_t a_scope_ptr = s.add((size_t)(n_cons + 1) * 8), a_rows = s.add((size_t)rows_cap * 8);
  const size_t a_status = s.add((size_t)n_cons * 4);
  const size_t a_work = s.add(list_work(ts_cells(n_cons, cand_max), kTsCellBytes).total);
  if ((rc = s.upload(bm25))) return rc;
  hipStream_t st = bm25->stream;
  if (n_base == 0) AMDR_HIP(hipMemsetAsync(s.at<void>(a_base_ptr), 0, 8, st));
  const BmIndex& ix = bm25->ix;
  const TsIndex I{ix.term_ptr, ix.post_doc, (long)ix.n_terms, (long)ix.n_docs, s.at<long long>(a_x_ptr), s.at<int>(a_x_doc),
                  (long)n_x};
  const TsCons C{s.at<long long>(a_grp_ptr), s.at<int>(a_grp_kind), s.at<long long>(a_grp_term_ptr), s.at<int>(a_grp_terms),
                 s.at<long long>(a_base_ptr), s.at<long long>(a_base_rows), s.at<int>(a_cons_base), (int)n_base};
  const TsOut o{s.at<long long>(a_scope_ptr), s.at<long long>(a_rows), s.at<int>(a_status)};
  if ((rc = ts_launch(I, C, n_cons, cand_max, rows_cap, o, s.at<unsigned char>(a_work), st))) return rc;
  // (used <= rows_cap: only the rows the table names come back)
  return list_fetch(st, n_cons, o.scope_ptr, o.status, o.rows, 8, out_scope_ptr, out_status, out_rows);
}

int amdr_term_scope(amdr_bm25_t* bm25, const int64_t* grp_ptr, const int32_t* grp_kind, const int64_t* grp_term_ptr,
                    const int32_t* grp_terms, const int64_t* base_ptr, const int64_t* base_rows, const int32_t* cons_base,
                    int64_t n_base, int64_t n_cons, int64_t n_groups, int64_t cand_max, int64_t rows_cap,
                    int64_t* out_scope_ptr, int64_t* out_rows, int32_t* out_status) {
  return amdr_term_scope_lists(bm25, grp_ptr, grp_kind, grp_term_ptr, grp_terms, base_ptr, base_rows, cons_base, nullptr,
                               nullptr, 0, n_base, n_cons, n_groups, cand_max, rows_cap, out_scope_ptr, out_rows, out_status);
}

}  // extern "C"

// Phrase constraints: exact token sequences resolved into ascending document lists on the device.
//
// No reference counterpart: the reference's BM25 channel scores bags of words (legalrag/retrieval/bm25_retriever.py:74-75)
// and keeps no token order anywhere.  Here the BM25 handle holds, beside its term-major postings, the TOKEN STREAM of the
// corpus (amdr_bm25_set_tokens: the forward index, 4 B per token), and a phrase is resolved into ITS OWN ascending
// document list — a virtual posting list — which amdr_term_scope_lists (term_scope.hip) reads as one more term.  The rule
// — what a phrase is, which posting list drives it — is phrase_rule.hpp's, shared with the host check.
//
// Three launches in the shape of term_scope.hip, no atomics, deterministic; grid = (x = phrase, y = tile of kPhTile = 256
// candidates of its driver, one per thread):
//   count   two phases inside the tile.  (1) thread t tests the conjunction for candidate t — posting_has on the other
//           tokens, as term_scope does — and the survivors are compacted into an LDS list.  (2) one WAVE per survivor
//           scans that document's token run: lane l tests the start positions l, l + 64, ... and a wave vote ends the
//           document at the first round with a hit.  The block then ranks its kept candidates, parks rank-or-minus-one
//           per candidate and writes its keep count to counts[p][tile]; a driver longer than cand_max: zero counts and
//           status[p] = 1.
//   scan    compact_scan_i64_kernel over the flattened [n_phr x tiles] counts: every tile's write offset.
//   write   kept candidate -> docs[offset + rank]; positions >= rows_cap are dropped and their phrases get status[p] = 2;
//           list_ptr is written clamped to rows_cap.
// The tile is 256 candidates: the block's LDS is the survivor list (512 B), the keep flags (256 B), the phrase (64 B) and
// the scan's wave sums; the parked ranks are 1 KiB per tile, the cell size of term_scope's keep bits; and four waves share
// the survivors of one tile, so one long document delays three others at most.
// Every barrier sits under a block-uniform condition: the driver is computed by one thread and read from LDS by all, the
// survivor count comes from the block scan, and the wave loop of phase 2 holds no barrier.
#include "bm25_handle.hpp"
#include "compact.hpp"
#include "phrase_rule.hpp"

#include <memory>
#include <mutex>
#include <new>

using namespace amdr;

namespace {

constexpr int kPhThreads = kPhTile;
constexpr int kPhWaves = kPhThreads / 64;
constexpr size_t kPhAlign = 256;
static_assert(kPhThreads % 64 == 0 && kPhLanes == 64, "whole waves; a wave is the scan's lane count");

size_t ph_align(size_t b) { return (b + kPhAlign - 1) / kPhAlign * kPhAlign; }

// Workspace: counts i64 [n_phr * tiles] | offsets i64 [n_phr * tiles + 1] | rank-or-minus-one i32 [n_phr * tiles * 256]
struct PhWork {
  size_t off_counts, off_offsets, off_rank, total;
};
PhWork ph_work(int64_t n_phr, int64_t cand_max) {
  const size_t cells = (size_t)n_phr * (size_t)ph_tiles(cand_max);
  PhWork w;
  w.off_counts = 0;
  w.off_offsets = ph_align(cells * sizeof(long long));
  w.off_rank = w.off_offsets + ph_align((cells + 1) * sizeof(long long));
  w.total = w.off_rank + ph_align(cells * kPhThreads * sizeof(int));
  return w;
}

// The block's phrase and driver: the length by all, the tokens into LDS by the first L threads (a length outside
// 2 .. kPhMaxLen reads none), the driver by thread 0; ends with a barrier.  Returns the phrase's length.
__device__ __forceinline__ int ph_block_phrase(const PhIndex& I, const long long* __restrict__ phr_ptr,
                                               const int* __restrict__ phr_terms, long p, int* terms, PhDriver* slot) {
  const long long b = phr_ptr[p], L = phr_ptr[p + 1] - b;
  const bool sized = L >= 2 && L <= kPhMaxLen;  // block-uniform
  if (sized && threadIdx.x < L) terms[threadIdx.x] = phr_terms[b + threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) *slot = sized ? ph_driver(I, terms, L) : PhDriver{-1, -1, 0, 0};
  __syncthreads();
  return sized ? (int)L : 0;
}

__global__ __launch_bounds__(kPhThreads) void phrase_count_kernel(PhIndex I, const long long* __restrict__ phr_ptr,
                                                                 const int* __restrict__ phr_terms, long long cand_max,
                                                                 long long* __restrict__ counts, int* __restrict__ rank_out,
                                                                 int* __restrict__ status) {
  __shared__ PhDriver drv;
  __shared__ int terms[kPhMaxLen];
  __shared__ unsigned short surv[kPhThreads];
  __shared__ unsigned char kept[kPhThreads];
  __shared__ int wsum[kPhWaves + 1];
  const long p = blockIdx.x;
  const long long tile = blockIdx.y, tiles = gridDim.y;
  const size_t cell = (size_t)p * tiles + tile;
  const int L = ph_block_phrase(I, phr_ptr, phr_terms, p, terms, &drv);
  const PhDriver D = drv;
  const bool over = D.len > cand_max;
  if (tile == 0 && threadIdx.x == 0) status[p] = over ? kTsCandOverflow : kTsOk;
  const long long i0 = tile * kPhTile;
  if (over || i0 >= D.len) {  // block-uniform
    if (threadIdx.x == 0) counts[cell] = 0;
    return;
  }
  // phase 1: the conjunction, one candidate per thread
  const long long i = i0 + threadIdx.x;
  const bool all = i < D.len && ph_has_all(I, terms, L, D, I.post_doc[D.begin + i]);
  kept[threadIdx.x] = 0;
  int n_surv;
  const int slot = compact_block_exclusive<kPhThreads, int>(all ? 1 : 0, wsum, &n_surv);
  if (all) surv[slot] = (unsigned short)threadIdx.x;
  __syncthreads();
  // phase 2: one wave per survivor (n_surv is block-uniform; the loop holds no barrier)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = wave; s < n_surv; s += kPhWaves) {
    const int t = surv[s];
    const long long doc = I.post_doc[D.begin + i0 + t];
    const long long last = ph_last_start(I, doc, L);
    bool found = false;
    for (long long base = I.doc_ptr[doc]; base <= last && !found; base += kPhLanes)  // wave-uniform
      found = __ballot(ph_lane_hit(I, terms, L, base, lane, last)) != 0;
    if (lane == 0) kept[t] = found ? 1 : 0;
  }
  __syncthreads();
  const int keep = kept[threadIdx.x];
  int total;
  const int rank = compact_block_exclusive<kPhThreads, int>(keep, wsum, &total);
  rank_out[cell * kPhThreads + threadIdx.x] = keep ? rank : -1;
  if (threadIdx.x == 0) counts[cell] = total;
}

__global__ __launch_bounds__(kPhThreads) void phrase_write_kernel(PhIndex I, const long long* __restrict__ phr_ptr,
                                                                 const int* __restrict__ phr_terms, long long cand_max,
                                                                 long n_phr, long long rows_cap,
                                                                 const long long* __restrict__ offsets,
                                                                 const int* __restrict__ rank_in,
                                                                 long long* __restrict__ list_ptr, int* __restrict__ docs,
                                                                 int* __restrict__ status) {
  __shared__ PhDriver drv;
  __shared__ int terms[kPhMaxLen];
  const long p = blockIdx.x;
  const long long tile = blockIdx.y, tiles = gridDim.y;
  const size_t cell = (size_t)p * tiles + tile;
  if (tile == 0 && threadIdx.x == 0) {
    const long long b = offsets[(size_t)p * tiles], e = offsets[(size_t)(p + 1) * tiles];
    list_ptr[p] = b < rows_cap ? b : rows_cap;
    if (p == n_phr - 1) list_ptr[n_phr] = e < rows_cap ? e : rows_cap;
    if (e > b && e > rows_cap) status[p] = kTsRowsOverflow;  // (a phrase over cand_max has no row: its 1 stays)
  }
  (void)ph_block_phrase(I, phr_ptr, phr_terms, p, terms, &drv);
  const PhDriver D = drv;
  const long long i0 = tile * kPhTile;
  if (D.len > cand_max || i0 >= D.len) return;  // block-uniform
  const int rank = rank_in[cell * kPhThreads + threadIdx.x];
  if (rank < 0) return;  // (no barrier follows)
  const long long at = offsets[cell] + rank;
  if (at < rows_cap) docs[at] = I.post_doc[D.begin + i0 + threadIdx.x];  // (a kept candidate lies inside the driver)
}

struct PhOut {
  long long* list_ptr;
  int* docs;
  int* status;
};

int ph_launch(const PhIndex& I, const long long* phr_ptr, const int* phr_terms, int64_t n_phr, int64_t cand_max,
              int64_t rows_cap, const PhOut& o, unsigned char* work, hipStream_t st) {
  if (n_phr == 0) {
    AMDR_HIP(hipMemsetAsync(o.list_ptr, 0, sizeof(long long), st));
    return AMDR_OK;
  }
  const PhWork w = ph_work(n_phr, cand_max);
  const long long tiles = ph_tiles(cand_max);
  long long* counts = reinterpret_cast<long long*>(work + w.off_counts);
  long long* offsets = reinterpret_cast<long long*>(work + w.off_offsets);
  int* rank = reinterpret_cast<int*>(work + w.off_rank);
  const dim3 grid((unsigned)n_phr, (unsigned)tiles);
  hipLaunchKernelGGL(phrase_count_kernel, grid, dim3(kPhThreads), 0, st, I, phr_ptr, phr_terms, (long long)cand_max, counts,
                     rank, o.status);
  AMDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(compact_scan_i64_kernel, dim3(1), dim3(kCompactScanThreads), 0, st, (const long long*)counts,
                     (long)(n_phr * tiles), offsets);
  AMDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(phrase_write_kernel, grid, dim3(kPhThreads), 0, st, I, phr_ptr, phr_terms, (long long)cand_max,
                     (long)n_phr, (long long)rows_cap, (const long long*)offsets, (const int*)rank, o.list_ptr, o.docs,
                     o.status);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

// sizes every entry point refuses (nothing is enqueued)
int ph_check_sizes(const char* who, int64_t n_phr, int64_t cand_max, int64_t rows_cap) {
  AMDR_REQUIRE(n_phr >= 0 && cand_max >= 0 && rows_cap >= 0, "%s: a negative size", who);
  AMDR_REQUIRE(n_phr <= INT32_MAX, "%s: more than 2^31 - 1 phrases", who);
  AMDR_REQUIRE(ph_tiles(cand_max) <= kGridYMax, "%s: cand_max=%lld beyond %d tiles of %d candidates", who,
               (long long)cand_max, kGridYMax, kPhTile);
  return AMDR_OK;
}

PhIndex ph_index(const amdr_bm25* h) {
  const BmIndex& ix = h->ix;
  return PhIndex{ix.term_ptr, ix.post_doc, (long)ix.n_terms, (long)ix.n_docs, h->tok_ptr, h->tok};
}

}  // namespace

extern "C" {

int amdr_bm25_set_tokens(amdr_bm25_t* h, const int64_t* doc_ptr, const int32_t* tokens) {
  static const char* const who = "bm25_set_tokens";
  AMDR_REQUIRE(h != nullptr, "bm25_set_tokens: null handle");
  AMDR_REQUIRE(doc_ptr != nullptr && tokens != nullptr, "bm25_set_tokens: null array");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  const BmIndex& ix = h->ix;
  const int64_t n = ix.n_docs;
  std::unique_ptr<int32_t[]> len(new (std::nothrow) int32_t[(size_t)n + 1]);
  if (!len) return fail(AMDR_ENOMEM, "bm25_set_tokens: no host memory for %lld document lengths", (long long)n);
  if (n) AMDR_HIP(hipMemcpy(len.get(), ix.doc_len, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  const int bad = ph_validate_stream(doc_ptr, tokens, len.get(), n, ix.n_terms);
  AMDR_REQUIRE(bad == kPhValid, "bm25_set_tokens: %s", ph_error_text(bad));
  const int64_t n_tok = doc_ptr[n];
  long long* np = nullptr;
  int* nt = nullptr;
  int rc = dev_alloc(&np, (size_t)n + 1, who);
  if (!rc) rc = dev_alloc(&nt, (size_t)n_tok + 1, who);  // (+ 1: never an empty allocation)
  if (!rc && hipMemcpy(np, doc_ptr, (size_t)(n + 1) * sizeof(long long), hipMemcpyHostToDevice) != hipSuccess) rc = AMDR_EHIP;
  if (!rc && n_tok && hipMemcpy(nt, tokens, (size_t)n_tok * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) rc = AMDR_EHIP;
  if (rc) {  // the handle keeps what it had
    if (rc == AMDR_EHIP) (void)fail(AMDR_EHIP, "bm25_set_tokens: the upload failed: %s", hipGetErrorString(hipGetLastError()));
    if (np) (void)hipFree(np);
    if (nt) (void)hipFree(nt);
    return rc;
  }
  h->drop_tokens();
  h->tok_ptr = np, h->tok = nt, h->n_tokens = n_tok, h->has_tokens = true;
  return AMDR_OK;
}

int amdr_bm25_tokens_info(amdr_bm25_t* h, int64_t* out2) {
  AMDR_REQUIRE(h && out2, "bm25_tokens_info: null");
  std::lock_guard<std::mutex> g(h->mu);
  out2[0] = h->has_tokens ? 1 : 0;
  out2[1] = h->has_tokens ? h->n_tokens : 0;
  return AMDR_OK;
}

int amdr_bm25_read_tokens(amdr_bm25_t* h, int64_t* doc_ptr, int32_t* tokens) {
  AMDR_REQUIRE(h != nullptr, "bm25_read_tokens: null handle");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_REQUIRE(h->has_tokens, "bm25_read_tokens: no token stream is resident (amdr_bm25_set_tokens; an update drops it)");
  AMDR_HIP(hipSetDevice(h->device));
  if (doc_ptr) AMDR_HIP(hipMemcpy(doc_ptr, h->tok_ptr, (size_t)(h->ix.n_docs + 1) * sizeof(long long), hipMemcpyDeviceToHost));
  if (tokens && h->n_tokens) AMDR_HIP(hipMemcpy(tokens, h->tok, (size_t)h->n_tokens * sizeof(int), hipMemcpyDeviceToHost));
  return AMDR_OK;
}

int amdr_phrase_lists_plan(int64_t n_phr, int64_t cand_max, int64_t* work_bytes) {
  AMDR_REQUIRE(work_bytes != nullptr, "phrase_lists_plan: null");
  int rc = ph_check_sizes("phrase_lists_plan", n_phr, cand_max, 0);
  if (rc) return rc;
  *work_bytes = (int64_t)ph_work(n_phr, cand_max).total;
  return AMDR_OK;
}

int amdr_phrase_lists_device(amdr_bm25_t* bm25, const int64_t* phr_ptr_dev, const int32_t* phr_terms_dev, int64_t n_phr,
                             int64_t cand_max, int64_t rows_cap, int64_t* out_list_ptr_dev, int32_t* out_docs_dev,
                             int32_t* out_status_dev, void* work_dev, int64_t work_bytes, void* stream) {
  AMDR_REQUIRE(bm25 != nullptr, "phrase_lists: null handle");
  int rc = ph_check_sizes("phrase_lists", n_phr, cand_max, rows_cap);
  if (rc) return rc;
  AMDR_REQUIRE(bm25->has_tokens, "phrase_lists: no token stream is resident (amdr_bm25_set_tokens; an update drops it)");
  AMDR_REQUIRE(out_list_ptr_dev != nullptr, "phrase_lists: null out_list_ptr");
  AMDR_REQUIRE(n_phr == 0 || (phr_ptr_dev && phr_terms_dev && out_status_dev), "phrase_lists: null operand");
  AMDR_REQUIRE(rows_cap == 0 || out_docs_dev, "phrase_lists: null out_docs");
  AMDR_REQUIRE(work_bytes >= 0, "phrase_lists: work_bytes=%lld", (long long)work_bytes);
  const size_t need = n_phr ? ph_work(n_phr, cand_max).total : 0;
  AMDR_REQUIRE((size_t)work_bytes >= need && (need == 0 || work_dev), "phrase_lists: a workspace of %lld bytes, the plan asks for %zu",
               (long long)work_bytes, need);
  AMDR_HIP(hipSetDevice(bm25->device));
  const PhOut o{(long long*)out_list_ptr_dev, out_docs_dev, out_status_dev};
  return ph_launch(ph_index(bm25), (const long long*)phr_ptr_dev, phr_terms_dev, n_phr, cand_max, rows_cap, o,
                   static_cast<unsigned char*>(work_dev), (hipStream_t)stream);
}

int amdr_phrase_lists(amdr_bm25_t* bm25, const int64_t* phr_ptr, const int32_t* phr_terms, int64_t n_phr, int64_t cand_max,
                      int64_t rows_cap, int64_t* out_list_ptr, int32_t* out_docs, int32_t* out_status) {
  AMDR_REQUIRE(bm25 != nullptr, "phrase_lists: null handle");
  int rc = ph_check_sizes("phrase_lists", n_phr, cand_max, rows_cap);
  if (rc) return rc;
  AMDR_REQUIRE(out_list_ptr != nullptr, "phrase_lists: null out_list_ptr");
  AMDR_REQUIRE(n_phr == 0 || out_status, "phrase_lists: null out_status");
  AMDR_REQUIRE(rows_cap == 0 || out_docs, "phrase_lists: null out_docs");
  std::lock_guard<std::mutex> g(bm25->mu);
  AMDR_REQUIRE(bm25->has_tokens, "phrase_lists: no token stream is resident (amdr_bm25_set_tokens; an update drops it)");
  const int bad = ph_validate(phr_ptr, phr_terms, n_phr);
  AMDR_REQUIRE(bad == kPhValid, "phrase_lists: %s", ph_error_text(bad));
  if (n_phr == 0) {
    out_list_ptr[0] = 0;
    return AMDR_OK;
  }
  AMDR_HIP(hipSetDevice(bm25->device));
  // Layout of the staging buffer: phr_ptr | phr_terms | list_ptr | docs | status | the workspace, each aligned.
  const size_t n_all = (size_t)phr_ptr[n_phr];
  size_t at[6], total = 0;
  at[0] = total, total += ph_align((size_t)(n_phr + 1) * 8);
  at[1] = total, total += ph_align(n_all * 4);
  at[2] = total, total += ph_align((size_t)(n_phr + 1) * 8);
  at[3] = total, total += ph_align((size_t)rows_cap * 4);
  at[4] = total, total += ph_align((size_t)n_phr * 4);
  at[5] = total, total += ph_work(n_phr, cand_max).total;
  if ((rc = bm25->tscope.ensure(total))) return rc;
  unsigned char* p = bm25->tscope.as<unsigned char>();
  hipStream_t st = bm25->stream;
  AMDR_HIP(hipMemcpyAsync(p + at[0], phr_ptr, (size_t)(n_phr + 1) * 8, hipMemcpyHostToDevice, st));
  AMDR_HIP(hipMemcpyAsync(p + at[1], phr_terms, n_all * 4, hipMemcpyHostToDevice, st));
  const PhOut o{(long long*)(p + at[2]), (int*)(p + at[3]), (int*)(p + at[4])};
  if ((rc = ph_launch(ph_index(bm25), (const long long*)(p + at[0]), (const int*)(p + at[1]), n_phr, cand_max, rows_cap, o,
                      p + at[5], st)))
    return rc;
  AMDR_HIP(hipMemcpyAsync(out_list_ptr, o.list_ptr, (size_t)(n_phr + 1) * 8, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipMemcpyAsync(out_status, o.status, (size_t)n_phr * 4, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipStreamSynchronize(st));
  const int64_t used = out_list_ptr[n_phr];  // <= rows_cap: only the documents the lists name come back
  if (used > 0) {
    AMDR_HIP(hipMemcpyAsync(out_docs, o.docs, (size_t)used * 4, hipMemcpyDeviceToHost, st));
    AMDR_HIP(hipStreamSynchronize(st));
  }
  return AMDR_OK;
}

}  // extern "C"

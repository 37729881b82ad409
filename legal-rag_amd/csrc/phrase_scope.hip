// Phrase constraints: exact token sequences resolved into ascending document lists on the device.
//
// No reference counterpart: the reference's BM25 channel scores bags of words (legalrag/retrieval/bm25_retriever.py:74-75)
// and keeps no token order anywhere.  Here the BM25 handle holds, beside its term-major postings, the TOKEN STREAM of the
// corpus (amdr_bm25_set_tokens: the forward index, 4 B per token), and a phrase is resolved into ITS OWN ascending
// document list — a virtual posting list — which amdr_term_scope_lists (term_scope.hip) reads as one more term.  The rule
// — what a phrase is, which posting list drives it — is phrase_rule.hpp's, shared with the host check.
//
// The three launches of list_step.hpp, no atomics, deterministic; grid = (x = phrase, y = tile of kPhTile = 256
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
//
// Proximity (amdr_span_lists*: no reference counterpart either).  The same three launches take ITEMS of three kinds — a
// phrase, a Near unordered, a Near ordered (near_rule.hpp) — so that the phrases and the Nears of one batch land in one
// list array; amdr_phrase_lists* are the form in which every item is a phrase.  Driver, phase 1, the ranking, the scan and
// the write are shared unchanged, which is why a Near lives in this file; only phase 2 differs.  For a Near one wave walks
// one surviving document, 64 ANCHOR positions per round: the round's run tokens[base, base + 64 + n), clamped to the
// document — at most kNearStage = 319 ints — is staged once per wave in LDS with coalesced loads (neighbouring lanes would
// re-read almost the same tokens from memory), each lane scans at most n tokens behind its anchor from there, and a wave
// vote ends the document at the first round with a hit.  A lane whose token is no member of the Near does nothing; why
// that loses no match is near_rule.hpp's anchor argument.  The staging is traffic between the lanes of ONE wave, fenced for
// the compiler alone, so phase 2 still holds no block barrier.  LDS grows by 4 x 319 ints = 5 104 B per block.
// Worst case of a Near: one wave, len x (n + 1) steps for a document of len tokens in which every token is an anchor that
// never completes (a 4 550-token document at n = 255: 1.16 M steps, 18 200 per lane); four waves share a tile's
// survivors, so such a document delays at most the other survivors of its own tile.
#include "list_step.hpp"
#include "near_rule.hpp"

#include <mutex>

using namespace amdr;

namespace {

constexpr int kPhThreads = kPhTile;
constexpr int kPhWaves = kPhThreads / 64;
static_assert(kPhThreads % 64 == 0 && kPhLanes == 64, "whole waves; a wave is the scan's lane count");

// Workspace (list_work): a cell is a tile of an item, its payload rank-or-minus-one i32 [256]
constexpr size_t kPhCellBytes = kPhThreads * sizeof(int);
size_t ph_cells(int64_t n_phr, int64_t cand_max) { return (size_t)n_phr * (size_t)ph_tiles(cand_max); }

// The items of a call: phrases and Nears side by side.  kind == nullptr: every item is a phrase (amdr_phrase_lists).
struct SpanItems {
  const long long* ptr;  // [n + 1]
  const int* terms;      // [ptr[n]]
  const int* kind;       // [n] SpanKind, or nullptr
  const int* dist;       // [n]; read for a Near only
};

// The block's item and driver: the length, kind and distance by all, the tokens into LDS by the first L threads (an item
// the rule does not define — span_sized — reads none), the driver by thread 0; ends with a barrier.  Returns the item's
// length, 0 for an item the rule does not define.
__device__ __forceinline__ int ph_block_phrase(const PhIndex& I, const SpanItems& S, long p, int* terms, PhDriver* slot,
                                               int* kind_out, int* dist_out) {
  const long long b = S.ptr[p], L = S.ptr[p + 1] - b;
  const int kind = S.kind ? S.kind[p] : (int)kSpanPhrase;
  const int dist = kind == kSpanPhrase || !S.dist ? 0 : S.dist[p];
  const bool sized = span_sized(kind, L, dist);  // block-uniform
  if (sized && threadIdx.x < L) terms[threadIdx.x] = S.terms[b + threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) *slot = sized ? ph_driver(I, terms, L) : PhDriver{-1, -1, 0, 0};
  __syncthreads();
  *kind_out = kind, *dist_out = dist;
  return sized ? (int)L : 0;
}

__global__ __launch_bounds__(kPhThreads) void phrase_count_kernel(PhIndex I, SpanItems S, long long cand_max,
                                                                 long long* __restrict__ counts, int* __restrict__ rank_out,
                                                                 int* __restrict__ status) {
  __shared__ PhDriver drv;
  __shared__ int terms[kPhMaxLen];
  __shared__ int stage[kPhWaves][kNearStage];  // a Near's round: one staged token run per wave
  __shared__ unsigned short surv[kPhThreads];
  __shared__ unsigned char kept[kPhThreads];
  __shared__ int wsum[kPhWaves + 1];
  const long p = blockIdx.x;
  const long long tile = blockIdx.y, tiles = gridDim.y;
  const size_t cell = (size_t)p * tiles + tile;
  int kind, dist;
  const int L = ph_block_phrase(I, S, p, terms, &drv, &kind, &dist);
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
  const int n_surv = list_compact_survivors<kPhThreads>(all, surv, kept, wsum);  // (barriers: every thread is here)
  // phase 2: one wave per survivor (n_surv is block-uniform; the loop holds no barrier)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = wave; s < n_surv; s += kPhWaves) {
    const int t = surv[s];
    const long long doc = I.post_doc[D.begin + i0 + t];
    bool found = false;
    if (kind == kSpanPhrase) {  // block-uniform
      const long long last = ph_last_start(I, doc, L);
      for (long long base = I.doc_ptr[doc]; base <= last && !found; base += kPhLanes)  // wave-uniform
        found = __ballot(ph_lane_hit(I, terms, L, base, lane, last)) != 0;
    } else {
      // A Near: 64 anchors per round; the round's run [base, base + 64 + dist), clamped to the document, goes through
      // LDS once with coalesced loads and every lane scans its window from there.
      const long long end = I.doc_ptr[doc + 1];
      int* run = stage[wave];
      for (long long base = I.doc_ptr[doc]; base < end && !found; base += kPhLanes) {  // wave-uniform
        const int len = near_run_len(base, end, dist);  // <= kNearStage; base + len <= end
        for (int j = lane; j < len; j += kPhLanes) run[j] = I.tokens[base + j];
        list_wave_lds_fence();
        found = __ballot(near_lane_hit(run, len, lane, terms, L, kind == kSpanNearOrdered, dist)) != 0;
        list_wave_lds_fence();  // (the next round overwrites the run)
      }
    }
    if (lane == 0) kept[t] = found ? 1 : 0;
  }
  list_rank_and_park<kPhThreads>(kept, wsum, rank_out + cell * kPhThreads, counts + cell);  // (barriers: as above)
}

__global__ __launch_bounds__(kPhThreads) void phrase_write_kernel(PhIndex I, SpanItems S, long long cand_max,
                                                                 long long rows_cap,
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
    const int s = list_write_header(list_ptr, 0, p, offsets[(size_t)p * tiles], offsets[(size_t)(p + 1) * tiles], rows_cap);
    if (s != kTsOk) status[p] = s;  // (a phrase over cand_max has no row: its 1 stays)
  }
  int kind, dist;
  (void)ph_block_phrase(I, S, p, terms, &drv, &kind, &dist);
  const PhDriver D = drv;
  const long long i0 = tile * kPhTile;
  if (D.len > cand_max || i0 >= D.len) return;  // block-uniform
  const long long at = list_kept_at(rank_in + cell * kPhThreads, offsets, cell, 0, rows_cap);
  if (at >= 0) docs[at] = I.post_doc[D.begin + i0 + threadIdx.x];  // (a kept candidate lies inside the driver)
}

struct PhOut {
  long long* list_ptr;
  int* docs;
  int* status;
};

int ph_launch(const PhIndex& I, const SpanItems& S, int64_t n_phr, int64_t cand_max, int64_t rows_cap, const PhOut& o,
              unsigned char* work, hipStream_t st) {
  const dim3 grid((unsigned)n_phr, (unsigned)ph_tiles(cand_max));
  return list_launch(
      st, n_phr, 0, ph_cells(n_phr, cand_max), kPhCellBytes, o.list_ptr, work,
      [&](long long* counts, unsigned char* rank) {
        hipLaunchKernelGGL(phrase_count_kernel, grid, dim3(kPhThreads), 0, st, I, S, (long long)cand_max, counts, (int*)rank,
                           o.status);
      },
      [&](const long long* offsets, const unsigned char* rank) {
        hipLaunchKernelGGL(phrase_write_kernel, grid, dim3(kPhThreads), 0, st, I, S, (long long)cand_max, (long long)rows_cap,
                           offsets, (const int*)rank, o.list_ptr, o.docs, o.status);
      });
}

// sizes every entry point refuses (nothing is enqueued)
int ph_check_sizes(const char* who, int64_t n_phr, int64_t cand_max, int64_t rows_cap) {
  AMDR_REQUIRE(n_phr >= 0 && cand_max >= 0 && rows_cap >= 0, "%s: a negative size", who);
  AMDR_REQUIRE(n_phr <= INT32_MAX, "%s: more than 2^31 - 1 phrases", who);
  AMDR_REQUIRE(ph_tiles(cand_max) <= kGridYMax, "%s: cand_max=%lld beyond %d tiles of %d candidates", who,
               (long long)cand_max, kGridYMax, kPhTile);
  return AMDR_OK;
}

// The "_device" entry of phrases (S.kind == nullptr) and of mixed items: checks, then enqueues.
int span_device(const char* who, amdr_bm25_t* bm25, const SpanItems& S, int64_t n, int64_t cand_max, int64_t rows_cap,
                int64_t* out_list_ptr_dev, int32_t* out_docs_dev, int32_t* out_status_dev, void* work_dev, int64_t work_bytes,
                void* stream, bool mixed) {
  AMDR_REQUIRE(bm25 != nullptr, "%s: null handle", who);
  int rc = ph_check_sizes(who, n, cand_max, rows_cap);
  if (rc) return rc;
  if ((rc = bm_require_tokens(bm25, who))) return rc;
  AMDR_REQUIRE(out_list_ptr_dev != nullptr, "%s: null out_list_ptr", who);
  AMDR_REQUIRE(n == 0 || (S.ptr && S.terms && out_status_dev && (!mixed || (S.kind && S.dist))), "%s: null operand", who);
  AMDR_REQUIRE(rows_cap == 0 || out_docs_dev, "%s: null out_docs", who);
  const size_t need = n ? list_work(ph_cells(n, cand_max), kPhCellBytes).total : 0;
  if ((rc = list_check_work(who, work_dev, work_bytes, need))) return rc;
  AMDR_HIP(hipSetDevice(bm25->device));
  const PhOut o{(long long*)out_list_ptr_dev, out_docs_dev, out_status_dev};
  return ph_launch(ph_index(bm25), S, n, cand_max, rows_cap, o, static_cast<unsigned char*>(work_dev), (hipStream_t)stream);
}

// The host-pointer twin of both: validates, stages, resolves on the handle's stream, synchronises.  S holds host arrays.
int span_host(const char* who, amdr_bm25_t* bm25, const SpanItems& S, int64_t n, int64_t cand_max, int64_t rows_cap,
              int64_t* out_list_ptr, int32_t* out_docs, int32_t* out_status, bool mixed) {
  AMDR_REQUIRE(bm25 != nullptr, "%s: null handle", who);
  int rc = ph_check_sizes(who, n, cand_max, rows_cap);
  if (rc) return rc;
  AMDR_REQUIRE(out_list_ptr != nullptr, "%s: null out_list_ptr", who);
  AMDR_REQUIRE(n == 0 || out_status, "%s: null out_status", who);
  AMDR_REQUIRE(rows_cap == 0 || out_docs, "%s: null out_docs", who);
  std::lock_guard<std::mutex> g(bm25->mu);
  if ((rc = bm_require_tokens(bm25, who))) return rc;
  const int bad = mixed ? span_validate((const int64_t*)S.ptr, S.terms, S.kind, S.dist, n)
                        : ph_validate((const int64_t*)S.ptr, S.terms, n);
  AMDR_REQUIRE(bad == kPhValid, "%s: %s", who, mixed ? span_error_text(bad) : ph_error_text(bad));
  if (n == 0) {
    out_list_ptr[0] = 0;
    return AMDR_OK;
  }
  AMDR_HIP(hipSetDevice(bm25->device));
  // The staging buffer: the item arrays (kind and dist for mixed items only), the outputs, the workspace.
  ListStage s;
  const size_t a_ptr = s.add((size_t)(n + 1) * 8, S.ptr), a_terms = s.add((size_t)S.ptr[n] * 4, S.terms);
  const size_t a_kind = mixed ? s.add((size_t)n * 4, S.kind) : 0, a_dist = mixed ? s.add((size_t)n * 4, S.dist) : 0;
  const size_t a_list_ptr = s.add((size_t)(n + 1) * 8), a_docs = s.add((size_t)rows_cap * 4), a_status = s.add((size_t)n * 4);
  const size_t a_work = s.add(list_work(ph_cells(n, cand_max), kPhCellBytes).total);
  if ((rc = s.upload(bm25))) return rc;
  const SpanItems dev{s.at<long long>(a_ptr), s.at<int>(a_terms), mixed ? s.at<int>(a_kind) : nullptr,
                      mixed ? s.at<int>(a_dist) : nullptr};
  const PhOut o{s.at<long long>(a_list_ptr), s.at<int>(a_docs), s.at<int>(a_status)};
  hipStream_t st = bm25->stream;
  if ((rc = ph_launch(ph_index(bm25), dev, n, cand_max, rows_cap, o, s.at<unsigned char>(a_work), st))) return rc;
  // (used <= rows_cap: only the documents the lists name come back)
  return list_fetch(st, n, o.list_ptr, o.status, o.docs, 4, out_list_ptr, out_status, out_docs);
}

}  // namespace

extern "C" {

int amdr_phrase_lists_plan(int64_t n_phr, int64_t cand_max, int64_t* work_bytes) {
  AMDR_REQUIRE(work_bytes != nullptr, "phrase_lists_plan: null");
  int rc = ph_check_sizes("phrase_lists_plan", n_phr, cand_max, 0);
  if (rc) return rc;
  *work_bytes = (int64_t)list_work(ph_cells(n_phr, cand_max), kPhCellBytes).total;
  return AMDR_OK;
}


int amdr_phrase_lists_device(amdr_bm25_t* bm25, const int64_t* phr_ptr_dev, const int32_t* phr_terms_dev, int64_t n_phr,
                             int64_t cand_max, int64_t rows_cap, int64_t* out_list_ptr_dev, int32_t* out_docs_dev,
                             int32_t* out_status_dev, void* work_dev, int64_t work_bytes, void* stream) {
  const SpanItems S{(const long long*)phr_ptr_dev, phr_terms_dev, nullptr, nullptr};
  return span_device("phrase_lists", bm25, S, n_phr, cand_max, rows_cap, out_list_ptr_dev, out_docs_dev, out_status_dev,
                     work_dev, work_bytes, stream, false);
}

int amdr_phrase_lists(amdr_bm25_t* bm25, const int64_t* phr_ptr, const int32_t* phr_terms, int64_t n_phr, int64_t cand_max,
                      int64_t rows_cap, int64_t* out_list_ptr, int32_t* out_docs, int32_t* out_status) {
  const SpanItems S{(const long long*)phr_ptr, phr_terms, nullptr, nullptr};
  return span_host("phrase_lists", bm25, S, n_phr, cand_max, rows_cap, out_list_ptr, out_docs, out_status, false);
}

int amdr_span_lists_plan(int64_t n_items, int64_t cand_max, int64_t* work_bytes) {
  AMDR_REQUIRE(work_bytes != nullptr, "span_lists_plan: null");
  int rc = ph_check_sizes("span_lists_plan", n_items, cand_max, 0);
  if (rc) return rc;
  *work_bytes = (int64_t)list_work(ph_cells(n_items, cand_max), kPhCellBytes).total;
  return AMDR_OK;
}

int amdr_span_lists_device(amdr_bm25_t* bm25, const int64_t* item_ptr_dev, const int32_t* item_terms_dev,
                           const int32_t* item_kind_dev, const int32_t* item_dist_dev, int64_t n_items, int64_t cand_max,
                           int64_t rows_cap, int64_t* out_list_ptr_dev, int32_t* out_docs_dev, int32_t* out_status_dev,
                           void* work_dev, int64_t work_bytes, void* stream) {
  const SpanItems S{(const long long*)item_ptr_dev, item_terms_dev, item_kind_dev, item_dist_dev};
  return span_device("span_lists", bm25, S, n_items, cand_max, rows_cap, out_list_ptr_dev, out_docs_dev, out_status_dev,
                     work_dev, work_bytes, stream, true);
}

int amdr_span_lists(amdr_bm25_t* bm25, const int64_t* item_ptr, const int32_t* item_terms, const int32_t* item_kind,
                    const int32_t* item_dist, int64_t n_items, int64_t cand_max, int64_t rows_cap, int64_t* out_list_ptr,
                    int32_t* out_docs, int32_t* out_status) {
  const SpanItems S{(const long long*)item_ptr, item_terms, item_kind, item_dist};
  return span_host("span_lists", bm25, S, n_items, cand_max, rows_cap, out_list_ptr, out_docs, out_status, true);
}

}  // extern "C"

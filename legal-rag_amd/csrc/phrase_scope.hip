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
#include "bm25_handle.hpp"
#include "compact.hpp"
#include "near_rule.hpp"

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

// LDS traffic between the lanes of ONE wave: the LDS unit serves a wave's operations in order, so only the compiler has
// to be kept from moving them.
__device__ __forceinline__ void ph_wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
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
        ph_wave_lds_fence();
        found = __ballot(near_lane_hit(run, len, lane, terms, L, kind == kSpanNearOrdered, dist)) != 0;
        ph_wave_lds_fence();  // (the next round overwrites the run)
      }
    }
    if (lane == 0) kept[t] = found ? 1 : 0;
  }
  __syncthreads();
  const int keep = kept[threadIdx.x];
  int total;
  const int rank = compact_block_exclusive<kPhThreads, int>(keep, wsum, &total);
  rank_out[cell * kPhThreads + threadIdx.x] = keep ? rank : -1;
  if (threadIdx.x == 0) counts[cell] = total;
}

__global__ __launch_bounds__(kPhThreads) void phrase_write_kernel(PhIndex I, SpanItems S, long long cand_max,
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
  int kind, dist;
  (void)ph_block_phrase(I, S, p, terms, &drv, &kind, &dist);
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

int ph_launch(const PhIndex& I, const SpanItems& S, int64_t n_phr, int64_t cand_max, int64_t rows_cap, const PhOut& o,
              unsigned char* work, hipStream_t st) {
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
  hipLaunchKernelGGL(phrase_count_kernel, grid, dim3(kPhThreads), 0, st, I, S, (long long)cand_max, counts, rank, o.status);
  AMDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(compact_scan_i64_kernel, dim3(1), dim3(kCompactScanThreads), 0, st, (const long long*)counts,
                     (long)(n_phr * tiles), offsets);
  AMDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(phrase_write_kernel, grid, dim3(kPhThreads), 0, st, I, S, (long long)cand_max, (long)n_phr,
                     (long long)rows_cap, (const long long*)offsets, (const int*)rank, o.list_ptr, o.docs, o.status);
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

// The "_device" entry of phrases (S.kind == nullptr) and of mixed items: checks, then enqueues.
int span_device(const char* who, amdr_bm25_t* bm25, const SpanItems& S, int64_t n, int64_t cand_max, int64_t rows_cap,
                int64_t* out_list_ptr_dev, int32_t* out_docs_dev, int32_t* out_status_dev, void* work_dev, int64_t work_bytes,
                void* stream, bool mixed) {
  AMDR_REQUIRE(bm25 != nullptr, "%s: null handle", who);
  int rc = ph_check_sizes(who, n, cand_max, rows_cap);
  if (rc) return rc;
  AMDR_REQUIRE(bm25->has_tokens, "%s: no token stream is resident (amdr_bm25_set_tokens; an update drops it)", who);
  AMDR_REQUIRE(out_list_ptr_dev != nullptr, "%s: null out_list_ptr", who);
  AMDR_REQUIRE(n == 0 || (S.ptr && S.terms && out_status_dev && (!mixed || (S.kind && S.dist))), "%s: null operand", who);
  AMDR_REQUIRE(rows_cap == 0 || out_docs_dev, "%s: null out_docs", who);
  AMDR_REQUIRE(work_bytes >= 0, "%s: work_bytes=%lld", who, (long long)work_bytes);
  const size_t need = n ? ph_work(n, cand_max).total : 0;
  AMDR_REQUIRE((size_t)work_bytes >= need && (need == 0 || work_dev), "%s: a workspace of %lld bytes, the plan asks for %zu", who,
               (long long)work_bytes, need);
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
  AMDR_REQUIRE(bm25->has_tokens, "%s: no token stream is resident (amdr_bm25_set_tokens; an update drops it)", who);
  const int bad = mixed ? span_validate((const int64_t*)S.ptr, S.terms, S.kind, S.dist, n)
                        : ph_validate((const int64_t*)S.ptr, S.terms, n);
  AMDR_REQUIRE(bad == kPhValid, "%s: %s", who, mixed ? span_error_text(bad) : ph_error_text(bad));
  if (n == 0) {
    out_list_ptr[0] = 0;
    return AMDR_OK;
  }
  AMDR_HIP(hipSetDevice(bm25->device));
  // Layout of the staging buffer: item_ptr | item_terms | list_ptr | docs | status | kind | dist | the workspace, each aligned.
  const size_t n_all = (size_t)S.ptr[n];
  size_t at[8], total = 0;
  at[0] = total, total += ph_align((size_t)(n + 1) * 8);
  at[1] = total, total += ph_align(n_all * 4);
  at[2] = total, total += ph_align((size_t)(n + 1) * 8);
  at[3] = total, total += ph_align((size_t)rows_cap * 4);
  at[4] = total, total += ph_align((size_t)n * 4);
  at[5] = total, total += mixed ? ph_align((size_t)n * 4) : 0;
  at[6] = total, total += mixed ? ph_align((size_t)n * 4) : 0;
  at[7] = total, total += ph_work(n, cand_max).total;
  if ((rc = bm25->tscope.ensure(total))) return rc;
  unsigned char* p = bm25->tscope.as<unsigned char>();
  hipStream_t st = bm25->stream;
  AMDR_HIP(hipMemcpyAsync(p + at[0], S.ptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
  AMDR_HIP(hipMemcpyAsync(p + at[1], S.terms, n_all * 4, hipMemcpyHostToDevice, st));
  if (mixed) {
    AMDR_HIP(hipMemcpyAsync(p + at[5], S.kind, (size_t)n * 4, hipMemcpyHostToDevice, st));
    AMDR_HIP(hipMemcpyAsync(p + at[6], S.dist, (size_t)n * 4, hipMemcpyHostToDevice, st));
  }
  const SpanItems dev{(const long long*)(p + at[0]), (const int*)(p + at[1]), mixed ? (const int*)(p + at[5]) : nullptr,
                      mixed ? (const int*)(p + at[6]) : nullptr};
  const PhOut o{(long long*)(p + at[2]), (int*)(p + at[3]), (int*)(p + at[4])};
  if ((rc = ph_launch(ph_index(bm25), dev, n, cand_max, rows_cap, o, p + at[7], st))) return rc;
  AMDR_HIP(hipMemcpyAsync(out_list_ptr, o.list_ptr, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipMemcpyAsync(out_status, o.status, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipStreamSynchronize(st));
  const int64_t used = out_list_ptr[n];  // <= rows_cap: only the documents the lists name come back
  if (used > 0) {
    AMDR_HIP(hipMemcpyAsync(out_docs, o.docs, (size_t)used * 4, hipMemcpyDeviceToHost, st));
    AMDR_HIP(hipStreamSynchronize(st));
  }
  return AMDR_OK;
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
  *work_bytes = (int64_t)ph_work(n_items, cand_max).total;
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

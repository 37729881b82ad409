// Marks and best passages: which tokens of each HIT document the query marks, and the window of the document that holds
// the most of the query (amdr_bm25_marks) — the output side of the query language that term_scope.hip, phrase_scope.hip,
// union_lists.hip and class_span.hip resolve on the input side.
//
// No reference counterpart: the reference returns whole chunks and has neither token order nor highlighting.  Here the
// rule is marks_rule.hpp's, read from the resident token stream of the BM25 handle: work is the tokens of the HIT documents
// (k per query, not the corpus) x log2 of the query's mark table, plus kept marks x marks per window.
//
// One launch, one WAVE per (query, hit) pair, pair = blockIdx.x (a block is one wave: the grid's x holds 2^31 - 1 pairs, so a
// batch past 65 535 queries needs nothing special).  LDS only: no workspace, no global atomics, nothing allocated,
// deterministic, capturable.
//   walk    rounds of kPhLanes = 64 positions.  Each token of the round's run (at most kMkStage = 79: the 64 anchors and the
//           15 tokens a phrase may reach behind the last) is read ONCE, coalesced, and turned into its slot mask by one
//           lower-bound search (mk_token_mask), staged in LDS.  Per sequence of the query every lane tests its anchor
//           (mk_seq_hit) and an occurrence ORs its slots into the cover array in LDS (ds_or: order-free); the cover's tail
//           is carried into the next round (mk_cover_carry).  The marked positions are then compacted into the LDS mark
//           list by ballot and prefix count: position order falls out without a sort.  Marks beyond kMkMaxMarks are counted.
//   window  64 kept anchors per round: each lane scans forward through the kept marks inside its window (mk_window_scan),
//           adds the weights of the distinct slots in ascending order (mk_score) and keeps its best; the wave's arg-max on
//           (score descending, anchor ascending) is a butterfly of lane_xor exchanges (topk.hpp).
//   write   lane 0 writes the pair's window, score, masks and status; lane i < marks_cap writes mark i of the best window
//           or the fill (-1, -1).
// LDS per wave, independent of the document's length: positions i32 [1 024] (4 096 B), slots u8 [1 024] (1 024 B), the
// staged masks and the cover u32 [80] each (640 B), the weights f64 [32] (256 B): 6 016 B -> 27 waves per CU by LDS, 6
// per SIMD; the 82 VGPRs allow 5.  The traffic between the lanes of the wave needs no block barrier (list_wave_lds_fence).
#include "list_step.hpp"
#include "marks_rule.hpp"
#include "topk.hpp"

#include <mutex>
#include <vector>

using namespace amdr;

namespace {

constexpr int kMkStagePad = 80;  // kMkStage rounded to whole 16-byte lines
static_assert(kMkStagePad >= kMkStage && kPhLanes == 64 && kMkStage <= 2 * kPhLanes, "a run is staged in two steps of a wave");

struct MkQueries {
  const long long* mk_ptr;   // [nq + 1]
  const int* mk_terms;       // [mk_ptr[nq]]
  const int* mk_slot;
  const double* slot_w;      // [nq, 32]
  const unsigned* slot_loose;  // [nq]
  const long long* sq_ptr;   // [nq + 1]
  const long long* sq_off;   // [n_seq + 1]
  const int* sq_slots;
};

struct MkOut {
  int* win;         // [pairs, 4]
  double* score;    // [pairs]
  unsigned* slots;  // [pairs, 2]
  int* marks;       // [pairs, marks_cap, 2]
  int* status;      // [pairs]
};

__device__ __forceinline__ double mk_lane_xor_f64(double x, int s) {
  return __longlong_as_double((long long)lane_xor_sw((u64)__double_as_longlong(x), s));
}

__global__ __launch_bounds__(kPhLanes) void bm25_marks_kernel(const long long* __restrict__ docs, long long k, long long ld_docs,
                                                              long long n_docs, const long long* __restrict__ doc_ptr,
                                                              const int* __restrict__ tokens, MkQueries Q, int window,
                                                              int marks_cap, MkOut o) {
  __shared__ int m_pos[kMkMaxMarks];
  __shared__ unsigned char m_slot[kMkMaxMarks];
  __shared__ unsigned run[kMkStagePad];
  __shared__ unsigned cover[kMkStagePad];
  __shared__ double w[kMkSlots];
  const int lane = threadIdx.x;
  const long long pair = blockIdx.x;
  const long long q = pair / k;
  const long long doc = docs[q * ld_docs + (pair - q * k)];
  int* marks_out = o.marks + (size_t)pair * (size_t)marks_cap * 2;
  if (doc < 0 || doc >= n_docs) {  // wave-uniform: nothing of the index or the query is read
    if (lane < 4) o.win[pair * 4 + lane] = 0;
    if (lane < 2) o.slots[pair * 2 + lane] = 0u;
    if (lane == 0) o.score[pair] = 0.0, o.status[pair] = 0;
    if (lane < marks_cap) marks_out[2 * lane] = -1, marks_out[2 * lane + 1] = -1;
    return;
  }
  const long long begin = doc_ptr[doc], end = doc_ptr[doc + 1];
  const long long doc_len = end > begin ? end - begin : 0;
  long long mb = Q.mk_ptr[q], me = Q.mk_ptr[q + 1];
  if (me < mb) me = mb;
  const MkTable T{Q.mk_terms + mb, Q.mk_slot + mb, me - mb};
  const unsigned loose = Q.slot_loose[q];
  const long long s0 = Q.sq_ptr[q], s1 = Q.sq_ptr[q + 1];
  if (lane < kMkSlots) w[lane] = Q.slot_w[q * kMkSlots + lane];
  cover[lane] = 0u;
  if (lane + kPhLanes < kMkStagePad) cover[lane + kPhLanes] = 0u;
  list_wave_lds_fence();

  // ---- the walk: marks in position order ------------------------------------------------------------------------------
  int n_marks = 0;          // the true count
  unsigned kept_slots = 0;  // this lane's share of the slots among the kept marks
  for (long long base = begin; base < end; base += kPhLanes) {  // wave-uniform
    const int len = mk_run_len(base, end);  // <= kMkStage; base + len <= end
    for (int j = lane; j < len; j += kPhLanes) run[j] = mk_token_mask(tokens[base + j], T);
    list_wave_lds_fence();
    for (long long s = s0; s < s1; ++s) {  // wave-uniform
      const long long b = Q.sq_off[s], L = Q.sq_off[s + 1] - b;
      const int* sq = Q.sq_slots + b;
      if (L < 2 || L > kPhMaxLen || !mk_seq_sized(sq, L)) continue;  // (the length first: an undefined one reads no slot)
      if (mk_seq_hit(run, len, lane, sq, (int)L))
        mk_cover_occurrence(cover, lane, sq, (int)L, [](unsigned* word, unsigned bits) { atomicOr(word, bits); });
    }
    list_wave_lds_fence();
    const bool inside = lane < len;  // (len >= 64 unless the document ends in this round)
    const unsigned m = inside ? mk_mark(run[lane], loose, cover[lane]) : 0u;
    const unsigned long long vote = __ballot(m != 0u);
    if (m != 0u) {
      const int at = n_marks + __popcll(vote & ((1ull << lane) - 1ull));
      if (at < kMkMaxMarks) {
        const int s = mk_slot_of(m);
        m_pos[at] = (int)(base - begin) + lane, m_slot[at] = (unsigned char)s;
        kept_slots |= 1u << s;
      }
    }
    n_marks += __popcll(vote);
    // the next round's cover: every word is read before any is written
    const unsigned c0 = mk_cover_carry(cover, lane);
    list_wave_lds_fence();
    cover[lane] = c0;
    if (lane + kPhLanes < kMkStagePad) cover[lane + kPhLanes] = 0u;
    list_wave_lds_fence();  // (the next round overwrites the run as well)
  }
  for (int s = 1; s < kPhLanes; s <<= 1) kept_slots |= lane_xor_sw(kept_slots, s);
  const int n_kept = n_marks < kMkMaxMarks ? n_marks : kMkMaxMarks;

  // ---- the best window among the kept anchors -------------------------------------------------------------------------
  double best = 0.0;
  int best_i = -1;
  for (int a0 = 0; a0 < n_kept; a0 += kPhLanes) {  // wave-uniform
    const int i = a0 + lane;
    if (i < n_kept) {
      unsigned bits;
      int e;
      (void)mk_window_scan(m_pos, m_slot, n_kept, i, window, doc_len, &bits, &e);
      const double sc = mk_score(bits, w);
      if (mk_better(sc, i, best, best_i)) best = sc, best_i = i;
    }
  }
  for (int s = 1; s < kPhLanes; s <<= 1) {
    const double other = mk_lane_xor_f64(best, s);
    const int other_i = (int)lane_xor_sw((u32)best_i, s);
    if (mk_better(other, other_i, best, best_i)) best = other, best_i = other_i;
  }
  // every lane now holds the wave's best (the exchange is symmetric and mk_better is a strict total order on anchors)
  int w_start = 0, w_end = (int)(doc_len < window ? doc_len : window), w_count = 0;
  unsigned w_bits = 0;
  if (best_i >= 0) {
    w_start = m_pos[best_i];
    w_count = mk_window_scan(m_pos, m_slot, n_kept, best_i, window, doc_len, &w_bits, &w_end);
  }
  if (lane == 0) {
    o.win[pair * 4 + 0] = w_start, o.win[pair * 4 + 1] = w_end, o.win[pair * 4 + 2] = w_count, o.win[pair * 4 + 3] = n_marks;
    o.score[pair] = best_i >= 0 ? best : 0.0;
    o.slots[pair * 2 + 0] = w_bits, o.slots[pair * 2 + 1] = kept_slots;
    o.status[pair] = n_marks > kMkMaxMarks ? 1 : 0;
  }
  if (lane < marks_cap) {
    const bool has = lane < w_count;  // (best_i + lane < n_kept: the window's marks are kept ones)
    marks_out[2 * lane] = has ? m_pos[best_i + lane] : -1;
    marks_out[2 * lane + 1] = has ? (int)m_slot[best_i + lane] : -1;
  }
}

// sizes every entry point refuses (nothing is enqueued)
int mk_check_sizes(const char* who, int64_t nq, int64_t k, int64_t ld_docs, int32_t window, int32_t marks_cap) {
  AMDR_REQUIRE(nq >= 0 && k >= 0 && ld_docs >= 0, "%s: a negative size", who);
  AMDR_REQUIRE(ld_docs >= k, "%s: ld_docs=%lld below k=%lld", who, (long long)ld_docs, (long long)k);
  AMDR_REQUIRE(window >= 1 && window <= kMkMaxWindow, "%s: window=%d outside 1 .. %d", who, (int)window, kMkMaxWindow);
  AMDR_REQUIRE(marks_cap >= 0 && marks_cap <= kMkMaxCap, "%s: marks_cap=%d outside 0 .. %d", who, (int)marks_cap, kMkMaxCap);
  AMDR_REQUIRE(k == 0 || nq <= 0x7fffffffLL / k, "%s: %lld x %lld pairs are more than the 2^31 - 1 blocks of one launch", who,
               (long long)nq, (long long)k);
  return AMDR_OK;
}

int mk_launch(const amdr_bm25* h, const long long* docs, int64_t nq, int64_t k, int64_t ld_docs, const MkQueries& Q, int window,
              int marks_cap, const MkOut& o, hipStream_t st) {
  const long long pairs = (long long)nq * k;
  if (pairs == 0) return AMDR_OK;
  hipLaunchKernelGGL(bm25_marks_kernel, dim3((unsigned)pairs), dim3(kPhLanes), 0, st, docs, (long long)k, (long long)ld_docs,
                     (long long)h->ix.n_docs, (const long long*)h->tok_ptr, (const int*)h->tok, Q, window, marks_cap, o);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

}  // namespace

extern "C" {

int amdr_bm25_marks_device(amdr_bm25_t* bm25, const int64_t* docs_dev, int64_t nq, int64_t k, int64_t ld_docs,
                           const int64_t* mk_ptr_dev, const int32_t* mk_terms_dev, const int32_t* mk_slot_dev,
                           const double* slot_w_dev, const uint32_t* slot_loose_dev, const int64_t* sq_ptr_dev,
                           const int64_t* sq_off_dev, const int32_t* sq_slots_dev, int32_t window, int32_t marks_cap,
                           int32_t* out_win_dev, double* out_score_dev, uint32_t* out_slots_dev, int32_t* out_marks_dev,
                           int32_t* out_status_dev, void* stream) {
  static const char* const who = "bm25_marks";
  AMDR_REQUIRE(bm25 != nullptr, "%s: null handle", who);
  int rc = mk_check_sizes(who, nq, k, ld_docs, window, marks_cap);
  if (rc) return rc;
  AMDR_REQUIRE(docs_dev && mk_ptr_dev && mk_terms_dev && mk_slot_dev && slot_w_dev && slot_loose_dev && sq_ptr_dev && sq_off_dev &&
                   sq_slots_dev, "%s: null operand", who);
  AMDR_REQUIRE(out_win_dev && out_score_dev && out_slots_dev && out_status_dev && (marks_cap == 0 || out_marks_dev),
               "%s: null output", who);
  if ((rc = bm_require_tokens(bm25, who))) return rc;
  AMDR_HIP(hipSetDevice(bm25->device));
  const MkQueries Q{(const long long*)mk_ptr_dev, mk_terms_dev, mk_slot_dev, slot_w_dev, slot_loose_dev,
                    (const long long*)sq_ptr_dev, (const long long*)sq_off_dev, sq_slots_dev};
  const MkOut o{out_win_dev, out_score_dev, out_slots_dev, out_marks_dev, out_status_dev};
  return mk_launch(bm25, (const long long*)docs_dev, nq, k, ld_docs, Q, window, marks_cap, o, (hipStream_t)stream);
}

int amdr_bm25_marks(amdr_bm25_t* bm25, const int64_t* docs, int64_t nq, int64_t k, int64_t ld_docs, const int64_t* mk_ptr,
                    const int32_t* mk_terms, const int32_t* mk_slot, const double* slot_w, const uint32_t* slot_loose,
                    const int64_t* sq_ptr, const int64_t* sq_off, const int32_t* sq_slots, int32_t window, int32_t marks_cap,
                    int32_t* out_win, double* out_score, uint32_t* out_slots, int32_t* out_marks, int32_t* out_status) {
  static const char* const who = "bm25_marks";
  AMDR_REQUIRE(bm25 != nullptr, "%s: null handle", who);
  int rc = mk_check_sizes(who, nq, k, ld_docs, window, marks_cap);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(bm25->mu);
  if ((rc = bm_require_tokens(bm25, who))) return rc;
  const int bad = mk_validate(docs, nq, k, ld_docs, mk_ptr, mk_terms, mk_slot, slot_w, slot_loose, sq_ptr, sq_off, sq_slots,
                              bm25->ix.n_terms, bm25->ix.n_docs);
  AMDR_REQUIRE(bad == kPhValid, "%s: %s", who, mk_error_text(bad));
  const size_t pairs = (size_t)nq * (size_t)k;
  AMDR_REQUIRE(pairs == 0 || (out_win && out_score && out_slots && out_status && (marks_cap == 0 || out_marks)),
               "%s: null output", who);
  bm25->marks_kernel_ms = -1.0;
  if (pairs == 0) return AMDR_OK;
  AMDR_HIP(hipSetDevice(bm25->device));
  hipStream_t st = bm25->stream;
  const size_t n_mk = (size_t)mk_ptr[nq], n_seq = (size_t)sq_ptr[nq], n_sq = (size_t)sq_off[n_seq];
  // the hit ids packed [nq, k]; every array holds one element more than its count, so none is empty
  std::vector<long long> packed(pairs);
  for (int64_t q = 0; q < nq; ++q)
    for (int64_t j = 0; j < k; ++j) packed[(size_t)(q * k + j)] = docs[q * ld_docs + j];
  CallScratch tmp;
  long long *d_docs, *d_mk_ptr, *d_sq_ptr, *d_sq_off;
  int *d_terms, *d_slot, *d_sq, *d_win, *d_marks, *d_status;
  double *d_w, *d_score;
  unsigned *d_loose, *d_slots;
  AMDR_TRY(tmp.alloc(&d_docs, pairs + 1, who));
  AMDR_TRY(tmp.alloc(&d_mk_ptr, (size_t)nq + 1, who));
  AMDR_TRY(tmp.alloc(&d_terms, n_mk + 1, who));
  AMDR_TRY(tmp.alloc(&d_slot, n_mk + 1, who));
  AMDR_TRY(tmp.alloc(&d_w, (size_t)nq * kMkSlots + 1, who));
  AMDR_TRY(tmp.alloc(&d_loose, (size_t)nq + 1, who));
  AMDR_TRY(tmp.alloc(&d_sq_ptr, (size_t)nq + 1, who));
  AMDR_TRY(tmp.alloc(&d_sq_off, n_seq + 1, who));
  AMDR_TRY(tmp.alloc(&d_sq, n_sq + 1, who));
  AMDR_TRY(tmp.alloc(&d_win, pairs * 4, who));
  AMDR_TRY(tmp.alloc(&d_score, pairs, who));
  AMDR_TRY(tmp.alloc(&d_slots, pairs * 2, who));
  AMDR_TRY(tmp.alloc(&d_marks, pairs * (size_t)marks_cap * 2 + 1, who));
  AMDR_TRY(tmp.alloc(&d_status, pairs, who));
  auto up = [&](void* dst, const void* src, size_t bytes) -> int {
    if (bytes) AMDR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
    return AMDR_OK;
  };
  AMDR_TRY(up(d_docs, packed.data(), pairs * 8));
  AMDR_TRY(up(d_mk_ptr, mk_ptr, ((size_t)nq + 1) * 8));
  AMDR_TRY(up(d_terms, mk_terms, n_mk * 4));
  AMDR_TRY(up(d_slot, mk_slot, n_mk * 4));
  AMDR_TRY(up(d_w, slot_w, (size_t)nq * kMkSlots * 8));
  AMDR_TRY(up(d_loose, slot_loose, (size_t)nq * 4));
  AMDR_TRY(up(d_sq_ptr, sq_ptr, ((size_t)nq + 1) * 8));
  AMDR_TRY(up(d_sq_off, sq_off, (n_seq + 1) * 8));
  AMDR_TRY(up(d_sq, sq_slots, n_sq * 4));
  const MkQueries Q{d_mk_ptr, d_terms, d_slot, d_w, d_loose, d_sq_ptr, d_sq_off, d_sq};
  const MkOut o{d_win, d_score, d_slots, d_marks, d_status};
  KernelSpans timer(1);  // the one kernel (amdr_bm25_marks_kernel_ms)
  AMDR_TRY(timer.begin(0, st));
  AMDR_TRY(mk_launch(bm25, d_docs, nq, k, k, Q, window, marks_cap, o, st));
  AMDR_TRY(timer.end(0, st));
  AMDR_HIP(hipMemcpyAsync(out_win, d_win, pairs * 4 * 4, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipMemcpyAsync(out_score, d_score, pairs * 8, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipMemcpyAsync(out_slots, d_slots, pairs * 2 * 4, hipMemcpyDeviceToHost, st));
  if (marks_cap > 0) AMDR_HIP(hipMemcpyAsync(out_marks, d_marks, pairs * (size_t)marks_cap * 2 * 4, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipMemcpyAsync(out_status, d_status, pairs * 4, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipStreamSynchronize(st));
  bm25->marks_kernel_ms = timer.ms();
  return AMDR_OK;
}

int amdr_bm25_marks_kernel_ms(amdr_bm25_t* h, double* ms) {
  AMDR_REQUIRE(h && ms, "bm25_marks_kernel_ms: null");
  std::lock_guard<std::mutex> g(h->mu);
  *ms = h->marks_kernel_ms;
  return AMDR_OK;
}

}  // extern "C"

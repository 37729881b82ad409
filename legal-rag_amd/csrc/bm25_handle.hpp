// The BM25 handle, shared by bm25.hip (create, plan, score, search, destroy), bm25_update.hip (add, remove, info, read, the
// token stream) and the list resolvers of list_step.hpp: term_scope.hip (term constraints), phrase_scope.hip (phrases,
// Nears), union_lists.hip (unions of posting lists), class_span.hip (class spans) and unit_span.hip (unit spans and the break
// flags), and marks.hip (marks and best passages of the hit documents).  The per-call plumbing of the updates
// (dev_alloc, CallScratch, KernelSpans, AMDR_TRY) is call_scratch.hpp's, shared with the other two channels.
#pragma once
#include "call_scratch.hpp"
#include "common.hpp"

#include <mutex>
#include <utility>

namespace amdr {

// The resident index: term-major CSR postings, the per-posting factors, idf and the document lengths.  Every array
// carries ONE padding element behind its `count` values — the scoring kernel's clamped prefetch may touch [count] — and
// alloc() is the only place that knows it: amdr_bm25_create's upload and the updates allocate through it.
struct BmIndex {
  long long* term_ptr = nullptr;  // [n_terms + 1]
  int* post_doc = nullptr;        // [nnz]
  int* post_tf = nullptr;         // [nnz] resident for the updates: the factors are recomputed from (tf, doc_len, avgdl)
  double* post_w = nullptr;       // [nnz] tf*(k1+1) / (tf + k1*(1 - b + b*len/avgdl)) per posting, fp64
  double* idf = nullptr;          // [n_terms]
  int* doc_len = nullptr;         // [n_docs]
  int64_t n_terms = 0, n_docs = 0, nnz = 0;
  double avgdl = 0;

  template <class T>
  static int alloc(T** dst, size_t count, const char* who) {
    return dev_alloc(dst, count + 1, who);
  }
  // the tables of n_terms terms and n_docs documents; the postings, once their number is known
  int alloc_tables(int64_t V, int64_t n, double avg, const char* who) {
    n_terms = V, n_docs = n, avgdl = avg;
    int rc = alloc(&term_ptr, (size_t)V + 1, who);
    if (!rc) rc = alloc(&idf, (size_t)V, who);
    if (!rc) rc = alloc(&doc_len, (size_t)n, who);
    return rc;
  }
  int alloc_postings(int64_t count, const char* who) {
    nnz = count;
    int rc = alloc(&post_doc, (size_t)count, who);
    if (!rc) rc = alloc(&post_tf, (size_t)count, who);
    if (!rc) rc = alloc(&post_w, (size_t)count, who);
    return rc;
  }
  void free() {
    for (void* q : {(void*)term_ptr, (void*)post_doc, (void*)post_tf, (void*)post_w, (void*)idf, (void*)doc_len})
      if (q) (void)hipFree(q);
    *this = BmIndex();
  }
};

// An index in the making, beside the live one (amdr_bm25_add, amdr_bm25_remove).  commit() is the whole update: the two
// values change places, so this one's destructor frees the OLD arrays after a commit and the half-built ones after a
// failure — a failed update leaves the handle as it was.
struct BmStagedIndex : BmIndex {
  BmStagedIndex() = default;
  BmStagedIndex(const BmStagedIndex&) = delete;
  BmStagedIndex& operator=(const BmStagedIndex&) = delete;
  ~BmStagedIndex() { free(); }
  void commit(BmIndex& live, int64_t& updates) {
    std::swap(live, static_cast<BmIndex&>(*this));
    ++updates;
  }
};

}  // namespace amdr

struct amdr_bm25 {
  int device = 0;
  amdr::BmIndex ix;
  int64_t adds = 0, removes = 0, replaces = 0;
  double k1 = 1.5, b = 0.75;
  double add_kernel_ms = -1;     // event time of the last add's merge kernel (amdr_bm25_add_kernel_ms)
  double remove_kernel_ms = -1;  // summed event time of the last remove's passes (amdr_bm25_remove_kernel_ms)
  double replace_kernel_ms = -1;  // summed event time of the last replace's passes (amdr_bm25_replace_kernel_ms)
  double carry_kernel_ms = -1;    // summed event time of the last carrying update's carry passes (amdr_bm25_carry_kernel_ms)
  double marks_kernel_ms = -1;    // event time of the kernel of the last amdr_bm25_marks (amdr_bm25_marks_kernel_ms)
  hipStream_t stream = nullptr;
  std::mutex mu;
  // part[0]: "_device" calls, part[1]: host-pointer calls (see dense.hip)
  amdr::DevBuf part[2], qterms, qptr, sbuf, ibuf, full;
  amdr::DevBuf tscope;  // the host twins of the list resolvers (ListStage, list_step.hpp): staged operands, outputs, workspace
  amdr::DevBuf ticket;  // 64 zeroed ints: arrival counters of the one-launch serving step (dense_tail.hip), self-resetting
  // The token stream (amdr_bm25_set_tokens, bm25_update.hip): document d's text as the term ids
  // tok[tok_ptr[d] .. tok_ptr[d + 1]).  It describes ONE state of the index: every successful plain update drops it, a
  // carrying one (amdr_bm25_*_carry, bm25_update.hip) commits a new stream together with the new index.
  long long* tok_ptr = nullptr;  // [n_docs + 1]
  int* tok = nullptr;            // [n_tokens]
  int64_t n_tokens = 0;
  bool has_tokens = false;
  // The break flags (amdr_bm25_set_breaks, unit_span.hip): one byte per token of the stream, bit 0 a sentence start, bit 1 a
  // paragraph start.  They describe ONE state of the stream: whatever drops or replaces the stream drops them.
  unsigned char* brk = nullptr;  // [n_tokens]
  bool has_breaks = false;
  void drop_breaks() {
    if (brk) (void)hipFree(brk);
    brk = nullptr, has_breaks = false;
  }
  void drop_tokens() {
    if (tok_ptr) (void)hipFree(tok_ptr);
    if (tok) (void)hipFree(tok);
    tok_ptr = nullptr, tok = nullptr, n_tokens = 0, has_tokens = false;
    drop_breaks();
  }
};

namespace amdr {

// What every call that reads the token stream asks of the handle (under h->mu where the call takes it).
inline int bm_require_tokens(const amdr_bm25* h, const char* who) {
  AMDR_REQUIRE(h->has_tokens, "%s: no token stream is resident (amdr_bm25_set_tokens; an update drops it)", who);
  return AMDR_OK;
}

// A token stream in the making, beside the live one (the carrying updates): BmStagedIndex's contract.  commit() changes the
// two streams' places, so the destructor frees the OLD arrays after a commit and the half-built ones after a failure.
struct BmStagedTokens {
  long long* tok_ptr = nullptr;  // [n_docs + 1]
  int* tok = nullptr;            // [n_tokens]
  int64_t n_tokens = 0;
  BmStagedTokens() = default;
  BmStagedTokens(const BmStagedTokens&) = delete;
  BmStagedTokens& operator=(const BmStagedTokens&) = delete;
  ~BmStagedTokens() {
    if (tok_ptr) (void)hipFree(tok_ptr);
    if (tok) (void)hipFree(tok);
  }
  void commit(amdr_bm25& h) {
    std::swap(h.tok_ptr, tok_ptr);
    std::swap(h.tok, tok);
    std::swap(h.n_tokens, n_tokens);
    h.has_tokens = true;
    h.drop_breaks();  // (they described the stream as it was; the carry kernels do not carry them)
  }
};

}  // namespace amdr

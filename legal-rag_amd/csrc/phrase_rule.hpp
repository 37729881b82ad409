// The rules of amdr_phrase_lists (phrase_scope.hip) that are plain C++: what a phrase is, when a document holds it, which
// posting list drives it, and the host validation of the operands and of a token stream.  The kernels, the host twin and
// the host check (check_phrase_scope.cpp, which applies the same functions tile by tile and lane by lane on the CPU) share
// this one source, in the style of term_scope_rule.hpp.
//
// The token stream (the forward index).  Document d's text, as the index tokeniser cut it, is the term ids
// tokens[doc_ptr[d] .. doc_ptr[d + 1]): doc_ptr[d + 1] - doc_ptr[d] == doc_len[d], every id in [0, n_terms).
//
// The rule.  A phrase is a list of L term ids, 2 <= L <= kPhMaxLen.  A document d HOLDS it when tokens[p + j] ==
// phrase[j] for all j in [0, L), for some p with doc_ptr[d] <= p <= doc_ptr[d + 1] - L: a match never reaches into the
// next document; overlapping occurrences and repeated tokens are plain cases of this.  An id outside [0, n_terms)
// anywhere in the phrase gives an empty list without reading anything, and so does a length outside 2 .. kPhMaxLen
// (the host twin refuses that one; the "_device" call takes its operands as they are).
//
// The driver of a phrase is the shortest posting list among its tokens, ties -> the first in phrase order: every
// document that holds the phrase holds every token, so the answer is a subset of each list, and the output is ascending
// without a sort because a posting list is.  Work: |driver| x the sum of log2(df) over the other tokens, plus the token
// runs of the documents that hold all of them — not the corpus.
#pragma once
#include "term_scope_rule.hpp"

namespace amdr {

constexpr int kPhMaxLen = 16;  // tokens of a phrase
constexpr int kPhTile = 256;   // candidates per block: one per thread
constexpr int kPhLanes = 64;   // start positions tested side by side in one document (a wave)

// The resident postings and the token stream.
struct PhIndex {
  const long long* term_ptr;
  const int* post_doc;
  long n_terms, n_docs;
  const long long* doc_ptr;  // [n_docs + 1]
  const int* tokens;         // [doc_ptr[n_docs]]
};

struct PhDriver {
  int at;           // the driver's position in the phrase; -1: the list is empty
  int term;         // its term id
  long long begin;  // first candidate: an index into post_doc
  long long len;    // the candidate count
};

// The driver of the phrase terms[0 .. L).  Reads term_ptr of the phrase's tokens only.
AMDR_TS_HD inline PhDriver ph_driver(const PhIndex& I, const int* terms, long long L) {
  PhDriver d{-1, -1, 0, 0};
  if (L < 2 || L > kPhMaxLen) return d;
  for (int j = 0; j < (int)L; ++j)
    if (terms[j] < 0 || terms[j] >= I.n_terms) return d;
  for (int j = 0; j < (int)L; ++j) {
    const int t = terms[j];
    const long long p0 = I.term_ptr[t], len = I.term_ptr[t + 1] - p0;
    if (d.at < 0 || len < d.len) d = PhDriver{j, t, p0, len};
  }
  if (d.len < 0) d.len = 0;
  return d;
}

// Whether `doc`, a candidate of driver D, has a posting for every other token of the phrase.
AMDR_TS_HD inline bool ph_has_all(const PhIndex& I, const int* terms, int L, const PhDriver& D, long long doc) {
  for (int j = 0; j < L; ++j) {
    if (j == D.at || terms[j] == D.term) continue;
    if (!posting_has(I.term_ptr, I.post_doc, I.n_terms, terms[j], doc)) return false;
  }
  return true;
}

// Whether the phrase stands at position p of the stream.  The caller keeps p + L inside the document.
AMDR_TS_HD inline bool ph_match_at(const int* tokens, long long p, const int* terms, int L) {
  for (int j = 0; j < L; ++j)
    if (tokens[p + j] != terms[j]) return false;
  return true;
}

// The last start position of a phrase of L tokens inside document `doc` (below doc_ptr[doc]: the document is shorter).
AMDR_TS_HD inline long long ph_last_start(const PhIndex& I, long long doc, int L) { return I.doc_ptr[doc + 1] - L; }

// One lane's share of one round of the scan of `doc`: the start position base + lane, if it lies inside the document.
AMDR_TS_HD inline bool ph_lane_hit(const PhIndex& I, const int* terms, int L, long long base, int lane, long long last) {
  const long long p = base + lane;
  return p <= last && ph_match_at(I.tokens, p, terms, L);
}

// Tiles of kPhTile candidates that cover a driver of up to cand_max candidates (at least one, as ts_tiles).
AMDR_TS_HD inline long long ph_tiles(long long cand_max) {
  const long long t = (cand_max + kPhTile - 1) / kPhTile;
  return t < 1 ? 1 : t;
}

// ---- host validation ------------------------------------------------------------------------------------------------------
enum PhError {
  kPhValid = 0,
  kPhNull,     // a null array that the sizes say is read
  kPhSizes,    // a negative count
  kPhPtr,      // phr_ptr does not start at 0 or is not monotone
  kPhLength,   // a phrase shorter than 2 or longer than kPhMaxLen tokens
  kPhDocPtr,   // doc_ptr does not start at 0 or is not monotone
  kPhToken,    // a token outside [0, n_terms)
  kPhDocLen,   // a document's run is not doc_len[d] tokens long
};

inline const char* ph_error_text(int e) {
  switch (e) {
    case kPhNull: return "a null operand array";
    case kPhSizes: return "a negative count";
    case kPhPtr: return "phr_ptr does not run monotonically from 0";
    case kPhLength: return "a phrase of fewer than 2 or more than 16 tokens";
    case kPhDocPtr: return "doc_ptr does not run monotonically from 0";
    case kPhToken: return "a token outside [0, n_terms)";
    case kPhDocLen: return "a document's token run differs from its doc_len (a stream made for another state of the index)";
    default: return "ok";
  }
}

// The phrases of a call (amdr_phrase_lists; the "_device" call takes them as they are).
inline int ph_validate(const int64_t* phr_ptr, const int32_t* phr_terms, int64_t n_phr) {
  if (n_phr < 0) return kPhSizes;
  if (!phr_ptr) return kPhNull;
  if (phr_ptr[0] != 0) return kPhPtr;
  for (int64_t p = 0; p < n_phr; ++p) {
    if (phr_ptr[p + 1] < phr_ptr[p]) return kPhPtr;
    const int64_t L = phr_ptr[p + 1] - phr_ptr[p];
    if (L < 2 || L > kPhMaxLen) return kPhLength;
  }
  if (n_phr > 0 && !phr_terms) return kPhNull;
  return kPhValid;
}

// A token stream against the index it is set on (amdr_bm25_set_tokens).
inline int ph_validate_stream(const int64_t* doc_ptr, const int32_t* tokens, const int32_t* doc_len, int64_t n_docs,
                              int64_t n_terms) {
  if (n_docs < 0 || n_terms < 0) return kPhSizes;
  if (!doc_ptr || !tokens || (n_docs > 0 && !doc_len)) return kPhNull;
  if (doc_ptr[0] != 0) return kPhDocPtr;
  for (int64_t d = 0; d < n_docs; ++d)
    if (doc_ptr[d + 1] < doc_ptr[d]) return kPhDocPtr;
  for (int64_t d = 0; d < n_docs; ++d)
    if (doc_ptr[d + 1] - doc_ptr[d] != (int64_t)doc_len[d]) return kPhDocLen;
  for (int64_t i = 0; i < doc_ptr[n_docs]; ++i)
    if (tokens[i] < 0 || tokens[i] >= n_terms) return kPhToken;
  return kPhValid;
}

}  // namespace amdr

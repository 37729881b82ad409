// The rules of amdr_bm25_marks (marks.hip) that are plain C++: which tokens of a hit document a query MARKS, which window
// of the document is its best passage, and the host validation of the operands.  The kernel, the host twin and the host
// check (check_marks.cpp, which applies the same functions round by round and lane by lane on the CPU) share this one
// source, in the style of near_rule.hpp and class_span_rule.hpp, whose lane count, phrase length and run length are reused.
//
// Operands of query q.
//   mark table  mk_terms[mk_ptr[q] .. mk_ptr[q + 1]) strictly ascending, distinct term ids, mk_slot parallel to it: the SLOT
//               0 .. kMkSlots - 1 the token fills.  A slot is one query word — a plain token, or a class (the vocabulary
//               tokens of a Prefix, the members of a OneOf).  One lower-bound search per token (mk_token_mask); a token
//               that is not in the table, or whose slot lies outside 0 .. 31, fills nothing.
//   slot_w      f64 [32]: the slots' weights.
//   loose       u32: a loose slot marks its token wherever it stands.
//   sequences   sq_ptr[q] .. sq_ptr[q + 1] index sq_off, sq_off[s] .. sq_off[s + 1] index sq_slots: L slots, 2 <= L <=
//               kPhMaxLen.  Sequence s OCCURS at position p of a document when token p + j fills slot sq[j] for every j and
//               p + L stays inside the document.  A length outside 2 .. 16 or a slot outside 0 .. 31 never occurs.
// Mark of position p of a document:  m(p) = (mask of token p & loose) | cover(p),  cover(p) = the OR of bit sq[j] over every
// occurrence of a sequence at p - j.  p is MARKED when m(p) != 0, and its slot is the lowest set bit of m(p): a slot that is
// only a phrase member marks a token only inside an occurrence of the phrase.
// Best window, W = window: the candidates are [a, a + W) for every marked a, clamped to the document; a window's score is
// the sum of slot_w[s] over the DISTINCT slots of its marks, added in ascending s from 0.0 in fp64 (mk_score); the greatest
// score wins, ties -> the smallest a (mk_better).  A document without marks: [0, min(W, len)), score 0.0, masks 0.
// Mark cap: the marks are kept in position order up to kMkMaxMarks; later ones are counted only, the best window is the
// best among the kept anchors over the kept marks, and the pair's status is 1.
//
// The staged run.  One round tests the kPhLanes anchors base .. base + 63 and needs the masks of tokens[base .. base + 64 +
// kPhMaxLen - 1), clamped to the document: at most kMkStage = 79 words.  An occurrence at an anchor of this round may cover
// up to 15 positions of the NEXT round: the cover array has kMkStage words too and its tail becomes the next round's head
// (mk_cover_carry).  Position base + i, i < 64, is final once the round's anchors are tested, since an occurrence that
// covers it starts at base + i - 15 at the earliest: in this round or, through the carried tail, the one before.
#pragma once
#include "near_rule.hpp"

namespace amdr {

constexpr int kMkSlots = 32;        // slots of a query
constexpr int kMkMaxMarks = 1024;   // marks kept per document
constexpr int kMkMaxWindow = 4096;  // the largest window, in tokens
constexpr int kMkMaxCap = 64;       // marks written per pair, at most (one per lane)
constexpr int kMkStage = kPhLanes + kPhMaxLen - 1;  // words of one round's staged run and of its cover, at most
static_assert(kMkMaxCap <= kPhLanes, "the marks of a window are written one per lane");

// The mark table of one query: terms[0 .. n) strictly ascending, slot parallel.
struct MkTable {
  const int* terms;
  const int* slot;
  long long n;
};

// The mask of the slots token x fills: one bit, or 0.
AMDR_TS_HD inline unsigned mk_token_mask(int x, const MkTable& T) {
  long long lo = 0, hi = T.n;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (T.terms[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo >= T.n || T.terms[lo] != x) return 0u;
  const int s = T.slot[lo];
  return s >= 0 && s < kMkSlots ? 1u << s : 0u;
}

// The masks of the round that starts at stream position `base` of a document that ends at `end` (base < end).
AMDR_TS_HD inline int mk_run_len(long long base, long long end) { return near_run_len(base, end, kPhMaxLen - 1); }

// Whether sq[0 .. L) is a sequence the rule defines.
AMDR_TS_HD inline bool mk_seq_sized(const int* sq, long long L) {
  if (L < 2 || L > kPhMaxLen) return false;
  for (int j = 0; j < (int)L; ++j)
    if (sq[j] < 0 || sq[j] >= kMkSlots) return false;
  return true;
}

// One lane's share of one sequence in one round: whether the (sized) sequence occurs at the anchor run[lane] of the staged
// masks run[0 .. len).  lane + L <= len keeps the occurrence inside the document, because the run is clamped to it and an
// unclamped run holds 64 + 15 masks.
AMDR_TS_HD inline bool mk_seq_hit(const unsigned* run, int len, int lane, const int* sq, int L) {
  if (lane + L > len) return false;
  for (int j = 0; j < L; ++j)
    if (!((run[lane + j] >> sq[j]) & 1u)) return false;
  return true;
}

// An occurrence at anchor `lane` ORs bit sq[j] into cover[lane + j]: lane + L <= 64 + 15 = kMkStage.  `or_into(word, bits)`
// is the caller's OR — an LDS atomic on the device, where the lanes of a wave land on the same words, a plain one on the
// host; an OR is order-free either way.
template <class OrInto>
AMDR_TS_HD inline void mk_cover_occurrence(unsigned* cover, int lane, const int* sq, int L, OrInto&& or_into) {
  for (int j = 0; j < L; ++j) or_into(&cover[lane + j], 1u << sq[j]);
}

// The cover word i (0 .. kMkStage) of the NEXT round, from this round's: the tail moves to the head, the rest is clear.
AMDR_TS_HD inline unsigned mk_cover_carry(const unsigned* cover, int i) {
  return i + kPhLanes < kMkStage ? cover[i + kPhLanes] : 0u;
}

// m(p) of a position, from its token's mask and its cover word; 0: unmarked.
AMDR_TS_HD inline unsigned mk_mark(unsigned token_mask, unsigned loose, unsigned cover) { return (token_mask & loose) | cover; }

// The slot of a marked position: the lowest set bit of m != 0.
AMDR_TS_HD inline int mk_slot_of(unsigned m) {
  int s = 0;
  while (!((m >> s) & 1u)) ++s;
  return s;
}

// The window of kept anchor i over the kept marks pos[0 .. n_kept) (ascending, relative to the document), slot[] parallel:
// [pos[i], *end), *end = min(pos[i] + W, doc_len); *bits: the slots of its marks; returns their number (>= 1).
AMDR_TS_HD inline int mk_window_scan(const int* pos, const unsigned char* slot, int n_kept, int i, int W, long long doc_len,
                                     unsigned* bits, int* end) {
  const long long e = (long long)pos[i] + W < doc_len ? (long long)pos[i] + W : doc_len;
  unsigned b = 0;
  int t = i;
  while (t < n_kept && pos[t] < e) b |= 1u << slot[t], ++t;
  *bits = b, *end = (int)e;
  return t - i;
}

// A window's score: the weights of its slots, added in ascending slot order from 0.0.  (Built without contraction: the
// Python restatement adds the same doubles in the same order.)
AMDR_TS_HD inline double mk_score(unsigned bits, const double* w) {
  double s = 0.0;
  for (int k = 0; k < kMkSlots; ++k)
    if ((bits >> k) & 1u) s += w[k];
  return s;
}

// Whether window (score a, kept anchor ia) beats (score b, kept anchor ib); ib < 0: there is no b yet.
AMDR_TS_HD inline bool mk_better(double a, int ia, double b, int ib) {
  if (ib < 0) return ia >= 0;
  if (ia < 0) return false;
  return a > b || (a == b && ia < ib);
}

// ---- host validation ------------------------------------------------------------------------------------------------------
enum MkError {  // behind CsError's
  kMkPtr = 300,  // mk_ptr, sq_ptr or sq_off does not start at 0 or is not monotone
  kMkTermOrder,  // the terms of a query's mark table are not strictly ascending
  kMkTerm,       // a term outside [0, n_terms)
  kMkSlot,       // a slot outside 0 .. 31
  kMkSeqLength,  // a sequence shorter than 2 or longer than kPhMaxLen slots
  kMkWeight,     // a weight that is not finite
  kMkDoc,        // a hit id outside [-1, n_docs)
};

inline const char* mk_error_text(int e) {
  switch (e) {
    case kMkPtr: return "mk_ptr, sq_ptr or sq_off does not run monotonically from 0";
    case kMkTermOrder: return "the terms of a mark table are not strictly ascending";
    case kMkTerm: return "a term outside [0, n_terms)";
    case kMkSlot: return "a slot outside 0 .. 31";
    case kMkSeqLength: return "a sequence of fewer than 2 or more than 16 slots";
    case kMkWeight: return "a slot weight that is not finite";
    case kMkDoc: return "a hit id outside [-1, n_docs)";
    default: return ph_error_text(e);
  }
}

inline bool mk_monotone(const int64_t* p, int64_t n) {
  if (p[0] != 0) return false;
  for (int64_t i = 0; i < n; ++i)
    if (p[i + 1] < p[i]) return false;
  return true;
}

// The operands of a call (amdr_bm25_marks; the "_device" call takes them as they are).
inline int mk_validate(const int64_t* docs, int64_t nq, int64_t k, int64_t ld_docs, const int64_t* mk_ptr, const int32_t* mk_terms,
                       const int32_t* mk_slot, const double* slot_w, const uint32_t* slot_loose, const int64_t* sq_ptr,
                       const int64_t* sq_off, const int32_t* sq_slots, int64_t n_terms, int64_t n_docs) {
  if (nq < 0 || k < 0 || ld_docs < k || n_terms < 0 || n_docs < 0) return kPhSizes;
  if (!mk_ptr || !sq_ptr || !sq_off) return kPhNull;
  if (nq > 0 && (!slot_w || !slot_loose)) return kPhNull;
  if (nq > 0 && k > 0 && !docs) return kPhNull;
  if (!mk_monotone(mk_ptr, nq) || !mk_monotone(sq_ptr, nq)) return kMkPtr;
  const int64_t n_seq = sq_ptr[nq];
  if (!mk_monotone(sq_off, n_seq)) return kMkPtr;
  if (mk_ptr[nq] > 0 && (!mk_terms || !mk_slot)) return kPhNull;
  if (sq_off[n_seq] > 0 && !sq_slots) return kPhNull;
  for (int64_t q = 0; q < nq; ++q)
    for (int64_t i = mk_ptr[q]; i < mk_ptr[q + 1]; ++i) {
      if (mk_terms[i] < 0 || mk_terms[i] >= n_terms) return kMkTerm;
      if (i > mk_ptr[q] && mk_terms[i] <= mk_terms[i - 1]) return kMkTermOrder;
      if (mk_slot[i] < 0 || mk_slot[i] >= kMkSlots) return kMkSlot;
    }
  for (int64_t s = 0; s < n_seq; ++s) {
    const int64_t L = sq_off[s + 1] - sq_off[s];
    if (L < 2 || L > kPhMaxLen) return kMkSeqLength;
    for (int64_t j = sq_off[s]; j < sq_off[s + 1]; ++j)
      if (sq_slots[j] < 0 || sq_slots[j] >= kMkSlots) return kMkSlot;
  }
  for (int64_t i = 0; i < nq * kMkSlots; ++i)
    if (!(slot_w[i] - slot_w[i] == 0.0)) return kMkWeight;  // (an infinity or a NaN)
  for (int64_t q = 0; q < nq; ++q)
    for (int64_t j = 0; j < k; ++j)
      if (docs[q * ld_docs + j] < -1 || docs[q * ld_docs + j] >= n_docs) return kMkDoc;
  return kPhValid;
}

}  // namespace amdr

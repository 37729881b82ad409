// The rules of amdr_class_spans (class_span.hip) that are plain C++: what a class span is, which bits a token sets in the
// mask of an item's slots, what one lane of the scan does with the staged MASKS of a round, which list drives an item,
// and the host validation of the operands.  The kernels, the host twin and the host check (check_class_span.cpp, which
// applies the same functions tile by tile, round by round and lane by lane on the CPU) share this one source, in the
// style of phrase_rule.hpp and near_rule.hpp, whose constants and span_sized a class span reuses unchanged.
//
// The rule.  A class span is a phrase or a Near whose SLOTS name token classes instead of tokens: sell! /5 good!,
// "secur! interest", (buyer purchaser) +3 accept!.  An item is L slot ids, a kind (SpanKind) and a distance n, sized as
// span_sized says.  A slot id s is
//   0 <= s < n_terms                                        a plain token: token x FILLS the slot when x == s;
//   n_terms + cls_first <= s < n_terms + cls_first + n_cls  class c = s - n_terms - cls_first: x fills the slot when x is
//                                                           one of cls_terms[cls_ptr[c] .. cls_ptr[c + 1]), strictly
//                                                           ascending — the union step's item_ptr / item_terms — and the
//                                                           documents that hold a member are list cls_first + c of the
//                                                           call's list array (what the union step wrote there);
//   anything else                                           unknown: the item's list is empty, nothing is dereferenced.
// Within one document d, tokens[doc_ptr[d] .. doc_ptr[d + 1]):
//   phrase     some position p has token p + j filling slot j for every j; p + L stays inside d.
//   ordered    positions p0 < p1 < ... inside d, token p_i fills slot i, p[L-1] - p0 <= n.
//   unordered  some run of at most n + 1 consecutive tokens of d admits an assignment of the slots to DISTINCT positions
//              of the run, each token filling its slot: a bipartite matching.
// Masks.  A token is turned ONCE into the bit mask of the slots it fills (cs_token_mask: an equality test for a plain
// slot, a lower-bound search in the member ids for a class slot) and the scan reads masks only.  A phrase tests bit j of
// mask p + j.  The ordered form takes the earliest next match of each slot from every anchor that has bit 0 — near_rule's
// argument, which holds for any per-slot predicate.  The unordered form keeps near_rule's tally: a token fills the FIRST
// unfilled slot it may fill.  That tally equals the matching exactly when the slots' id sets are PAIRWISE EQUAL OR
// DISJOINT: the slots then fall into groups of equal sets, a token belongs to one group at most, and a group of k slots is
// filled by the first k of its tokens.  With slots {a, b}, {a} on the tokens a b it fails — a fills the first slot, b the
// second never — though the matching b -> slot 0, a -> slot 1 exists: cs_validate refuses such an item and the packer
// raises.  The anchor argument of near_rule.hpp (drop the leading tokens that fill no slot) carries over word for word.
//
// The driver of an item is the shortest of its slots' document lists — a posting list or a class list — ties -> the first
// slot; it is found on the device because the class lists' lengths exist only there.  Every document that holds the item
// has a token for every slot, so the answer is a subset of every list (cs_has_all: a lower-bound search in each other
// slot's list) and ascending because the driver is.
//
// The staged run.  One round tests the kPhLanes anchors base .. base + 63 and needs the masks of tokens[base .. base + 64
// + w), w = n for a Near and L - 1 for a phrase, clamped to the document: at most kNearStage = 319 unsigned shorts.
#pragma once
#include "near_rule.hpp"

namespace amdr {

constexpr long long kCsMaxCells = (1LL << 32) / kPhTile - 1;  // cells x 256 threads stay below 2^32 (union_rule.hpp's reason)
static_assert(kPhMaxLen <= 16, "a mask is an unsigned short");

// The postings, the token stream and the list array of the call with its classes.
struct CsIndex {
  PhIndex ph;
  const long long* x_ptr;  // the list array: list k's documents are x_doc[x_ptr[k] .. x_ptr[k + 1])
  const int* x_doc;
  const long long* cls_ptr;  // [n_cls + 1]
  const int* cls_terms;
  long n_cls, cls_first;
};

// One slot of an item, resolved.
struct CsSlot {
  int id;            // the slot id as given
  int same;          // the first slot of the item with this id (the slot's own position when none stands before)
  int known;         // 0: unknown (nothing below is valid)
  long long mb, me;  // a class slot's member ids cls_terms[mb .. me); mb == me: a plain slot
  const int* docs;   // its document list docs[lo .. hi)
  long long lo, hi;
};

struct CsDriver {
  int at;  // the driving slot; -1: the list is empty
  const int* docs;
  long long begin, len;
};

AMDR_TS_HD inline CsSlot cs_slot(const CsIndex& I, int s) {
  CsSlot r{s, 0, 0, 0, 0, nullptr, 0, 0};
  if (s < 0) return r;
  if (s < I.ph.n_terms) {
    r.known = 1, r.docs = I.ph.post_doc, r.lo = I.ph.term_ptr[s], r.hi = I.ph.term_ptr[s + 1];
    return r;
  }
  const long long c = (long long)s - I.ph.n_terms - I.cls_first;
  if (c < 0 || c >= I.n_cls) return r;
  r.known = 1, r.mb = I.cls_ptr[c], r.me = I.cls_ptr[c + 1];
  r.docs = I.x_doc, r.lo = I.x_ptr[I.cls_first + c], r.hi = I.x_ptr[I.cls_first + c + 1];
  if (r.me < r.mb) r.me = r.mb;
  if (r.hi < r.lo) r.hi = r.lo;
  return r;
}

// `same` of every slot, once all L are resolved.
AMDR_TS_HD inline void cs_link_slots(CsSlot* slots, int L) {
  for (int j = 0; j < L; ++j) {
    int k = 0;
    while (slots[k].id != slots[j].id) ++k;  // (ends at k == j at the latest)
    slots[j].same = k;
  }
}

// The driver of the resolved slots[0 .. L): the shortest list, ties to the first slot; empty with an unknown slot.
AMDR_TS_HD inline CsDriver cs_driver(const CsSlot* slots, int L) {
  CsDriver d{-1, nullptr, 0, 0};
  for (int j = 0; j < L; ++j)
    if (!slots[j].known) return d;
  for (int j = 0; j < L; ++j) {
    const long long len = slots[j].hi - slots[j].lo;
    if (d.at < 0 || len < d.len) d = CsDriver{j, slots[j].docs, slots[j].lo, len};
  }
  return d;
}

// Whether the ascending docs[lo .. hi) hold `doc`.
AMDR_TS_HD inline bool cs_list_has(const int* docs, long long lo, long long hi, long long doc) {
  const long long end = hi;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (docs[mid] < doc)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < end && docs[lo] == doc;
}

// Whether `doc`, a candidate of driver D, stands in every other slot's list.
AMDR_TS_HD inline bool cs_has_all(const CsSlot* slots, int L, const CsDriver& D, long long doc) {
  for (int j = 0; j < L; ++j) {
    if (slots[j].same != j || j == slots[D.at].same) continue;  // (a repeated slot, the driver's own list)
    if (!cs_list_has(slots[j].docs, slots[j].lo, slots[j].hi, doc)) return false;
  }
  return true;
}

// The bit mask of the slots token x fills.
AMDR_TS_HD inline unsigned cs_token_mask(int x, const CsSlot* slots, int L, const int* cls_terms) {
  unsigned m = 0;
  for (int j = 0; j < L; ++j) {
    const CsSlot& s = slots[j];
    unsigned bit;
    if (s.same != j)
      bit = (m >> s.same) & 1u;
    else if (s.mb == s.me)
      bit = x == s.id ? 1u : 0u;
    else
      bit = cs_list_has(cls_terms, s.mb, s.me, x) ? 1u : 0u;
    m |= bit << j;
  }
  return m;
}

// The masks of the round that starts at stream position `base` of a document that ends at `end` (base < end): the 64
// anchors and the w positions behind the last of them, clamped to the document.  1 .. kNearStage.
AMDR_TS_HD inline int cs_run_len(long long base, long long end, int kind, int L, int n) {
  return near_run_len(base, end, kind == kSpanPhrase ? L - 1 : n);
}

// One lane's share of one round: the anchor run[lane] of the staged masks run[0 .. len).
AMDR_TS_HD inline bool cs_lane_hit(const unsigned short* run, int len, int lane, int L, int kind, int n) {
  if (lane >= len) return false;
  if (kind == kSpanPhrase) {
    if (lane + L > len) return false;
    for (int j = 0; j < L; ++j)
      if (!((run[lane + j] >> j) & 1u)) return false;
    return true;
  }
  const int last = lane + n < len - 1 ? lane + n : len - 1;
  if (kind == kSpanNearOrdered) {
    if (!(run[lane] & 1u)) return false;
    int cursor = 1;
    for (int q = lane + 1; q <= last; ++q)
      if ((run[q] >> cursor) & 1u)
        if (++cursor == L) return true;
    return false;
  }
  const unsigned full = (1u << L) - 1u;
  unsigned filled = 0;
  for (int q = lane; q <= last; ++q) {
    const unsigned open = run[q] & ~filled & full;  // the unfilled slots the token may fill
    filled |= open & (0u - open);                   // the first of them
    if (filled == 0) return false;                  // (q == lane: the anchor fills no slot)
    if (filled == full) return true;
  }
  return false;
}

// Whether n_items x tiles(cand_max) cells fit one launch; *cells is set when they do.
AMDR_TS_HD inline bool cs_cells(long long n_items, long long cand_max, long long* cells) {
  if (n_items < 0 || cand_max < 0) return false;
  const long long tiles = ph_tiles(cand_max);
  if (n_items > kCsMaxCells / tiles) return false;
  *cells = n_items * tiles;
  return true;
}

// ---- host validation ------------------------------------------------------------------------------------------------------
enum CsError {  // behind NearError's
  kCsClsPtr = 200,  // cls_ptr does not start at 0 or is not monotone
  kCsClsOrder,      // the member ids of a class are not strictly ascending
  kCsOverlap,       // two slots of an unordered item intersect without being equal
};

inline const char* cs_error_text(int e) {
  switch (e) {
    case kCsClsPtr: return "cls_ptr does not run monotonically from 0";
    case kCsClsOrder: return "the member ids of a class are not strictly ascending";
    case kCsOverlap: return "two slots of an unordered item name overlapping, unequal token sets";
    default: return span_error_text(e);
  }
}

// Whether two strictly ascending id sets are equal or disjoint.
inline bool cs_equal_or_disjoint(const int32_t* a, int64_t na, const int32_t* b, int64_t nb) {
  if (na == nb) {
    int64_t k = 0;
    while (k < na && a[k] == b[k]) ++k;
    if (k == na) return true;
  }
  for (int64_t i = 0, j = 0; i < na && j < nb;) {
    if (a[i] == b[j]) return false;
    if (a[i] < b[j])
      ++i;
    else
      ++j;
  }
  return true;
}

// The items and the classes of a call (amdr_class_spans, where class c is the slot id n_terms + c; the "_device" call
// takes its operands as they are).
inline int cs_validate(const int64_t* item_ptr, const int32_t* item_slots, const int32_t* item_kind, const int32_t* item_dist,
                       int64_t n_items, const int64_t* cls_ptr, const int32_t* cls_terms, int64_t n_cls, int64_t n_terms) {
  if (n_cls < 0 || n_terms < 0) return kPhSizes;
  const int bad = span_validate(item_ptr, item_slots, item_kind, item_dist, n_items);
  if (bad != kPhValid) return bad;
  if (n_cls > 0) {
    if (!cls_ptr) return kPhNull;
    if (cls_ptr[0] != 0) return kCsClsPtr;
    for (int64_t c = 0; c < n_cls; ++c)
      if (cls_ptr[c + 1] < cls_ptr[c]) return kCsClsPtr;
    if (cls_ptr[n_cls] > 0 && !cls_terms) return kPhNull;
    for (int64_t c = 0; c < n_cls; ++c)
      for (int64_t j = cls_ptr[c] + 1; j < cls_ptr[c + 1]; ++j)
        if (cls_terms[j] <= cls_terms[j - 1]) return kCsClsOrder;
  }
  for (int64_t p = 0; p < n_items; ++p) {
    if (item_kind[p] != kSpanNearUnordered) continue;
    const int64_t b = item_ptr[p], L = item_ptr[p + 1] - b;
    const int32_t* set[kNearMaxTerms];
    int64_t size[kNearMaxTerms];
    for (int64_t j = 0; j < L; ++j) {
      const int32_t s = item_slots[b + j];
      const int64_t c = (int64_t)s - n_terms;
      if (s >= 0 && s < n_terms)
        set[j] = &item_slots[b + j], size[j] = 1;
      else if (c >= 0 && c < n_cls)
        set[j] = cls_terms + cls_ptr[c], size[j] = cls_ptr[c + 1] - cls_ptr[c];
      else
        set[j] = nullptr, size[j] = 0;  // (unknown: the item is empty whatever the others are)
    }
    for (int64_t j = 0; j < L; ++j)
      for (int64_t k = 0; k < j; ++k)
        if (!cs_equal_or_disjoint(set[j], size[j], set[k], size[k])) return kCsOverlap;
  }
  return kPhValid;
}

}  // namespace amdr

// The rules of amdr_span_lists (phrase_scope.hip) that are plain C++: what a Near is, when a document holds it, what one
// lane of the scan does with the staged token run of a round, and the host validation of a mixed batch of phrases and
// Nears.  The kernels, the host twin and the host check (check_near_scope.cpp, which applies the same functions tile by
// tile, round by round and lane by lane on the CPU) share this one source, in the style of phrase_rule.hpp, whose driver
// (ph_driver) and conjunction (ph_has_all) a Near reuses unchanged.
//
// The rule.  A Near is M term ids t[0 .. M), 2 <= M <= kNearMaxTerms — repeats are allowed and are meaningful — a
// distance n, 1 <= n <= kNearMaxDist, and a kind.  Within one document d, tokens[doc_ptr[d] .. doc_ptr[d + 1]):
//   unordered  d HOLDS it when some run of at most n + 1 consecutive tokens of d contains every distinct term at least
//              as many times as the Near names it: Near(a, a, b) needs two a and one b inside one window; for two
//              different tokens at p and q this is |q - p| <= n.
//   ordered    d HOLDS it when there are positions p0 < p1 < ... < p[M-1] inside d with tokens[p_i] == t[i] and
//              p[M-1] - p0 <= n.
// A window never reaches into the next document; at the end of a document it is clamped.  An id outside [0, n_terms)
// anywhere in the Near gives an empty list without reading anything, and so does an M or n outside its range (the host
// twin refuses those; the "_device" call takes its operands as they are).
//
// Anchors.  The scan tries every position p of the document as the FIRST token of a window, and a lane whose token is no
// member does nothing.  That loses no match:
//   unordered  take any window that holds the Near and drop its leading tokens up to the first one that is a member
//              (equal to some t[j]): what is left still holds every term, is no longer, and starts at a member — any
//              member, not just t[0].  So it suffices to scan [p, p + n] from every member position p.
//   ordered    p0 holds t[0], so only those positions are anchors; from a fixed anchor, taking the EARLIEST next match of
//              each further term is optimal (any other choice ends no sooner), but a later anchor may succeed where an
//              earlier one fails (a a b with n = 1), so every anchor is tried.
// The tally of the unordered form is a mask of the M slots: an occurrence of a token fills the first unfilled slot that
// names it, and the window holds the Near when every slot is filled — the multiset cover, without a table of quotas.
//
// The staged run.  One round tests the kPhLanes anchors base .. base + 63 and reads tokens[base .. base + 64 + n), clamped
// to the document: at most kNearStage = 319 ints, staged once and scanned from there (near_lane_hit takes the run, not
// the stream, so the host check hands it an array of exactly that size).
#pragma once
#include "phrase_rule.hpp"

namespace amdr {

constexpr int kNearMaxTerms = 8;   // tokens of a Near
constexpr int kNearMaxDist = 255;  // the largest distance
constexpr int kNearStage = kPhLanes + kNearMaxDist;  // ints of one round's staged run, at most

// The kinds of an item of amdr_span_lists.
enum SpanKind { kSpanPhrase = 0, kSpanNearUnordered = 1, kSpanNearOrdered = 2 };

// Whether an item of L tokens is one the rule defines; an item that is not gets an empty list.
AMDR_TS_HD inline bool span_sized(int kind, long long L, int dist) {
  if (kind == kSpanPhrase) return L >= 2 && L <= kPhMaxLen;
  if (kind != kSpanNearUnordered && kind != kSpanNearOrdered) return false;
  return L >= 2 && L <= kNearMaxTerms && dist >= 1 && dist <= kNearMaxDist;
}

// The driver of an item: the phrase's (the shortest posting list among the tokens, ties to the first).
AMDR_TS_HD inline PhDriver span_driver(const PhIndex& I, const int* terms, long long L, int kind, int dist) {
  return span_sized(kind, L, dist) ? ph_driver(I, terms, L) : PhDriver{-1, -1, 0, 0};
}

// The tokens of the round that starts at stream position `base` of a document that ends at `end` (base < end): the 64
// anchors and the n tokens behind the last of them, clamped to the document.  1 .. kNearStage.
AMDR_TS_HD inline int near_run_len(long long base, long long end, int n) {
  const long long want = kPhLanes + n, have = end - base;
  return (int)(have < want ? have : want);
}

// One lane's share of one round: the anchor run[lane] of the staged run[0 .. len).  The window is run[lane .. lane + n],
// clamped to len; lane + n < kPhLanes + n, so an unclamped window lies inside an unclamped run.
AMDR_TS_HD inline bool near_lane_hit(const int* run, int len, int lane, const int* terms, int M, bool ordered, int n) {
  if (lane >= len) return false;
  const int last = lane + n < len - 1 ? lane + n : len - 1;
  // (the Near is read once: a step then waits for ONE dependent read, run[q], where `terms` lies in LDS as `run` does)
  if (ordered) {
    if (run[lane] != terms[0]) return false;
    int cursor = 1, want = terms[1];
    for (int q = lane + 1; q <= last; ++q)
      if (run[q] == want) {
        if (++cursor == M) return true;
        want = terms[cursor];
      }
    return false;
  }
  int t[kNearMaxTerms];
  for (int j = 0; j < kNearMaxTerms; ++j) t[j] = j < M ? terms[j] : -1;  // (a token is never negative)
  const unsigned full = (1u << M) - 1u;
  unsigned filled = 0;
  for (int q = lane; q <= last; ++q) {
    const int x = run[q];
    unsigned open = 0;  // the unfilled slots that name x
    for (int j = 0; j < kNearMaxTerms; ++j) open |= (t[j] == x ? 1u : 0u) << j;
    open &= ~filled & full;
    filled |= open & (0u - open);  // the first of them
    if (filled == 0) return false;  // (q == lane: the anchor is no member)
    if (filled == full) return true;
  }
  return false;
}

// ---- host validation ------------------------------------------------------------------------------------------------------
enum NearError {  // behind PhError's
  kNearKind = 100,  // a kind outside 0 .. 2
  kNearLength,      // a Near shorter than 2 or longer than kNearMaxTerms tokens
  kNearDist,        // a Near's distance outside 1 .. kNearMaxDist
};

inline const char* span_error_text(int e) {
  switch (e) {
    case kPhPtr: return "item_ptr does not run monotonically from 0";
    case kNearKind: return "an item kind outside 0 .. 2";
    case kNearLength: return "a Near of fewer than 2 or more than 8 tokens";
    case kNearDist: return "a Near's distance outside 1 .. 255";
    default: return ph_error_text(e);
  }
}

// The items of a call (amdr_span_lists; the "_device" call takes them as they are).  A phrase's dist is not read.
inline int span_validate(const int64_t* item_ptr, const int32_t* item_terms, const int32_t* item_kind, const int32_t* item_dist,
                         int64_t n_items) {
  if (n_items < 0) return kPhSizes;
  if (!item_ptr || (n_items > 0 && (!item_kind || !item_dist))) return kPhNull;
  if (item_ptr[0] != 0) return kPhPtr;
  for (int64_t p = 0; p < n_items; ++p) {
    if (item_ptr[p + 1] < item_ptr[p]) return kPhPtr;
    const int64_t L = item_ptr[p + 1] - item_ptr[p];
    const int kind = item_kind[p];
    if (kind == kSpanPhrase) {
      if (L < 2 || L > kPhMaxLen) return kPhLength;
    } else if (kind == kSpanNearUnordered || kind == kSpanNearOrdered) {
      if (L < 2 || L > kNearMaxTerms) return kNearLength;
      if (item_dist[p] < 1 || item_dist[p] > kNearMaxDist) return kNearDist;
    } else {
      return kNearKind;
    }
  }
  if (n_items > 0 && !item_terms) return kPhNull;
  return kPhValid;
}

}  // namespace amdr

// The rules of amdr_unit_spans (unit_span.hip) that are plain C++: what a unit item is, how one ROUND of 64 tokens is
// decided from the wave's ballots, what the unit that is still open at the end of a round carries into the next one, and
// the host validation of the operands.  The kernel and the host check (check_unit_span.cpp, which applies the same
// functions tile by tile and round by round on the CPU) share this one source, in the style of class_span_rule.hpp, whose
// CsIndex, cs_slot, cs_link_slots, cs_driver, cs_has_all and cs_token_mask a unit item reuses unchanged.
//
// The rule.  Beside the token stream lies one BREAK byte per token (amdr_bm25_set_breaks): bit 0 — the token begins a
// sentence, bit 1 — it begins a paragraph; a paragraph start is a sentence start too (0, 1, 3), and the first token of a
// document begins both whatever its byte says.  The flagged tokens partition a document into UNITS.  A unit item
// (buyer /s seller, buyer +p seller) is L slot ids, 2 <= L <= kUsMaxSlots, as a class span's are, and a kind: bit 0
// ordered, bit 1 paragraph (sentence otherwise).  Within one document:
//   unordered  some unit admits an assignment of the slots to DISTINCT positions of the unit, each token filling its slot:
//              a bipartite matching.
//   ordered    positions p0 < p1 < ... inside ONE unit, token p_i filling slot i.
// Groups.  Slots with the same id form a group (cs_link_slots); slots with DIFFERENT ids must name DISJOINT token sets in
// an unordered item (us_validate; pack() gives equal sets one id and raises for overlapping unequal ones, the reason
// class_span_rule.hpp gives).  A token then belongs to one group at most, so the matching exists in a unit exactly when
// every group of k slots has at least k of its tokens there: popcount(B_group & unit) >= k, Hall's condition on disjoint
// groups.  The ordered form takes, slot after slot, the earliest set bit of the slot's ballot behind the previous slot's
// inside the unit: the greedy subsequence match, which finds a match whenever one exists.
//
// A round.  Lane i of the wave holds token base + i of the document (len <= 64 of them) and its break byte; the wave
// forms `starts` — the unit bit of the breaks, bit 0 forced in the document's first round — and one ballot B[j] per slot
// (equal for the slots of a group).  From there us_round is wave-uniform arithmetic on 64-bit words: the bits below the
// first start continue the unit the CARRY describes, every set bit of `starts` clears the carry and opens the next unit,
// and the last unit's state stays in the carry.  The wave LOOPS over the set bits of `starts` (one scalar iteration per
// unit of the round, a handful in prose; at most 64) instead of giving each lane one unit: a unit's test is a few scalar
// popcounts, the carried unit and the hit vote would otherwise need a cross-lane step of their own, and no LDS is used.
#pragma once
#include "class_span_rule.hpp"

namespace amdr {

constexpr int kUsMaxSlots = 8;  // slots of a unit item (kNearMaxTerms)
enum UsKind { kUsOrdered = 1, kUsParagraph = 2 };
enum UsBreak { kBrkSentence = 1, kBrkParagraph = 2 };
static_assert(kUsMaxSlots <= kNearMaxTerms && kPhLanes == 64, "a round is one 64-bit ballot per slot");

// Whether an item of L slots and this kind is one the rule defines; an item that is not gets an empty list.
AMDR_TS_HD inline bool us_sized(int kind, long long L) { return kind >= 0 && kind <= 3 && L >= 2 && L <= kUsMaxSlots; }

// The break bit that opens a unit of this kind.
AMDR_TS_HD inline int us_break_bit(int kind) { return (kind & kUsParagraph) ? kBrkParagraph : kBrkSentence; }

// Whether a break byte is one amdr_bm25_set_breaks takes.
AMDR_TS_HD inline bool us_break_valid(int b) { return b == 0 || b == 1 || b == 3; }

// The shape of an item as the round rule reads it: per slot the first slot of its group (CsSlot.same) and, at that first
// slot, the group's size (0 elsewhere).
struct UsShape {
  int L, ordered;
  unsigned char same[kUsMaxSlots], need[kUsMaxSlots];
};

AMDR_TS_HD inline UsShape us_shape(const CsSlot* slots, int L, int kind) {
  UsShape s{L, kind & kUsOrdered, {}, {}};
  for (int j = 0; j < kUsMaxSlots; ++j) s.same[j] = 0, s.need[j] = 0;
  for (int j = 0; j < L; ++j) {
    s.same[j] = (unsigned char)slots[j].same;
    ++s.need[slots[j].same];
  }
  return s;
}

// The state of the unit that is open at the end of a round.  unordered: have[j], at a group's first slot, the group's
// tokens seen so far, saturated at kUsMaxSlots; ordered: cursor, the slots matched so far.
struct UsCarry {
  int cursor;
  unsigned char have[kUsMaxSlots];
};

AMDR_TS_HD inline UsCarry us_carry_clear() {
  UsCarry c;
  c.cursor = 0;
  for (int j = 0; j < kUsMaxSlots; ++j) c.have[j] = 0;
  return c;
}

AMDR_TS_HD inline unsigned long long us_low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }  // n in 0 .. 64

// One segment (the bits `seg` of one unit inside the round) on top of the carry; whether the unit now holds the item.
AMDR_TS_HD inline bool us_segment(const UsShape& s, const unsigned long long* B, unsigned long long seg, UsCarry& c) {
  if (s.L < 2) return false;  // (an item the rule does not define holds nowhere)
  // (every loop runs to the constant kUsMaxSlots with constant indices: unrolled, B and the carry stay in registers)
  if (s.ordered) {
    unsigned long long from = seg;
    for (int j = 0; j < kUsMaxSlots; ++j) {
      if (j < c.cursor || j >= s.L) continue;  // (slot j is the cursor's from here on)
      const unsigned long long m = B[j] & from;
      if (!m) break;
      const int p = __builtin_ctzll(m);
      from &= ~us_low_bits(p + 1);  // strictly behind p
      c.cursor = j + 1;
    }
    return c.cursor == s.L;
  }
  bool all = true;
  for (int j = 0; j < kUsMaxSlots; ++j) {
    if (j >= s.L || !s.need[j]) continue;  // (not a group's first slot)
    int have = c.have[j] + __builtin_popcountll(B[j] & seg);
    if (have > kUsMaxSlots) have = kUsMaxSlots;
    c.have[j] = (unsigned char)have;
    all = all && have >= s.need[j];
  }
  return all;
}

// One round: B[j] the ballot of slot j over the round's lanes, `starts` the ballot of the unit starts (bit 0 already forced
// in a document's first round), len the round's tokens (1 .. 64).  Bits at and above len are ignored.  Returns whether a
// unit of the round — the carried one included — holds the item; otherwise `c` is the state of the round's last unit.
AMDR_TS_HD inline bool us_round(const UsShape& s, const unsigned long long* B, unsigned long long starts, int len, UsCarry& c) {
  const unsigned long long valid = us_low_bits(len);
  starts &= valid;
  const int first = starts ? __builtin_ctzll(starts) : len;
  if (first > 0 && us_segment(s, B, us_low_bits(first), c)) return true;  // the carried unit goes on
  while (starts) {
    const int b = __builtin_ctzll(starts);
    starts &= starts - 1;
    const int e = starts ? __builtin_ctzll(starts) : len;
    c = us_carry_clear();
    if (us_segment(s, B, us_low_bits(e) & ~us_low_bits(b), c)) return true;
  }
  return false;
}

// ---- host validation ------------------------------------------------------------------------------------------------------
enum UsError {  // behind CsError's
  kUsLength = 300,  // an item of fewer than 2 or more than kUsMaxSlots slots
  kUsKind,          // a kind outside 0 .. 3
  kUsTwoIds,        // two slots of an unordered item with different ids name intersecting token sets
};

inline const char* us_error_text(int e) {
  switch (e) {
    case kUsLength: return "a unit item of fewer than 2 or more than 8 slots";
    case kUsKind: return "a unit item's kind outside 0 .. 3 (bit 0 ordered, bit 1 paragraph)";
    case kUsTwoIds: return "two slots of an unordered item with different ids name intersecting token sets (equal sets share one id)";
    default: return cs_error_text(e);
  }
}

// The items and the classes of a call (amdr_unit_spans, where class c is the slot id n_terms + c).
inline int us_validate(const int64_t* item_ptr, const int32_t* item_slots, const int32_t* item_kind, int64_t n_items,
                       const int64_t* cls_ptr, const int32_t* cls_terms, int64_t n_cls, int64_t n_terms) {
  if (n_items < 0 || n_cls < 0 || n_terms < 0) return kPhSizes;
  if (!item_ptr || (n_items > 0 && !item_kind)) return kPhNull;
  if (item_ptr[0] != 0) return kPhPtr;
  for (int64_t p = 0; p < n_items; ++p) {
    if (item_ptr[p + 1] < item_ptr[p]) return kPhPtr;
    const int64_t L = item_ptr[p + 1] - item_ptr[p];
    if (L < 2 || L > kUsMaxSlots) return kUsLength;
    if (item_kind[p] < 0 || item_kind[p] > 3) return kUsKind;
  }
  if (n_items > 0 && item_ptr[n_items] > 0 && !item_slots) return kPhNull;
  const int64_t none = 0;
  const int bad = cs_validate(&none, nullptr, nullptr, nullptr, 0, cls_ptr, cls_terms, n_cls, n_terms);  // the classes alone
  if (bad != kPhValid) return bad;
  for (int64_t p = 0; p < n_items; ++p) {
    if (item_kind[p] & kUsOrdered) continue;
    const int64_t b = item_ptr[p], L = item_ptr[p + 1] - b;
    const int32_t* set[kUsMaxSlots];
    int64_t size[kUsMaxSlots];
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
      for (int64_t k = 0; k < j; ++k) {
        if (item_slots[b + j] == item_slots[b + k]) continue;
        if (!cs_equal_or_disjoint(set[j], size[j], set[k], size[k])) return kCsOverlap;
        if (size[j] > 0 && size[j] == size[k] && set[j][0] == set[k][0]) return kUsTwoIds;  // (equal, since not overlapping)
      }
  }
  return kPhValid;
}

}  // namespace amdr

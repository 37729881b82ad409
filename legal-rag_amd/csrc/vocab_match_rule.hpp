// The rules of amdr_vocab_match (vocab_match.hip) that are plain C++: how a vocabulary term's UTF-8 bytes become code
// points, when a Wildcard pattern and when a Fuzzy pattern names a term, the length pre-test, where a term's bit stands
// in a tile's bitmap, how a word of that bitmap becomes a pattern's row of (term id, distance), the workspace layout and
// the validation of the operands.  The kernels, the host twin's validation and the host check (check_vocab_match.cpp,
// which applies the same functions cell by cell and word by word on the CPU) share this one source, in the style of
// union_rule.hpp and facet_rule.hpp.
//
// The rule.  A pattern is M code points (1 .. kVmMaxLen) with a kind and an argument.
//   kind 0, Wildcard   kVmAnyOne ('?') stands for exactly one code point, kVmAnyRun ('*') for any run of code points, the
//                      empty one included, every other value for itself.  The two are values ABOVE 0x10FFFF, so a literal
//                      question mark in a TERM is an ordinary code point.  The argument is 0 and the pattern holds at
//                      least one literal.
//   kind 1, Fuzzy      the term is within `arg` (1 or 2) of the pattern under the optimal-string-alignment distance:
//                      insertion, deletion, substitution and the transposition of two ADJACENT code points cost 1 each
//                      and no code point is edited twice ("ca" -> "abc" is 3, not 2).  Every value is a code point.
// Code points, never bytes: é against e is one substitution.  A term of zero bytes matches nothing.  A pattern that breaks
// a promise above (vm_pattern_info: ok == false) matches nothing: the kernels take the patterns as they lie on the device.
//
// The cell is (pattern p, tile y of kVmTile consecutive term ids); what lies inside one is a bitmap of kVmTile bits.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define AMDR_VM_HD __host__ __device__
#else
#define AMDR_VM_HD
#endif

namespace amdr {

constexpr int kVmTile = 8192;                   // terms per tile: a 1 KiB bitmap (AMDR_VOCAB_TILE_TERMS)
constexpr int kVmWords = kVmTile / 32;          // 32-bit words of a tile's bitmap
constexpr int kVmThreads = 256;                 // threads of a block
constexpr int kVmPer = kVmWords / kVmThreads;   // consecutive words a thread of the write pass expands
static_assert(kVmTile % 32 == 0 && kVmWords % kVmThreads == 0 && kVmPer >= 1, "whole words per thread");
constexpr int kVmMaxLen = 64;                   // code points of a pattern (AMDR_VOCAB_MAX_PATTERN)
constexpr int kVmMaxCap = 4096;                 // the widest row of matches (AMDR_VOCAB_MAX_ITEMS)
constexpr int kVmMaxEdits = 2;
constexpr long long kVmMaxCells = (1LL << 24) - 1;  // blocks of the one-dimensional grid
constexpr unsigned kVmMaxCodePoint = 0x10FFFFu;
constexpr unsigned kVmAnyOne = 0x110000u;       // '?'
constexpr unsigned kVmAnyRun = 0x110001u;       // '*'
constexpr int kVmFar = 1000;                    // a distance outside the band
constexpr int kVmNoDist = 255;                  // the padding of the dist rows

enum VmKind { kVmWildcard = 0, kVmFuzzy = 1 };

// The resident vocabulary: term i is blob[offs[i] .. offs[i + 1]), cp_len[i] its code-point count.
struct VmVocab {
  const unsigned char* blob;
  const long long* offs;
  const int* cp_len;
  long long n_terms;
};

// ---- cells and the workspace ---------------------------------------------------------------------------------------------
AMDR_VM_HD inline long long vm_tiles(long long n_terms) {
  const long long t = (n_terms + kVmTile - 1) / kVmTile;
  return t < 1 ? 1 : t;  // (at least one: every pattern has a block that writes its n_match and pads its row)
}
AMDR_VM_HD inline bool vm_cells(long long n_pat, long long n_terms, long long* cells) {
  if (n_pat < 0 || n_terms < 0) return false;
  const long long tiles = vm_tiles(n_terms);
  if (n_pat > kVmMaxCells / tiles) return false;
  *cells = n_pat * tiles;
  return true;
}
// counts i64 [cells] | offsets i64 [cells + 1] | parked bitmaps u32 [cells][kVmWords], each region aligned to 256 bytes
constexpr long long kVmAlign = 256;
AMDR_VM_HD inline long long vm_align(long long b) { return (b + kVmAlign - 1) / kVmAlign * kVmAlign; }
struct VmWork {
  long long off_counts, off_offsets, off_parked, total;
};
AMDR_VM_HD inline VmWork vm_work(long long cells) {
  VmWork w;
  w.off_counts = 0;
  w.off_offsets = vm_align(cells * 8);
  w.off_parked = w.off_offsets + vm_align((cells + 1) * 8);
  w.total = cells ? w.off_parked + vm_align(cells * kVmWords * 4) : 0;
  return w;
}

// ---- UTF-8 ---------------------------------------------------------------------------------------------------------------
// The code point that starts at byte `at` (< end) and the byte behind it.  Bounded: whatever the bytes, nothing at or
// behind `end` is read — a sequence cut short by the term's end yields the bits it has.
AMDR_VM_HD inline long long vm_decode(const unsigned char* s, long long at, long long end, unsigned* cp) {
  const unsigned b = s[at++];
  int more = b < 0xC0u ? 0 : b < 0xE0u ? 1 : b < 0xF0u ? 2 : 3;
  unsigned v = more ? (b & (0x3Fu >> more)) : b;
  for (; more > 0 && at < end; --more) v = (v << 6) | (s[at++] & 0x3Fu);
  *cp = v;
  return at;
}

// The code points of well-formed bytes: those that are no continuation byte.
inline int vm_cp_count(const unsigned char* s, long long b, long long e) {
  long long n = 0;
  for (long long i = b; i < e; ++i) n += (s[i] & 0xC0u) != 0x80u;
  return n > 0x7fffffffLL ? 0x7fffffff : (int)n;
}

// Whether s[b .. e) is well-formed UTF-8: shortest forms only, no surrogates, nothing above U+10FFFF.
inline bool vm_utf8_ok(const unsigned char* s, long long b, long long e) {
  long long i = b;
  while (i < e) {
    const unsigned c = s[i];
    int more;
    unsigned v, least;
    if (c < 0x80u) {
      ++i;
      continue;
    } else if (c >= 0xC2u && c < 0xE0u) {
      more = 1, v = c & 0x1Fu, least = 0x80u;
    } else if (c >= 0xE0u && c < 0xF0u) {
      more = 2, v = c & 0x0Fu, least = 0x800u;
    } else if (c >= 0xF0u && c < 0xF5u) {
      more = 3, v = c & 0x07u, least = 0x10000u;
    } else {
      return false;
    }
    if (i + more >= e) return false;
    for (int k = 1; k <= more; ++k) {
      if ((s[i + k] & 0xC0u) != 0x80u) return false;
      v = (v << 6) | (s[i + k] & 0x3Fu);
    }
    if (v < least || v > kVmMaxCodePoint || (v >= 0xD800u && v < 0xE000u)) return false;
    i += more + 1;
  }
  return true;
}

// ---- a pattern ------------------------------------------------------------------------------------------------------------
struct VmPat {
  int m;         // code points
  int kind;      // VmKind
  int edits;     // Fuzzy: 1 or 2; Wildcard: 0
  int min_len;   // Wildcard: the literals and the '?': the least code points of a term it names
  bool any_run;  // Wildcard: holds a '*'
  bool ok;       // false: the pattern names nothing
};

// Whether [b, e) is a pattern's span inside a code-point array of cp_total values.
AMDR_VM_HD inline bool vm_span_ok(long long b, long long e, long long cp_total) {
  return b >= 0 && e > b && e - b <= kVmMaxLen && e <= cp_total;
}

// What the match needs to know of pattern pat[0 .. m): every promise of the rule is checked here, so any contents are safe.
AMDR_VM_HD inline VmPat vm_pattern_info(const unsigned* pat, int m, int kind, int arg) {
  VmPat P;
  P.m = m, P.kind = kind, P.edits = 0, P.min_len = 0, P.any_run = false;
  P.ok = m >= 1 && m <= kVmMaxLen && (kind == kVmWildcard || kind == kVmFuzzy);
  if (!P.ok) return P;
  if (kind == kVmFuzzy) {
    P.edits = arg;
    P.ok = arg >= 1 && arg <= kVmMaxEdits;
    for (int j = 0; j < m; ++j) P.ok = P.ok && pat[j] <= kVmMaxCodePoint;
    return P;
  }
  int literals = 0;
  for (int j = 0; j < m; ++j) {
    const unsigned c = pat[j];
    if (c == kVmAnyRun) {
      P.any_run = true;
    } else {
      ++P.min_len;
      if (c != kVmAnyOne) {
        ++literals;
        P.ok = P.ok && c <= kVmMaxCodePoint;
      }
    }
  }
  P.ok = P.ok && arg == 0 && literals >= 1;
  return P;
}

// The length pre-test on code-point counts: false only for a term the pattern cannot name.
AMDR_VM_HD inline bool vm_len_ok(const VmPat& P, int n) {
  if (n <= 0) return false;
  if (P.kind == kVmFuzzy) return n - P.m <= P.edits && P.m - n <= P.edits;
  return P.any_run ? n >= P.min_len : n == P.min_len;
}

// Wildcard: greedy, with ONE backtrack point — the last '*' seen and the term position it has swallowed up to.
AMDR_VM_HD inline bool vm_wild_match(const unsigned* pat, int m, const unsigned char* s, long long b, long long e) {
  if (e <= b) return false;
  int p = 0, star_p = -1;
  long long t = b, star_t = b;
  while (t < e) {
    if (p < m && pat[p] == kVmAnyRun) {
      star_p = p++;
      star_t = t;
      continue;
    }
    unsigned c;
    const long long next = vm_decode(s, t, e, &c);
    if (p < m && (pat[p] == kVmAnyOne || pat[p] == c)) {
      ++p;
      t = next;
    } else if (star_p >= 0) {  // the run takes one more code point
      unsigned skipped;
      star_t = vm_decode(s, star_t, e, &skipped);
      t = star_t;
      p = star_p + 1;
    } else {
      return false;
    }
  }
  while (p < m && pat[p] == kVmAnyRun) ++p;
  return p == m;
}

AMDR_VM_HD inline int vm_min(int a, int b) { return a < b ? a : b; }

// One cell of the banded recurrence: row i (the term's i-th code point `ti`, the one before it `tp`), diagonal d = j - i.
//   diag = D[i-1][j-1], up = D[i-1][j], left = D[i][j-1], trans = D[i-2][j-2]
AMDR_VM_HD inline int vm_osa_cell(const unsigned* pat, int m, int edits, int i, int d, unsigned ti, unsigned tp, int diag, int up,
                                  int left, int trans) {
  const int j = i + d;
  if (d > edits || -d > edits || j < 0 || j > m) return kVmFar;
  if (j == 0) return i;
  const unsigned pj = pat[j - 1];
  int best = diag + (ti != pj ? 1 : 0);
  best = vm_min(best, up + 1);
  best = vm_min(best, left + 1);
  if (i >= 2 && j >= 2 && ti == pat[j - 2] && tp == pj) best = vm_min(best, trans + 1);
  return vm_min(best, kVmFar);
}

// The first row, D[0][d] = d.
AMDR_VM_HD inline int vm_osa_first(int m, int edits, int d) { return d >= 0 && d <= edits && d <= m ? d : kVmFar; }

// Fuzzy: the optimal-string-alignment distance between pat[0 .. m) and the term s[b .. e) when it is <= edits, else a
// value > edits.  A band of 2 x kVmMaxEdits + 1 diagonals in named scalars with the two rows before (the transposition
// reaches two rows back): a path of cost <= edits never leaves the diagonals |j - i| <= edits, so inside the band the
// values <= edits are the full matrix's.
AMDR_VM_HD inline int vm_osa_banded(const unsigned* pat, int m, int edits, const unsigned char* s, long long b, long long e) {
  int p0 = vm_osa_first(m, edits, -2), p1 = vm_osa_first(m, edits, -1), p2 = vm_osa_first(m, edits, 0);
  int p3 = vm_osa_first(m, edits, 1), p4 = vm_osa_first(m, edits, 2);
  int q0 = kVmFar, q1 = kVmFar, q2 = kVmFar, q3 = kVmFar, q4 = kVmFar;
  unsigned tp = 0;
  int i = 0;
  for (long long t = b; t < e;) {
    unsigned ti;
    t = vm_decode(s, t, e, &ti);
    ++i;
    if (i > m + edits) return kVmFar;  // (a term longer than the pre-test lets through)
    const int c0 = vm_osa_cell(pat, m, edits, i, -2, ti, tp, p0, p1, kVmFar, q0);
    const int c1 = vm_osa_cell(pat, m, edits, i, -1, ti, tp, p1, p2, c0, q1);
    const int c2 = vm_osa_cell(pat, m, edits, i, 0, ti, tp, p2, p3, c1, q2);
    const int c3 = vm_osa_cell(pat, m, edits, i, 1, ti, tp, p3, p4, c2, q3);
    const int c4 = vm_osa_cell(pat, m, edits, i, 2, ti, tp, p4, kVmFar, c3, q4);
    // a row and the row before both beyond `edits`: every later value derives from one of them and is no smaller
    const int now = vm_min(vm_min(vm_min(c0, c1), vm_min(c2, c3)), c4);
    const int was = vm_min(vm_min(vm_min(p0, p1), vm_min(p2, p3)), p4);
    if (now > edits && was > edits) return kVmFar;
    q0 = p0, q1 = p1, q2 = p2, q3 = p3, q4 = p4;
    p0 = c0, p1 = c1, p2 = c2, p3 = c3, p4 = c4;
    tp = ti;
  }
  const int d = m - i;  // D[i][m] stands on diagonal m - i
  if (i == 0) return kVmFar;
  return d == -2 ? p0 : d == -1 ? p1 : d == 0 ? p2 : d == 1 ? p3 : d == 2 ? p4 : kVmFar;
}

// Whether pattern P names term `term`; *dist: its distance (0 for a wildcard).  A term outside the vocabulary is never read.
AMDR_VM_HD inline bool vm_term_match(const VmVocab& V, const unsigned* pat, const VmPat& P, long long term, int* dist) {
  *dist = 0;
  if (!P.ok || term < 0 || term >= V.n_terms) return false;
  if (!vm_len_ok(P, V.cp_len[term])) return false;
  const long long b = V.offs[term], e = V.offs[term + 1];
  if (e <= b) return false;
  if (P.kind == kVmWildcard) return vm_wild_match(pat, P.m, V.blob, b, e);
  *dist = vm_osa_banded(pat, P.m, P.edits, V.blob, b, e);
  return *dist <= P.edits;
}

// ---- the bitmap ----------------------------------------------------------------------------------------------------------
AMDR_VM_HD inline int vm_bit_word(long long term, long long tile) { return (int)((term - tile * kVmTile) >> 5); }
AMDR_VM_HD inline unsigned vm_bit_mask(long long term) { return 1u << (unsigned)(term & 31); }
AMDR_VM_HD inline int vm_popcount(unsigned w) { return __builtin_popcount(w); }

// Word w (of kVmWords) of tile `tile` expanded into pattern rows, ascending: bit b is term tile * kVmTile + w * 32 + b and
// the r-th set bit goes to position at + r of the row — unless that position is >= item_cap: it is dropped.  The distance
// is computed again for the kept terms only.  Returns the number of set bits, written or not.
AMDR_VM_HD inline int vm_expand_word(unsigned bits, long long tile, int w, long long at, long long item_cap, const VmVocab& V,
                                     const unsigned* pat, const VmPat& P, int* ids_row, unsigned char* dist_row) {
  const long long first = tile * kVmTile + (long long)w * 32;
  int r = 0;
  for (; bits; bits &= bits - 1, ++r) {
    const int b = __builtin_ctz(bits);
    if (at + r >= 0 && at + r < item_cap) {
      int dist;
      (void)vm_term_match(V, pat, P, first + b, &dist);
      ids_row[at + r] = (int)(first + b);
      dist_row[at + r] = (unsigned char)(dist <= kVmMaxEdits ? dist : kVmNoDist);
    }
  }
  return r;
}

// ---- validation ----------------------------------------------------------------------------------------------------------
enum VmError {
  kVmValid = 0,
  kVmNull,      // a null array
  kVmSizes,     // a negative size
  kVmCap,       // item_cap outside 1 .. kVmMaxCap
  kVmCells,     // more than kVmMaxCells cells
  kVmTerms,     // more than 2^31 - 1 terms
  kVmPtr,       // pat_ptr does not run monotonically from 0 to cp_total
  kVmLength,    // a pattern of 0 or more than kVmMaxLen code points
  kVmKindArg,   // a kind outside {0, 1}, a Fuzzy's edits outside 1 .. 2, a Wildcard's argument not 0
  kVmValue,     // a value that is neither a code point nor, in a Wildcard, one of the two reserved ones
  kVmLiteral,   // a Wildcard without a literal
  kVmOffsets,   // vocabulary offsets that do not ascend from 0
  kVmUtf8,      // a term that is not well-formed UTF-8
};

inline const char* vm_error_text(int e) {
  switch (e) {
    case kVmNull: return "a null handle or array";
    case kVmSizes: return "a negative size";
    case kVmCap: return "item_cap outside 1 .. 4096";
    case kVmCells: return "more than 2^24 - 1 cells (patterns x tiles of terms)";
    case kVmTerms: return "more than 2^31 - 1 terms";
    case kVmPtr: return "pat_ptr does not run monotonically from 0 to cp_total";
    case kVmLength: return "a pattern of 0 or more than 64 code points";
    case kVmKindArg: return "a kind outside {0, 1}, a Fuzzy's edits outside 1 .. 2 or a Wildcard's argument not 0";
    case kVmValue: return "a pattern value that is no code point (the reserved '?' and '*' stand in a Wildcard only)";
    case kVmLiteral: return "a Wildcard without a literal names every term of its length";
    case kVmOffsets: return "the vocabulary's offsets do not ascend from 0";
    case kVmUtf8: return "a vocabulary term is not well-formed UTF-8";
    default: return "ok";
  }
}

// The sizes and pointers every entry point refuses before anything is enqueued; *cells: the cells of the launch.
inline int vm_check_args(const void* handle, long long n_terms, const void* pat_cp, const void* pat_ptr, const void* pat_kind,
                         const void* pat_arg, long long n_pat, long long cp_total, long long item_cap, const void* ids,
                         const void* dist, const void* n_match, long long* cells) {
  if (!handle) return kVmNull;
  if (n_pat < 0 || cp_total < 0 || n_terms < 0) return kVmSizes;
  if (item_cap < 1 || item_cap > kVmMaxCap) return kVmCap;
  if (!vm_cells(n_pat, n_terms, cells)) return kVmCells;
  if (n_pat > 0 && (!pat_cp || !pat_ptr || !pat_kind || !pat_arg || !ids || !dist || !n_match)) return kVmNull;
  return kVmValid;
}

// The patterns of a host-pointer call (amdr_vocab_match; the "_device" call takes them as they lie on the device).
inline int vm_validate(const uint32_t* pat_cp, const int64_t* pat_ptr, const int32_t* pat_kind, const int32_t* pat_arg,
                       int64_t n_pat, int64_t cp_total) {
  if (n_pat < 0 || cp_total < 0) return kVmSizes;
  if (n_pat == 0) return kVmValid;
  if (!pat_cp || !pat_ptr || !pat_kind || !pat_arg) return kVmNull;
  if (pat_ptr[0] != 0) return kVmPtr;
  for (int64_t p = 0; p < n_pat; ++p)
    if (pat_ptr[p + 1] < pat_ptr[p] || pat_ptr[p + 1] > cp_total) return kVmPtr;
  if (pat_ptr[n_pat] != cp_total) return kVmPtr;
  for (int64_t p = 0; p < n_pat; ++p) {
    const int64_t b = pat_ptr[p], m = pat_ptr[p + 1] - b;
    if (m < 1 || m > kVmMaxLen) return kVmLength;
    const int kind = pat_kind[p], arg = pat_arg[p];
    if (kind != kVmWildcard && kind != kVmFuzzy) return kVmKindArg;
    if (kind == kVmFuzzy ? (arg < 1 || arg > kVmMaxEdits) : arg != 0) return kVmKindArg;
    for (int64_t j = 0; j < m; ++j) {
      const uint32_t c = pat_cp[b + j];
      if (c > kVmMaxCodePoint && (kind == kVmFuzzy || (c != kVmAnyOne && c != kVmAnyRun))) return kVmValue;
    }
    if (!vm_pattern_info(pat_cp + b, (int)m, kind, arg).ok) return kVmLiteral;
  }
  return kVmValid;
}

// The vocabulary of a create call; cp_len [n_terms] (nullable) receives the code-point counts.
inline int vm_validate_vocab(const unsigned char* blob, const int64_t* offsets, int64_t n_terms, int32_t* cp_len) {
  if (n_terms < 0) return kVmSizes;
  if (n_terms > 0x7fffffffLL) return kVmTerms;
  if (!offsets || offsets[0] != 0) return offsets ? kVmOffsets : kVmNull;
  for (int64_t t = 0; t < n_terms; ++t)
    if (offsets[t + 1] < offsets[t]) return kVmOffsets;
  if (offsets[n_terms] > 0 && !blob) return kVmNull;
  for (int64_t t = 0; t < n_terms; ++t) {
    if (!vm_utf8_ok(blob, offsets[t], offsets[t + 1])) return kVmUtf8;
    if (cp_len) cp_len[t] = vm_cp_count(blob, offsets[t], offsets[t + 1]);
  }
  return kVmValid;
}

}  // namespace amdr

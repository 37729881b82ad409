// The rules of amdr_term_scope (term_scope.hip) that are plain C++: whether a document has a posting for a term, whether
// it satisfies a group and a constraint, which list drives a constraint and how long it is, and the host validation of the
// operands.  The kernels and the host check (check_term_scope.cpp, which applies the same functions tile by tile on the
// CPU) share this one source, in the style of rows_compact.hpp and bm25_*_rule.hpp.
//
// The rule.  A constraint is a list of groups; a group is a non-empty list of term ids with a kind.  A document
// SATISFIES a group when it has a posting for EVERY term of the group: a conjunction — ("consequential", "damages") names
// the documents that hold both words, anywhere.  The words in that order are a phrase: amdr_phrase_lists (phrase_rule.hpp)
// resolves it into an ascending document list of its own, a VIRTUAL posting list, and the term id n_terms + p names the
// p-th such list of a call (TsIndex::x_ptr / x_doc / n_x), wherever a term id may stand.  The id -1 (and any id outside
// [0, n_terms + n_x)) is a token the vocabulary does not hold: present in no document, never dereferenced.
// A document QUALIFIES when it satisfies every MUST group, at least one ANY group (or there is none), no NOT group, and
// lies in the constraint's base scope (an ascending row list), if it has one.
//
// The driver.  The candidates of a constraint are the shortest of { its base scope's rows, the posting list of each term
// of its MUST groups }, ties -> the first in that order.  A term outside the vocabulary among the MUST terms makes the
// constraint empty without reading anything.  With no MUST term and no base scope the candidates are the documents
// 0 .. n_docs-1 themselves (the iota form): work is then proportional to the corpus.  Every driver is ascending, hence
// every output is.  Work per constraint: |driver| x the sum of log2(df) over the OTHER terms (and log2 |base| when the
// base is not the driver).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define AMDR_TS_HD __host__ __device__
#else
#define AMDR_TS_HD
#endif

namespace amdr {

enum TsKind { kTsMust = 0, kTsAny = 1, kTsNot = 2 };
enum TsStatus {
  kTsOk = 0,
  kTsCandOverflow = 1,  // the driver is longer than cand_max: the constraint's scope is left empty
  kTsRowsOverflow = 2,  // rows of the constraint lie at positions >= rows_cap and were dropped
};
constexpr int kTsTile = 1024;  // candidates per block

// The resident postings (BmIndex): term t's documents are post_doc[term_ptr[t] .. term_ptr[t + 1]), strictly ascending.
// The virtual lists of the call: term n_terms + p, p < n_x, has the documents x_doc[x_ptr[p] .. x_ptr[p + 1]), strictly
// ascending as well (n_x = 0, what an initialiser without them yields: none).
struct TsIndex {
  const long long* term_ptr;
  const int* post_doc;
  long n_terms, n_docs;
  const long long* x_ptr;
  const int* x_doc;
  long n_x;
};

// The constraints of a call.  Groups of constraint c: grp_ptr[c] .. grp_ptr[c + 1]; terms of group g:
// grp_terms[grp_term_ptr[g] .. grp_term_ptr[g + 1]).  cons_base[c]: the base scope of c, rows
// base_rows[base_ptr[b] .. base_ptr[b + 1]), or -1 (any value outside [0, n_base)): the whole corpus.
struct TsCons {
  const long long* grp_ptr;
  const int* grp_kind;
  const long long* grp_term_ptr;
  const int* grp_terms;
  const long long* base_ptr;
  const long long* base_rows;
  const int* cons_base;
  int n_base;
};

enum TsDriverKind { kTsDrvEmpty = 0, kTsDrvBase = 1, kTsDrvPosting = 2, kTsDrvIota = 3, kTsDrvVirtual = 4 };
struct TsDriver {
  int kind;
  int term;         // kTsDrvPosting / kTsDrvVirtual: the term whose list drives (every candidate has it), else -1
  long long begin;  // first candidate: an index into base_rows / post_doc / x_doc (0 for the iota form)
  long long len;    // the candidate count of the constraint
};

// Whether `doc` has a posting for `term`: a binary search in the term's ascending list; false for a term outside
// [0, n_terms), which is never dereferenced.
AMDR_TS_HD inline bool posting_has(const long long* term_ptr, const int* post_doc, long n_terms, int term, long long doc) {
  if (term < 0 || term >= n_terms) return false;
  long long lo = term_ptr[term], hi = term_ptr[term + 1];
  const long long end = hi;
  while (lo < hi) {  // lower_bound
    const long long mid = lo + ((hi - lo) >> 1);
    if (post_doc[mid] < doc)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < end && post_doc[lo] == doc;
}

// The list of term `t` of the index, a resident or a virtual one, as [*lo, *hi) of *docs; false: no such term.
AMDR_TS_HD inline bool ts_list_of(const TsIndex& I, int t, const int** docs, long long* lo, long long* hi) {
  if (t < 0) return false;
  if (t < I.n_terms) {
    *docs = I.post_doc, *lo = I.term_ptr[t], *hi = I.term_ptr[t + 1];
    return true;
  }
  const long p = (long)t - I.n_terms;
  if (p >= I.n_x) return false;
  *docs = I.x_doc, *lo = I.x_ptr[p], *hi = I.x_ptr[p + 1];
  return true;
}

// posting_has over the index with its virtual lists: one binary search in the list the id names.
AMDR_TS_HD inline bool posting_has(const TsIndex& I, int term, long long doc) {
  if (term < I.n_terms) return posting_has(I.term_ptr, I.post_doc, I.n_terms, term, doc);
  return posting_has(I.x_ptr, I.x_doc, I.n_x, (int)(term - I.n_terms), doc);
}

// Whether `doc` is one of the ascending rows[lo .. hi).
AMDR_TS_HD inline bool ts_rows_have(const long long* rows, long long lo, long long hi, long long doc) {
  const long long end = hi;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (rows[mid] < doc)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < end && rows[lo] == doc;
}

// The base scope of constraint c as [*lo, *hi) of base_rows; false: it has none.
AMDR_TS_HD inline bool ts_base_of(const TsCons& C, long c, long long* lo, long long* hi) {
  const int b = C.cons_base[c];
  if (b < 0 || b >= C.n_base) return false;
  *lo = C.base_ptr[b];
  *hi = C.base_ptr[b + 1];
  if (*hi < *lo) *hi = *lo;
  return true;
}

// Whether `doc` satisfies group g: a posting for every term (a repeated term counts once; no term: every document).
// known_term: a term every candidate is known to have (the driver's), not searched again; -1: none.
AMDR_TS_HD inline bool ts_group_has(const TsIndex& I, const TsCons& C, long long g, long long doc, int known_term) {
  for (long long j = C.grp_term_ptr[g]; j < C.grp_term_ptr[g + 1]; ++j) {
    const int t = C.grp_terms[j];
    if (t >= 0 && t == known_term) continue;
    if (!posting_has(I, t, doc)) return false;
  }
  return true;
}

// Whether `doc`, a candidate of constraint c under driver D, qualifies.
AMDR_TS_HD inline bool ts_qualifies(const TsIndex& I, const TsCons& C, long c, const TsDriver& D, long long doc) {
  if (doc < 0 || doc >= I.n_docs) return false;
  bool any_seen = false, any_ok = false;
  for (long long g = C.grp_ptr[c]; g < C.grp_ptr[c + 1]; ++g) {
    const int kind = C.grp_kind[g];
    if (kind == kTsAny && any_ok) continue;
    const bool has = ts_group_has(I, C, g, doc, D.term);
    if (kind == kTsMust) {
      if (!has) return false;
    } else if (kind == kTsAny) {
      any_seen = true;
      any_ok = has;
    } else if (has) {  // kTsNot
      return false;
    }
  }
  if (any_seen && !any_ok) return false;
  if (D.kind != kTsDrvBase) {
    long long lo, hi;
    if (ts_base_of(C, c, &lo, &hi) && !ts_rows_have(C.base_rows, lo, hi, doc)) return false;
  }
  return true;
}

// The driver of constraint c (see the top of this file).  Reads term_ptr of the MUST terms only.
AMDR_TS_HD inline TsDriver ts_driver(const TsIndex& I, const TsCons& C, long c) {
  TsDriver d{kTsDrvIota, -1, 0, (long long)I.n_docs};
  bool have = false;
  long long lo, hi;
  if (ts_base_of(C, c, &lo, &hi)) {
    d = TsDriver{kTsDrvBase, -1, lo, hi - lo};
    have = true;
  }
  for (long long g = C.grp_ptr[c]; g < C.grp_ptr[c + 1]; ++g) {
    if (C.grp_kind[g] != kTsMust) continue;
    for (long long j = C.grp_term_ptr[g]; j < C.grp_term_ptr[g + 1]; ++j) {
      const int t = C.grp_terms[j];
      const int* docs;
      long long p0, p1;
      if (!ts_list_of(I, t, &docs, &p0, &p1)) return TsDriver{kTsDrvEmpty, -1, 0, 0};
      const long long len = p1 - p0;
      if (!have || len < d.len) {
        d = TsDriver{t < I.n_terms ? kTsDrvPosting : kTsDrvVirtual, t, p0, len};
        have = true;
      }
    }
  }
  if (d.len < 0) d.len = 0;
  return d;
}

// Candidate i of the driver, i in [0, D.len).
AMDR_TS_HD inline long long ts_candidate(const TsIndex& I, const TsCons& C, const TsDriver& D, long long i) {
  return D.kind == kTsDrvBase      ? C.base_rows[D.begin + i]
         : D.kind == kTsDrvPosting ? (long long)I.post_doc[D.begin + i]
         : D.kind == kTsDrvVirtual ? (long long)I.x_doc[D.begin + i]
                                   : i;
}

// Tiles of kTsTile candidates that cover a driver of up to cand_max candidates (at least one: every constraint has a
// block that writes its count and its status).
AMDR_TS_HD inline long long ts_tiles(long long cand_max) {
  const long long t = (cand_max + kTsTile - 1) / kTsTile;
  return t < 1 ? 1 : t;
}

// ---- host validation of the operands (amdr_term_scope; the "_device" call takes them as they are) ------------------------
enum TsError {
  kTsValid = 0,
  kTsNull,        // a null array that the sizes say is read
  kTsSizes,       // a negative count
  kTsGrpPtr,      // grp_ptr does not start at 0, is not monotone or does not end at n_groups
  kTsTermPtr,     // grp_term_ptr does not start at 0 or is not monotone
  kTsEmptyGroup,  // a group without a term
  kTsKind,        // a kind outside 0 .. 2
  kTsBasePtr,     // base_ptr does not start at >= 0 or is not monotone
  kTsBaseRange,   // a base row outside [0, n_docs)
  kTsBaseOrder,   // base rows of one scope not strictly ascending
  kTsConsBase,    // cons_base outside [-1, n_base)
  kTsListPtr,     // x_ptr does not start at 0 or is not monotone
  kTsListRange,   // a document of a virtual list outside [0, n_docs)
  kTsListOrder,   // the documents of a virtual list not strictly ascending
};

inline const char* ts_error_text(int e) {
  switch (e) {
    case kTsNull: return "a null operand array";
    case kTsSizes: return "a negative count";
    case kTsGrpPtr: return "grp_ptr does not run monotonically from 0 to n_groups";
    case kTsTermPtr: return "grp_term_ptr does not run monotonically from 0";
    case kTsEmptyGroup: return "a group without a term";
    case kTsKind: return "a group kind outside 0 .. 2 (MUST, ANY, NOT)";
    case kTsBasePtr: return "base_ptr is negative or not monotone";
    case kTsBaseRange: return "a base row outside [0, n_docs)";
    case kTsBaseOrder: return "the rows of a base scope are not strictly ascending";
    case kTsConsBase: return "a cons_base outside [-1, n_base)";
    case kTsListPtr: return "x_ptr does not run monotonically from 0";
    case kTsListRange: return "a document of a virtual list outside [0, n_docs)";
    case kTsListOrder: return "the documents of a virtual list are not strictly ascending";
    default: return "ok";
  }
}

inline int ts_validate(const int64_t* grp_ptr, const int32_t* grp_kind, const int64_t* grp_term_ptr, const int64_t* base_ptr,
                       const int64_t* base_rows, const int32_t* cons_base, int64_t n_base, int64_t n_cons, int64_t n_groups,
                       int64_t n_docs) {
  if (n_cons < 0 || n_groups < 0 || n_base < 0) return kTsSizes;
  if (!grp_ptr || !grp_term_ptr || (n_cons > 0 && !cons_base) || (n_groups > 0 && !grp_kind) || (n_base > 0 && !base_ptr))
    return kTsNull;
  if (grp_ptr[0] != 0) return kTsGrpPtr;
  for (int64_t c = 0; c < n_cons; ++c)
    if (grp_ptr[c + 1] < grp_ptr[c]) return kTsGrpPtr;
  if (grp_ptr[n_cons] != n_groups) return kTsGrpPtr;
  if (grp_term_ptr[0] != 0) return kTsTermPtr;
  for (int64_t g = 0; g < n_groups; ++g) {
    if (grp_term_ptr[g + 1] < grp_term_ptr[g]) return kTsTermPtr;
    if (grp_term_ptr[g + 1] == grp_term_ptr[g]) return kTsEmptyGroup;
    if (grp_kind[g] < kTsMust || grp_kind[g] > kTsNot) return kTsKind;
  }
  if (n_base > 0) {
    if (base_ptr[0] < 0) return kTsBasePtr;
    for (int64_t b = 0; b < n_base; ++b)
      if (base_ptr[b + 1] < base_ptr[b]) return kTsBasePtr;
    if (base_ptr[n_base] > base_ptr[0] && !base_rows) return kTsNull;
    for (int64_t b = 0; b < n_base; ++b)
      for (int64_t j = base_ptr[b]; j < base_ptr[b + 1]; ++j) {
        if (base_rows[j] < 0 || base_rows[j] >= n_docs) return kTsBaseRange;
        if (j > base_ptr[b] && base_rows[j] <= base_rows[j - 1]) return kTsBaseOrder;
      }
  }
  for (int64_t c = 0; c < n_cons; ++c)
    if (cons_base[c] < -1 || cons_base[c] >= n_base) return kTsConsBase;
  return kTsValid;
}

// The virtual lists of amdr_term_scope_lists (n_x = 0: none, nothing is read).
inline int ts_validate_lists(const int64_t* x_ptr, const int32_t* x_doc, int64_t n_x, int64_t n_docs) {
  if (n_x < 0) return kTsSizes;
  if (n_x == 0) return kTsValid;
  if (!x_ptr) return kTsNull;
  if (x_ptr[0] != 0) return kTsListPtr;
  for (int64_t p = 0; p < n_x; ++p)
    if (x_ptr[p + 1] < x_ptr[p]) return kTsListPtr;
  if (x_ptr[n_x] > 0 && !x_doc) return kTsNull;
  for (int64_t p = 0; p < n_x; ++p)
    for (int64_t j = x_ptr[p]; j < x_ptr[p + 1]; ++j) {
      if (x_doc[j] < 0 || x_doc[j] >= n_docs) return kTsListRange;
      if (j > x_ptr[p] && x_doc[j] <= x_doc[j - 1]) return kTsListOrder;
    }
  return kTsValid;
}

}  // namespace amdr

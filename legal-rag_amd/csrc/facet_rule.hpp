// The rules of amdr_facet_counts (facet.hip) that are plain C++: what a facet field is, which bin a row's code falls into,
// the tiles of a scope, the layout of the counters, the order key of the returned list and its padding, and the host
// validation of the operands.  The kernels, the host twin and the host check (check_facets.cpp, which walks tiles and bins
// as the kernels do on the CPU) share this one source, in the style of marks_rule.hpp and union_rule.hpp.
//
// The rule.  A facet field of a chunk list is a code column codes i32 [n_rows]: a value in [0, n_codes) names a field
// value, any other value (-1 the canonical one) says the row has none.  For one constraint with qualifying rows R — its
// slice of a scope table — and one field:
//   total      |R|
//   missing    #{r in R : codes[r] outside [0, n_codes)}
//   count[c]   #{r in R : codes[r] == c}
//   distinct   #{c : count[c] > 0}
//   the list   the first `top` codes with count > 0 by (count descending, code ascending); slots past `distinct` hold
//              code -1 and count 0.  1 <= top <= kFcMaxTop.
// A row outside [0, n_rows) is never dereferenced and counted nowhere, `total` included (the host twin refuses it).
#pragma once
#include "term_scope_rule.hpp"

namespace amdr {

constexpr int kFcTile = 2048;     // rows of a scope per block of the count pass (AMDR_FACET_TILE_ROWS)
constexpr int kFcBins = 4096;     // the widest field a block bins in LDS (AMDR_FACET_LDS_BINS): 16 KiB of int32
constexpr int kFcMaxTop = 64;     // AMDR_FACET_MAX_TOP
constexpr int kFcMaxFields = 8;
constexpr int kFcThreads = 256;   // threads of a block of the count pass
constexpr long long kFcMaxRows = 1LL << 31;  // n_rows and every n_codes stay below: codes are i32, counters int32
static_assert(kFcTile % kFcThreads == 0, "a thread takes whole strides of its tile");

// The blocks of a launch stand in the grid's x, and a dispatch counts its work-items in 32 bits (union_rule.hpp).
constexpr long long kFcMaxCells = (1LL << 32) / kFcThreads - 1;

// Tiles of kFcTile rows that cover the longest scope (at least one).  A strictly ascending scope inside [0, n_rows) has
// at most n_rows rows, so rows_max counts only up to there: a counter then stays below 2^31.
AMDR_TS_HD inline long long fc_rows_max(long long rows_max, long long n_rows) { return rows_max < n_rows ? rows_max : n_rows; }
AMDR_TS_HD inline long long fc_tiles(long long rows_max, long long n_rows) {
  const long long t = (fc_rows_max(rows_max, n_rows) + kFcTile - 1) / kFcTile;
  return t < 1 ? 1 : t;
}
// Whether n_cons x tiles cells fit one launch; *cells is set when they do.
AMDR_TS_HD inline bool fc_cells(long long n_cons, long long tiles, long long* cells) {
  if (n_cons < 0 || tiles < 1 || n_cons > kFcMaxCells / tiles) return false;
  *cells = n_cons * tiles;
  return true;
}

// The part [*lo, *hi) of a scope of `len` rows that tile `tile` reads; false: the tile starts past the scope's end (or
// the scope table breaks its promise and names a negative length) and its block leaves at once.
AMDR_TS_HD inline bool fc_tile_range(long long len, long long rows_max, long long tile, long long* lo, long long* hi) {
  if (len > rows_max) len = rows_max;
  const long long t0 = tile * kFcTile;
  if (t0 >= len) return false;
  *lo = t0;
  *hi = t0 + kFcTile < len ? t0 + kFcTile : len;
  return true;
}

// Whether the table's row may be dereferenced, and the bin of its code: the code itself, or n_codes — the bin of `missing`.
AMDR_TS_HD inline bool fc_row_ok(long long row, long long n_rows) { return row >= 0 && row < n_rows; }
AMDR_TS_HD inline long long fc_bin(int code, long long n_codes) { return code >= 0 && code < n_codes ? (long long)code : n_codes; }
// Whether a block bins the field in LDS (kFcBins + 1 counters, the last for `missing`) or adds straight to global memory.
AMDR_TS_HD inline bool fc_in_lds(long long n_codes) { return n_codes <= kFcBins; }

// The counters of a call: int32 [n_cons][stride], constraint p's row of field f at p * stride + off[f], n_codes[f] + 1 wide.
struct FcFields {
  long long n_codes[kFcMaxFields];
  long long off[kFcMaxFields];
  long long stride;
  int n_fields;
};
// false: n_fields or an n_codes out of range
inline bool fc_fields(int n_fields, const int64_t* n_codes, FcFields* F) {
  if (n_fields < 1 || n_fields > kFcMaxFields || !n_codes) return false;
  F->n_fields = n_fields, F->stride = 0;
  for (int f = 0; f < kFcMaxFields; ++f) F->n_codes[f] = 0, F->off[f] = 0;
  for (int f = 0; f < n_fields; ++f) {
    if (n_codes[f] < 0 || n_codes[f] >= kFcMaxRows) return false;
    F->n_codes[f] = n_codes[f], F->off[f] = F->stride;
    F->stride += n_codes[f] + 1;
  }
  return true;
}
// The workspace in bytes; false when it would not fit 2^62.
inline bool fc_work_bytes(long long n_cons, const FcFields& F, long long* bytes) {
  if (n_cons < 0) return false;
  if (n_cons > 0 && F.stride > (1LL << 60) / n_cons) return false;
  *bytes = n_cons * F.stride * 4;
  return true;
}

// The order key of a code with count > 0: greater is better — count descending, then code ascending.  The packing of
// topk.hpp's C32 (score word | ~id), so the kernel ranks with the selectors there; 0 is their padding and never a key.
AMDR_TS_HD inline unsigned long long fc_key(int count, long long code) {
  return ((unsigned long long)(unsigned)count << 32) | (unsigned long long)(0xffffffffu - (unsigned)code);
}
AMDR_TS_HD inline int fc_key_code(unsigned long long key) { return (int)(0xffffffffu - (unsigned)key); }
AMDR_TS_HD inline long long fc_key_count(unsigned long long key) { return (long long)(key >> 32); }
// Slot j of a list of `kept` keys, best first: the code and the count, or the padding.
AMDR_TS_HD inline int fc_slot_code(const unsigned long long* keys, int kept, int j) { return j < kept ? fc_key_code(keys[j]) : -1; }
AMDR_TS_HD inline long long fc_slot_count(const unsigned long long* keys, int kept, int j) {
  return j < kept ? fc_key_count(keys[j]) : 0;
}

// ---- argument and host validation -----------------------------------------------------------------------------------------
enum FcError {
  kFcValid = 0,
  kFcNull,     // a null array that the sizes say is read or written
  kFcSizes,    // a negative size, n_rows >= 2^31, n_fields / n_codes / top out of range, too many cells
  kFcPtr,      // scope_ptr does not start at 0 or is not monotone
  kFcRowsMax,  // a scope longer than rows_max
  kFcRows,     // rows not strictly ascending inside a scope, or outside [0, n_rows)
};

inline const char* fc_error_text(int e) {
  switch (e) {
    case kFcNull: return "a null operand or output array";
    case kFcSizes: return "a size out of range (negative, n_rows >= 2^31, n_fields outside 1 .. 8, an n_codes outside [0, 2^31), "
                          "top outside 1 .. 64, or more cells than one launch takes)";
    case kFcPtr: return "scope_ptr does not run monotonically from 0";
    case kFcRowsMax: return "a scope is longer than rows_max";
    case kFcRows: return "rows are not strictly ascending inside [0, n_rows)";
    default: return "ok";
  }
}

// What both entry points refuse before anything is enqueued: the sizes, and the arrays the sizes say are touched.
// *F and *cells are set when the arguments are valid.
inline int fc_check_args(const void* scope_ptr, const void* rows, int64_t n_cons, int64_t rows_max, const void* codes,
                         int64_t n_rows, int32_t n_fields, const int64_t* n_codes, int32_t top, const void* out_total,
                         const void* out_missing, const void* out_distinct, const void* out_code, const void* out_count,
                         FcFields* F, long long* cells) {
  if (n_cons < 0 || rows_max < 0 || n_rows < 0 || n_rows >= kFcMaxRows) return kFcSizes;
  if (top < 1 || top > kFcMaxTop) return kFcSizes;
  if (!n_codes) return kFcNull;
  if (!fc_fields(n_fields, n_codes, F)) return kFcSizes;
  if (!fc_cells(n_cons, fc_tiles(rows_max, n_rows), cells)) return kFcSizes;
  if (n_cons > kFcMaxCells / n_fields) return kFcSizes;  // (the select pass: one block per constraint and field)
  if (!scope_ptr) return kFcNull;
  if (n_cons > 0 && !(out_total && out_missing && out_distinct && out_code && out_count)) return kFcNull;
  if (n_cons > 0 && rows_max > 0 && (!rows || (n_rows > 0 && !codes))) return kFcNull;
  return kFcValid;
}

// The contents of a host table (amdr_facet_counts; the "_device" call takes them as they are).
inline int fc_validate(const int64_t* scope_ptr, const int64_t* rows, int64_t n_cons, int64_t rows_max, int64_t n_rows) {
  if (!scope_ptr) return kFcNull;
  if (scope_ptr[0] != 0) return kFcPtr;
  for (int64_t p = 0; p < n_cons; ++p) {
    if (scope_ptr[p + 1] < scope_ptr[p]) return kFcPtr;
    if (scope_ptr[p + 1] - scope_ptr[p] > rows_max) return kFcRowsMax;
  }
  if (scope_ptr[n_cons] > 0 && !rows) return kFcNull;
  for (int64_t p = 0; p < n_cons; ++p)
    for (int64_t i = scope_ptr[p]; i < scope_ptr[p + 1]; ++i) {
      if (!fc_row_ok(rows[i], n_rows)) return kFcRows;
      if (i > scope_ptr[p] && rows[i] <= rows[i - 1]) return kFcRows;
    }
  return kFcValid;
}

}  // namespace amdr

// The rules of amdr_union_lists (union_lists.hip) that are plain C++: what a union item is, which part of a posting list
// lies in a tile of documents, where a document's bit stands in the tile's bitmap, how a word of that bitmap becomes
// documents, the clamp of a list pointer, and the host validation of the operands.  The kernels, the host twin and the
// host check (check_union_lists.cpp, which applies the same functions cell by cell and word by word on the CPU) share this
// one source, in the style of phrase_rule.hpp and near_rule.hpp.
//
// The rule.  A union item is a list of M >= 0 term ids.  Its list is the strictly ascending set of the documents that
// have a posting for AT LEAST ONE of them: the root expander (sell! = sell, seller, seller's, selling, sells) and the
// alternatives of a conjunction (buyer OR purchaser) are both this.  An id outside [0, n_terms) names a token present in
// no document: it contributes nothing and is never dereferenced.  M = 0, or every id unknown, gives an empty list.  A
// repeated id is harmless.
//
// The tile is a DOCUMENT RANGE.  A phrase has a driver — one ascending list the answer is a subset of — and tiles its
// candidates.  A union has none: its output must be ascending across DIFFERENT lists, so a cell is (item p, tile y) with
// tile y the documents [y * kUnTile, (y + 1) * kUnTile), and what lies inside a cell is a bitmap of kUnTile bits, one per
// document: setting a bit is idempotent and independent of order, so the lists need no merge and a document two terms
// share is counted once.  The part of term t's list inside the tile is found by two lower-bound searches (un_tile_range).
// Work per cell: M x 2 searches of log2(df) steps, plus the postings inside the tile.
#pragma once
#include "term_scope_rule.hpp"

namespace amdr {

constexpr int kUnTile = 32768;              // documents per tile: a 4 KiB bitmap
constexpr int kUnWords = kUnTile / 32;      // 32-bit words of a tile's bitmap
constexpr int kUnThreads = 256;             // threads of a block
constexpr int kUnPer = kUnWords / kUnThreads;  // consecutive words a thread of the write pass expands
static_assert(kUnTile % 32 == 0 && kUnWords % kUnThreads == 0 && kUnPer == 4, "a thread reads its words as one 16-byte load");

// The cells of a launch are the blocks of a one-dimensional grid of kUnThreads threads each, and a dispatch counts its
// work-items in 32 bits: this many cells at most (far below the 2^31 an index of blocks could hold).
constexpr long long kUnMaxCells = (1LL << 32) / kUnThreads - 1;

// The resident postings (BmIndex): term t's documents are post_doc[term_ptr[t] .. term_ptr[t + 1]), strictly ascending.
struct UnIndex {
  const long long* term_ptr;
  const int* post_doc;
  long n_terms, n_docs;
};

// Tiles of kUnTile documents that cover n_docs documents (at least one: every item has a block that writes its entry of
// list_ptr and its status).
AMDR_TS_HD inline long long un_tiles(long long n_docs) {
  const long long t = (n_docs + kUnTile - 1) / kUnTile;
  return t < 1 ? 1 : t;
}

// Whether n_items x tiles(n_docs) cells fit one launch; *cells is set when they do.
AMDR_TS_HD inline bool un_cells(long long n_items, long long n_docs, long long* cells) {
  const long long tiles = un_tiles(n_docs);
  if (n_items < 0 || n_docs < 0) return false;
  if (n_items > kUnMaxCells / tiles) return false;
  *cells = n_items * tiles;
  return true;
}

// The first index in [lo, hi) of the ascending docs whose document is >= doc; hi when there is none.
AMDR_TS_HD inline long long un_lower_bound(const int* docs, long long lo, long long hi, long long doc) {
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (docs[mid] < doc)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// The part [*lo, *hi) of term t's posting list whose documents lie in tile `tile`.  false (nothing is read): a term
// outside [0, n_terms).  Two searches, the second inside what the first left.
AMDR_TS_HD inline bool un_tile_range(const UnIndex& I, int t, long long tile, long long* lo, long long* hi) {
  if (t < 0 || t >= I.n_terms) return false;
  const long long p0 = I.term_ptr[t], p1 = I.term_ptr[t + 1];
  const long long base = tile * kUnTile;
  *lo = un_lower_bound(I.post_doc, p0, p1, base);
  *hi = un_lower_bound(I.post_doc, *lo, p1, base + kUnTile);
  return true;
}

// Where document `doc` of tile `tile` stands in the tile's bitmap: the word and the bit inside it.
AMDR_TS_HD inline int un_bit_word(long long doc, long long tile) { return (int)((doc - tile * kUnTile) >> 5); }
AMDR_TS_HD inline unsigned un_bit_mask(long long doc) { return 1u << (unsigned)(doc & 31); }

// The set bits of a word.
AMDR_TS_HD inline int un_popcount(unsigned w) { return __builtin_popcount(w); }

// Word w (of kUnWords) of tile `tile` expanded into documents, ascending: bit b is document tile * kUnTile + w * 32 + b,
// and the r-th set bit goes to docs[at + r] — unless that position is >= rows_cap: it is dropped.  Returns the number of
// set bits, written or not.
AMDR_TS_HD inline int un_expand_word(unsigned bits, long long tile, int w, long long at, long long rows_cap, int* docs) {
  const long long first = tile * kUnTile + (long long)w * 32;
  int r = 0;
  for (; bits; bits &= bits - 1, ++r) {
    const int b = __builtin_ctz(bits);  // the lowest set bit's position
    if (at + r >= 0 && at + r < rows_cap) docs[at + r] = (int)(first + b);
  }
  return r;
}

// A list pointer clamped to the capacity of the documents array.
AMDR_TS_HD inline long long un_clamp(long long v, long long rows_cap) { return v < rows_cap ? v : rows_cap; }

// The status of an item whose list is [begin, end) of the unclamped array: rows dropped, or none.
AMDR_TS_HD inline int un_status(long long begin, long long end, long long rows_cap) {
  return end > begin && end > rows_cap ? (int)kTsRowsOverflow : (int)kTsOk;
}

// ---- host validation ------------------------------------------------------------------------------------------------------
enum UnError {
  kUnValid = 0,
  kUnNull,   // a null array that the sizes say is read
  kUnSizes,  // a negative count
  kUnPtr,    // item_ptr does not start at 0 or is not monotone
};

inline const char* un_error_text(int e) {
  switch (e) {
    case kUnNull: return "a null operand array";
    case kUnSizes: return "a negative count";
    case kUnPtr: return "item_ptr does not run monotonically from 0";
    default: return "ok";
  }
}

// The items of a call (amdr_union_lists; the "_device" call takes them as they are).  Any id may stand in an item.
inline int un_validate(const int64_t* item_ptr, const int32_t* item_terms, int64_t n_items) {
  if (n_items < 0) return kUnSizes;
  if (!item_ptr) return kUnNull;
  if (item_ptr[0] != 0) return kUnPtr;
  for (int64_t p = 0; p < n_items; ++p)
    if (item_ptr[p + 1] < item_ptr[p]) return kUnPtr;
  if (item_ptr[n_items] > 0 && !item_terms) return kUnNull;
  return kUnValid;
}

}  // namespace amdr

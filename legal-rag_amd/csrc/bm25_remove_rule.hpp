// The rules of amdr_bm25_remove (bm25_update.hip) that are plain C++: the host validation of the call's own arrays, the new id of
// an old document, the rank of an old posting among the surviving ones, a term's surviving count and where a surviving
// posting goes.  The kernels and the host check (check_bm25_remove.cpp, which compacts on the CPU with the same
// functions) share this one source, in the style of bm25_add_rule.hpp.  The tile (here kBmTile consecutive OLD postings)
// and the term search are those of bm25_tile_rule.hpp.
#pragma once
#include <cstdint>
#include <memory>
#include <new>

#include "bm25_tile_rule.hpp"

namespace amdr {

static_assert(kBmTile <= 65536, "a posting's rank inside its tile is kept in 16 bits");

// Why a remove is refused (0 = it is accepted).  Reads the call's arrays only: O(V + n_remove).
enum BmRemoveError {
  kBmRmOk = 0,
  kBmRmNull,        // a null array the sizes say is read
  kBmRmSizes,       // n_remove < 0 or >= n_docs (an index keeps a document), n_terms_new outside [0, n_terms], or a
                    // null map with n_terms_new != n_terms
  kBmRmIdRange,     // a remove id outside [0, n_docs)
  kBmRmIdOrder,     // remove ids not strictly ascending
  kBmRmAvgdl,       // avgdl not finite or not positive
  kBmRmIdf,         // an idf that is not finite
  kBmRmMapRange,    // a term_map value below -1 or >= n_terms_new
  kBmRmMapTwice,    // two old terms on one new id
  kBmRmMapMissing,  // a new id no old term maps to
  kBmRmNoMem,       // no host memory for the map check's marks
};

inline const char* bm_rm_error_text(int e) {
  switch (e) {
    case kBmRmNull: return "null array";
    case kBmRmSizes: return "bad sizes (n_remove < 0 or >= n_docs, n_terms_new outside [0, n_terms], or no map and n_terms_new != n_terms)";
    case kBmRmIdRange: return "a remove id is outside [0, n_docs)";
    case kBmRmIdOrder: return "remove ids are not strictly ascending";
    case kBmRmAvgdl: return "avgdl is not a positive finite number";
    case kBmRmIdf: return "an idf is not finite";
    case kBmRmMapRange: return "a term_map value is below -1 or not below n_terms_new";
    case kBmRmMapTwice: return "two terms are mapped to one new id";
    case kBmRmMapMissing: return "a new term id has no old term";
    case kBmRmNoMem: return "no host memory for the map check";
    default: return "ok";
  }
}

// n_remove > 0 is the caller's to establish (n_remove == 0 reads nothing).
inline int bm_rm_validate(const int64_t* remove_ids, int64_t n_remove, const int32_t* term_map, int64_t n_terms_new,
                          const double* idf, double avgdl, int64_t n_terms_old, int64_t n_docs_old) {
  if (n_remove < 0 || n_remove >= n_docs_old || n_terms_new < 0 || n_terms_new > n_terms_old) return kBmRmSizes;
  if (!term_map && n_terms_new != n_terms_old) return kBmRmSizes;
  if (!remove_ids || (n_terms_new > 0 && !idf)) return kBmRmNull;
  for (int64_t i = 0; i < n_remove; ++i) {
    if (remove_ids[i] < 0 || remove_ids[i] >= n_docs_old) return kBmRmIdRange;
    if (i > 0 && remove_ids[i] <= remove_ids[i - 1]) return kBmRmIdOrder;
  }
  if (!bm_avgdl_ok(avgdl)) return kBmRmAvgdl;
  if (!bm_idf_all_finite(idf, n_terms_new)) return kBmRmIdf;
  if (term_map) {
    std::unique_ptr<unsigned char[]> seen(new (std::nothrow) unsigned char[(size_t)n_terms_new + 1]());
    if (!seen) return kBmRmNoMem;
    int64_t mapped = 0;
    for (int64_t t = 0; t < n_terms_old; ++t) {
      const int64_t m = term_map[t];
      if (m < -1 || m >= n_terms_new) return kBmRmMapRange;
      if (m < 0) continue;
      if (seen[(size_t)m]) return kBmRmMapTwice;
      seen[(size_t)m] = 1;
      ++mapped;
    }
    if (mapped != n_terms_new) return kBmRmMapMissing;
  }
  return kBmRmOk;
}

// The new id of old document d, or -1 when it is removed: d minus the number of remove ids below it (a lower bound in the
// strictly ascending list), so the survivors are 0 .. n-1 in their old order.
AMDR_HD inline int bm_rm_doc_new(const long long* remove_ids, long n_remove, long d) {
  long lo = 0, hi = n_remove;  // first index with remove_ids[index] >= d
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if (remove_ids[mid] < d)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo < n_remove && remove_ids[lo] == d) return -1;
  return (int)(d - lo);
}

// The number of surviving postings before old posting q, q in [0, nnz_old]: the base of q's tile (the exclusive scan of
// the tile counts, tile_base[n_tiles] being the total) plus q's rank inside the tile.
AMDR_HD inline long long bm_rm_rank(long long q, long long nnz_old, const long long* tile_base, const unsigned short* tile_rank) {
  if (q >= nnz_old) return tile_base[(nnz_old + kBmTile - 1) / kBmTile];
  return tile_base[q / kBmTile] + (long long)tile_rank[q];
}

// The new id of old term t (a null map is the identity).
AMDR_HD inline long bm_rm_term_new(const int* term_map, long t) { return term_map ? (long)term_map[t] : t; }

// Old term t's part in the new term table: rank_at[t] = the rank of its first old posting (thread t of n_terms_old + 1
// writes it; t = n_terms_old gives the total), and for t < n_terms_old the surviving count goes to df_new[new id].  A
// term mapped to -1 that still has a surviving posting raises *bad (every writer stores the same 1).
AMDR_HD inline void bm_rm_term_entry(long t, long n_terms_old, const long long* old_ptr, long long nnz_old,
                                     const long long* tile_base, const unsigned short* tile_rank, const int* term_map,
                                     long long* rank_at, long long* df_new, int* bad) {
  const long long r0 = bm_rm_rank(old_ptr[t], nnz_old, tile_base, tile_rank);
  rank_at[t] = r0;
  if (t >= n_terms_old) return;
  const long long cnt = bm_rm_rank(old_ptr[t + 1], nnz_old, tile_base, tile_rank) - r0;
  const long m = bm_rm_term_new(term_map, t);
  if (m >= 0)
    df_new[m] = cnt;
  else if (cnt > 0)
    *bad = 1;
}

// Where surviving old posting p of old term t goes: behind the survivors of its list that precede it, in the list of the
// term's new id.  -1 for a term that has no new id (the call fails before anything is scattered then).
AMDR_HD inline long long bm_rm_dest(long long p, long t, long long nnz_old, const long long* tile_base,
                                    const unsigned short* tile_rank, const long long* rank_at, const long long* new_ptr,
                                    const int* term_map) {
  const long m = bm_rm_term_new(term_map, t);
  if (m < 0) return -1;
  return new_ptr[m] + (bm_rm_rank(p, nnz_old, tile_base, tile_rank) - rank_at[t]);
}

}  // namespace amdr

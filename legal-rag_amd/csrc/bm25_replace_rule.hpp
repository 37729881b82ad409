// The rules of amdr_bm25_replace (bm25_update.hip) that are plain C++: the host validation of the call's own arrays and the
// inverse term map, the document map, a new term's document frequency and where a posting of either source goes.  The
// kernels and the host check (check_bm25_replace.cpp, which merges on the CPU with the same functions) share this one
// source, in the style of bm25_remove_rule.hpp, whose tile ranks (bm_rm_rank) and term map (bm_rm_term_new) are used as
// they are.
//
// The merge.  Documents keep their ids, so the list of new term u is the merge BY DOCUMENT ID of two ascending lists
// without a common document: the surviving postings of its old term t (documents not in replace_ids) and the add's
// postings of u, whose local document i is document replace_ids[i] — ascending in i, so the add's list is ascending in
// the document too.  A posting's place is its rank in its own list plus the number of postings of the OTHER list with a
// smaller document: one binary search (in the add's list, or in the old list followed by the tile rank tables of the
// remove).  Every place is a sum of counts: no atomics, the result is deterministic.
#pragma once
#include <cstdint>

#include "bm25_remove_rule.hpp"

namespace amdr {

// Why a replace is refused (0 = it is accepted).  Reads the call's arrays only: O(V + n_rep + added postings).
enum BmReplaceError {
  kBmRpOk = 0,
  kBmRpNull,      // a null array the sizes say is read
  kBmRpSizes,     // n_rep < 0 or > n_docs, n_terms_new outside [0, 2^31), or a null map with n_terms_new < n_terms
  kBmRpIdRange,   // a replace id outside [0, n_docs)
  kBmRpIdOrder,   // replace ids not strictly ascending
  kBmRpAvgdl,     // avgdl not finite or not positive
  kBmRpIdf,       // an idf that is not finite
  kBmRpMapRange,  // a term_map value below -1 or >= n_terms_new
  kBmRpMapTwice,  // two old terms on one new id
  kBmRpPtrStart,  // term_ptr_add[0] != 0
  kBmRpPtrOrder,  // term_ptr_add not monotone
  kBmRpDocRange,  // a post_doc_add outside [0, n_rep)
  kBmRpDocOrder,  // postings of one term not strictly ascending
};

inline const char* bm_rp_error_text(int e) {
  switch (e) {
    case kBmRpNull: return "null array";
    case kBmRpSizes: return "bad sizes (n_rep < 0 or > n_docs, n_terms_new outside [0, 2^31), or no map and n_terms_new < n_terms)";
    case kBmRpIdRange: return "a replace id is outside [0, n_docs)";
    case kBmRpIdOrder: return "replace ids are not strictly ascending";
    case kBmRpAvgdl: return "avgdl is not a positive finite number";
    case kBmRpIdf: return "an idf is not finite";
    case kBmRpMapRange: return "a term_map value is below -1 or not below n_terms_new";
    case kBmRpMapTwice: return "two terms are mapped to one new id";
    case kBmRpPtrStart: return "term_ptr_add[0] != 0";
    case kBmRpPtrOrder: return "term_ptr_add not monotone";
    case kBmRpDocRange: return "a posting's document is outside [0, n_rep)";
    case kBmRpDocOrder: return "postings of a term are not strictly ascending";
    default: return "ok";
  }
}

// n_rep > 0 is the caller's to establish (n_rep == 0 reads nothing).  On success inv[n_terms_new] (the caller's array) is
// the inverse of the term map: the old term of every new id, or -1 for a NEW term, whose list comes from the add alone.
// A null map is the identity on the old terms, with the new terms behind them.
inline int bm_rp_validate(const int64_t* replace_ids, int64_t n_rep, const int64_t* term_ptr_add,
                          const int32_t* post_doc_add, const int32_t* post_tf_add, const int32_t* doc_len_add,
                          const int32_t* term_map, int64_t n_terms_new, const double* idf, double avgdl,
                          int64_t n_terms_old, int64_t n_docs_old, int32_t* inv) {
  if (n_rep < 0 || n_rep > n_docs_old || n_terms_new < 0 || n_terms_new >= (1ll << 31)) return kBmRpSizes;
  if (!term_map && n_terms_new < n_terms_old) return kBmRpSizes;
  if (!replace_ids || !term_ptr_add || !doc_len_add || (n_terms_new > 0 && (!idf || !inv))) return kBmRpNull;
  for (int64_t i = 0; i < n_rep; ++i) {
    if (replace_ids[i] < 0 || replace_ids[i] >= n_docs_old) return kBmRpIdRange;
    if (i > 0 && replace_ids[i] <= replace_ids[i - 1]) return kBmRpIdOrder;
  }
  if (!bm_avgdl_ok(avgdl)) return kBmRpAvgdl;
  if (!bm_idf_all_finite(idf, n_terms_new)) return kBmRpIdf;
  for (int64_t u = 0; u < n_terms_new; ++u) inv[u] = -1;
  for (int64_t t = 0; t < n_terms_old; ++t) {
    const int64_t m = term_map ? term_map[t] : t;
    if (m < -1 || m >= n_terms_new) return kBmRpMapRange;
    if (m < 0) continue;
    if (inv[m] >= 0) return kBmRpMapTwice;
    inv[m] = (int32_t)t;
  }
  if (term_ptr_add[0] != 0) return kBmRpPtrStart;
  for (int64_t u = 0; u < n_terms_new; ++u)
    if (term_ptr_add[u + 1] < term_ptr_add[u]) return kBmRpPtrOrder;
  if (term_ptr_add[n_terms_new] > 0 && (!post_doc_add || !post_tf_add)) return kBmRpNull;
  for (int64_t u = 0; u < n_terms_new; ++u)
    for (int64_t p = term_ptr_add[u]; p < term_ptr_add[u + 1]; ++p) {
      if (post_doc_add[p] < 0 || post_doc_add[p] >= n_rep) return kBmRpDocRange;
      if (p > term_ptr_add[u] && post_doc_add[p] <= post_doc_add[p - 1]) return kBmRpDocOrder;
    }
  return kBmRpOk;
}

// The position of document d in replace_ids, or -1 when it stays.
AMDR_HD inline long bm_rp_local(const long long* replace_ids, long n_rep, long d) {
  long lo = 0, hi = n_rep;  // first index with replace_ids[index] >= d
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if (replace_ids[mid] < d)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < n_rep && replace_ids[lo] == d ? lo : -1;
}

// Document d afterwards: doc_keep[d] = d when its old postings stay and -1 when it is replaced (the remove's counting pass
// reads it as its document map: a posting survives where the entry is >= 0), and its length.
AMDR_HD inline void bm_rp_doc_entry(const long long* replace_ids, long n_rep, const int* doc_len_old, const int* doc_len_add,
                                    long d, int* doc_keep, int* doc_len_new) {
  const long i = bm_rp_local(replace_ids, n_rep, d);
  doc_keep[d] = i < 0 ? (int)d : -1;
  doc_len_new[d] = i < 0 ? doc_len_old[d] : doc_len_add[i];
}

// Entry e of max(n_terms_old + 1, n_terms_new) of the term pass.  As old term (e <= n_terms_old): rank_at[e] = the rank of
// its first old posting among the survivors, and a term mapped to -1 that still has a surviving posting raises *bad (every
// writer stores the same 1).  As new term (e < n_terms_new): df_new[e] = the survivors of its old term + its add postings.
AMDR_HD inline void bm_rp_term_entry(long e, long n_terms_old, long n_terms_new, const long long* old_ptr, long long nnz_old,
                                     const long long* tile_base, const unsigned short* tile_rank, const int* term_map,
                                     const int* inv, const long long* add_ptr, long long* rank_at, long long* df_new,
                                     int* bad) {
  if (e <= n_terms_old) {
    const long long r0 = bm_rm_rank(old_ptr[e], nnz_old, tile_base, tile_rank);
    rank_at[e] = r0;
    if (e < n_terms_old && bm_rm_term_new(term_map, e) < 0 &&
        bm_rm_rank(old_ptr[e + 1], nnz_old, tile_base, tile_rank) > r0)
      *bad = 1;
  }
  if (e < n_terms_new) {
    const long t = inv[e];
    long long kept = 0;
    if (t >= 0)
      kept = bm_rm_rank(old_ptr[t + 1], nnz_old, tile_base, tile_rank) - bm_rm_rank(old_ptr[t], nnz_old, tile_base, tile_rank);
    df_new[e] = kept + (add_ptr[e + 1] - add_ptr[e]);
  }
}

// The number of add postings in [a0, a1) (one term's list) whose document replace_ids[add_doc[.]] is below `doc`.
AMDR_HD inline long long bm_rp_adds_below(const int* add_doc, long long a0, long long a1, const long long* replace_ids,
                                          long long doc) {
  long long lo = a0, hi = a1;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (replace_ids[add_doc[mid]] < doc)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo - a0;
}

// The first old posting in [o0, o1) (one term's list) whose document is not below `doc`.
AMDR_HD inline long long bm_rp_old_lower(const int* old_doc, long long o0, long long o1, long long doc) {
  long long lo = o0, hi = o1;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (old_doc[mid] < doc)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// Where surviving old posting p (document doc) of old term t goes: behind the survivors of its list that precede it and
// the add postings of its new term with a smaller document.  -1 for a term that has no new id (the call fails before
// anything is scattered then).
AMDR_HD inline long long bm_rp_dest_old(long long p, int doc, long t, long long nnz_old, const long long* tile_base,
                                        const unsigned short* tile_rank, const long long* rank_at, const long long* new_ptr,
                                        const int* term_map, const long long* add_ptr, const int* add_doc,
                                        const long long* replace_ids) {
  const long u = bm_rm_term_new(term_map, t);
  if (u < 0) return -1;
  const long long a0 = add_ptr[u], a1 = add_ptr[u + 1];
  const long long adds = a0 < a1 ? bm_rp_adds_below(add_doc, a0, a1, replace_ids, doc) : 0;
  return new_ptr[u] + (bm_rm_rank(p, nnz_old, tile_base, tile_rank) - rank_at[t]) + adds;
}

// Where add posting q (document doc = replace_ids[add_doc[q]]) of new term u goes: behind the add postings of its list
// that precede it and the surviving old postings of the term's old list with a smaller document (none for a new term).
AMDR_HD inline long long bm_rp_dest_add(long long q, long long doc, long u, const int* inv, const long long* old_ptr,
                                        const int* old_doc, long long nnz_old, const long long* tile_base,
                                        const unsigned short* tile_rank, const long long* rank_at, const long long* new_ptr,
                                        const long long* add_ptr) {
  const long t = inv[u];
  long long kept = 0;
  if (t >= 0) {
    const long long lb = bm_rp_old_lower(old_doc, old_ptr[t], old_ptr[t + 1], doc);
    kept = bm_rm_rank(lb, nnz_old, tile_base, tile_rank) - rank_at[t];
  }
  return new_ptr[u] + (q - add_ptr[u]) + kept;
}

}  // namespace amdr

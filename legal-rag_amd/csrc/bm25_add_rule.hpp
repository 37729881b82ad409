// The rules of amdr_bm25_add (bm25_update.hip) that are plain C++: the host validation of an add's own arrays, the term
// table of the concatenation, and where output posting p of the merged index comes from.  The merge kernel and the host
// check (check_bm25_add.cpp, which merges on the CPU with the same functions) share this one source, in the style of
// tokenize_rule.hpp.  The tile (kBmTile consecutive OUTPUT postings per block) and the term search are those of
// bm25_tile_rule.hpp.
#pragma once
#include <cstdint>

#include "bm25_tile_rule.hpp"

namespace amdr {

// Why an add is refused (0 = it is accepted).  Reads the add's arrays only: O(V + added postings).
enum BmAddError {
  kBmAddOk = 0,
  kBmAddNull,        // a null array the sizes say is read
  kBmAddSizes,       // n_add < 0, n_terms below the handle's or >= 2^31, n_docs + n_add >= 2^31
  kBmAddAvgdl,       // avgdl not finite or not positive
  kBmAddPtrStart,    // term_ptr_add[0] != 0
  kBmAddPtrOrder,    // term_ptr_add not monotone
  kBmAddIdf,         // an idf that is not finite
  kBmAddDocRange,    // a post_doc_add outside [0, n_add)
  kBmAddDocOrder,    // postings of one term not strictly ascending
};

inline const char* bm_add_error_text(int e) {
  switch (e) {
    case kBmAddNull: return "null array";
    case kBmAddSizes: return "bad sizes (n_add < 0, n_terms below the handle's, or 2^31 documents / terms reached)";
    case kBmAddAvgdl: return "avgdl is not a positive finite number";
    case kBmAddPtrStart: return "term_ptr_add[0] != 0";
    case kBmAddPtrOrder: return "term_ptr_add not monotone";
    case kBmAddIdf: return "an idf is not finite";
    case kBmAddDocRange: return "a posting's document is outside [0, n_add)";
    case kBmAddDocOrder: return "postings of a term are not strictly ascending";
    default: return "ok";
  }
}

// n_add > 0 is the caller's to establish (n_add == 0 reads nothing and n_add < 0 is kBmAddSizes before any pointer is
// looked at).
inline int bm_add_validate(const int64_t* term_ptr_add, const int32_t* post_doc_add, const int32_t* post_tf_add,
                           const double* idf, const int32_t* doc_len_add, int64_t n_terms, int64_t n_add, double avgdl,
                           int64_t n_terms_old, int64_t n_docs_old) {
  if (n_add < 0 || n_terms < n_terms_old || n_terms >= (1ll << 31) || n_docs_old + n_add >= (1ll << 31)) return kBmAddSizes;
  if (!term_ptr_add || !doc_len_add || (n_terms > 0 && !idf)) return kBmAddNull;
  if (!bm_avgdl_ok(avgdl)) return kBmAddAvgdl;
  if (term_ptr_add[0] != 0) return kBmAddPtrStart;
  for (int64_t t = 0; t < n_terms; ++t)
    if (term_ptr_add[t + 1] < term_ptr_add[t]) return kBmAddPtrOrder;
  if (!bm_idf_all_finite(idf, n_terms)) return kBmAddIdf;
  if (term_ptr_add[n_terms] > 0 && (!post_doc_add || !post_tf_add)) return kBmAddNull;
  for (int64_t t = 0; t < n_terms; ++t)
    for (int64_t p = term_ptr_add[t]; p < term_ptr_add[t + 1]; ++p) {
      if (post_doc_add[p] < 0 || post_doc_add[p] >= n_add) return kBmAddDocRange;
      if (p > term_ptr_add[t] && post_doc_add[p] <= post_doc_add[p - 1]) return kBmAddDocOrder;
    }
  return kBmAddOk;
}

// term_ptr of the concatenated index, entry t of n_terms_new + 1: both tables are prefix sums over the same term ids, the
// old one extended by its last value over the new terms.
AMDR_HD inline long long bm_add_term_ptr(const long long* old_ptr, long n_terms_old, const long long* add_ptr, long t) {
  return old_ptr[t < n_terms_old ? t : n_terms_old] + add_ptr[t];
}

// Output posting p of term t (new_start = the term's first output position): its first old_df entries are the old
// list, the rest the add's.  Returns the source index and sets *from_add.
AMDR_HD inline long long bm_add_source(long long p, long long new_start, long t, const long long* old_ptr, long n_terms_old,
                                       const long long* add_ptr, bool* from_add) {
  const long long r = p - new_start;
  const long long o0 = t < n_terms_old ? old_ptr[t] : 0;
  const long long odf = t < n_terms_old ? old_ptr[t + 1] - o0 : 0;
  *from_add = r >= odf;
  return *from_add ? add_ptr[t] + (r - odf) : o0 + r;
}

}  // namespace amdr

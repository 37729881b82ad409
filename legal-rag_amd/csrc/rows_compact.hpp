// The rules of amdr_dense_remove and amdr_maxsim_remove (rows_compact.hip) that are plain C++: the host validation of the
// removal list, the old row a new row comes from, the walk that carries that answer along a range of new rows, and the
// segmented form (documents are removed, their token rows move), and the replace form behind them (rs_*: documents keep
// their ids and take new rows from a second, staged buffer).  The kernels and the host check (check_rows_compact.cpp,
// which compacts on the CPU with the same functions) share this one source, in the style of bm25_remove_rule.hpp.
//
// The map.  remove_ids[n_remove] is strictly ascending in [0, n); the survivors close up in their old order (the faiss
// remove_ids convention of flat indexes, as amdr_bm25_remove).  g[i] = remove_ids[i] - i is non-decreasing (the number
// of SURVIVING old rows below remove_ids[i]), so with r(j) = upper_bound(g, j) = |{i : g[i] <= j}|, new row j comes from
// old row src(j) = j + r(j): exactly r(j) removed rows lie below it.  r is non-decreasing in j, so a range of new rows
// j0, j0 + 1, ... needs one binary search (rc_removed_upto at j0) and then only steps forward (rc_walk).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define AMDR_RC_HD __host__ __device__
#else
#define AMDR_RC_HD
#endif

namespace amdr {

// Why a removal list is refused (0 = it is accepted).  Reads the list only: O(n_remove).
enum RcError {
  kRcOk = 0,
  kRcNull,     // a null list with n_remove > 0
  kRcSizes,    // n_remove < 0 or n_remove > n
  kRcIdRange,  // an id outside [0, n)
  kRcIdOrder,  // ids not strictly ascending
};

inline const char* rc_error_text(int e) {
  switch (e) {
    case kRcNull: return "null remove_ids";
    case kRcSizes: return "n_remove is negative or above the number of rows";
    case kRcIdRange: return "a remove id is outside [0, n)";
    case kRcIdOrder: return "remove ids are not strictly ascending";
    default: return "ok";
  }
}

inline int rc_validate(const int64_t* remove_ids, int64_t n_remove, int64_t n) {
  if (n_remove < 0 || n_remove > n) return kRcSizes;
  if (n_remove > 0 && !remove_ids) return kRcNull;
  for (int64_t i = 0; i < n_remove; ++i) {
    if (remove_ids[i] < 0 || remove_ids[i] >= n) return kRcIdRange;
    if (i > 0 && remove_ids[i] <= remove_ids[i - 1]) return kRcIdOrder;
  }
  return kRcOk;
}

// r(j): the number of removed rows below the old row that new row j comes from — the first index i with
// remove_ids[i] - i > j.  Defined for every j >= 0 (past the last survivor it is n_remove).
AMDR_RC_HD inline long rc_removed_upto(const long long* remove_ids, long n_remove, long long j) {
  long lo = 0, hi = n_remove;
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if (remove_ids[mid] - mid <= j)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// r(j) from r = r(j') of any earlier new row j' <= j: the linear walk of a range.
AMDR_RC_HD inline long rc_walk(const long long* remove_ids, long n_remove, long r, long long j) {
  while (r < n_remove && remove_ids[r] - r <= j) ++r;
  return r;
}

// The old row of new row j.
AMDR_RC_HD inline long long rc_src(const long long* remove_ids, long n_remove, long long j) {
  return j + rc_removed_upto(remove_ids, n_remove, j);
}

// src of `count` consecutive new rows from j0 into out[0 .. count): one search, then the walk.
AMDR_RC_HD inline void rc_src_range(const long long* remove_ids, long n_remove, long long j0, long count, long long* out) {
  if (count <= 0) return;
  long r = rc_removed_upto(remove_ids, n_remove, j0);
  out[0] = j0 + r;
  for (long i = 1; i < count; ++i) {
    r = rc_walk(remove_ids, n_remove, r, j0 + i);
    out[i] = j0 + i + r;
  }
}

// ---- the segmented form: rows grouped into documents by doc_ptr[n_docs + 1]; documents are removed --------------------
// New document j is old document s = src(j): len[j] = doc_ptr[s + 1] - doc_ptr[s] rows, the first of them old row
// start[j] = doc_ptr[s].  The new doc_ptr is the exclusive scan of len (compact.hpp).
AMDR_RC_HD inline void rc_seg_entry(const long long* doc_ptr, long long s, long long* len, long long* start) {
  *start = doc_ptr[s];
  *len = doc_ptr[s + 1] - doc_ptr[s];
}

// The new document of new row t, t in [0, new_ptr[n_docs_new]): upper_bound(new_ptr, t) - 1 (every document has a row,
// so new_ptr is strictly ascending and the answer is the one document whose range holds t).
AMDR_RC_HD inline long rc_seg_doc(const long long* new_ptr, long n_docs_new, long long t) {
  long lo = 0, hi = n_docs_new;  // the largest j in [0, n_docs_new) with new_ptr[j] <= t
  while (hi - lo > 1) {
    const long mid = lo + ((hi - lo) >> 1);
    if (new_ptr[mid] <= t)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// The document of row t from the document j of any earlier row: the walk of a range of rows.
AMDR_RC_HD inline long rc_seg_walk(const long long* new_ptr, long n_docs_new, long j, long long t) {
  while (j + 1 < n_docs_new && new_ptr[j + 1] <= t) ++j;
  return j;
}

// The old row of new row t of new document j.
AMDR_RC_HD inline long long rc_seg_src(const long long* new_ptr, const long long* start, long j, long long t) {
  return start[j] + (t - new_ptr[j]);
}

// ---- the replace form (amdr_dense_replace, amdr_maxsim_replace): documents keep their ids, their rows are exchanged -----
// replace_ids[n_rep] is strictly ascending in [0, n) (rc_validate); the new rows of replace_ids[i] are staged rows
// add_ptr[i] .. add_ptr[i + 1] of a second buffer (add_ptr[0] == 0, every document has a row).  A source row is named by
// one signed number: s >= 0 is row s of the old store, s < 0 is row ~s of the staged rows.
inline const char* rs_error_text(int e) {
  switch (e) {
    case kRcNull: return "null replace_ids";
    case kRcSizes: return "n_rep is negative or above the number of rows";
    case kRcIdRange: return "a replace id is outside [0, n)";
    case kRcIdOrder: return "replace ids are not strictly ascending";
    default: return "ok";
  }
}

// The position of document j in replace_ids, or -1 when it is not replaced.
AMDR_RC_HD inline long rs_find(const long long* replace_ids, long n_rep, long long j) {
  long lo = 0, hi = n_rep;  // lower_bound
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if (replace_ids[mid] < j)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < n_rep && replace_ids[lo] == j ? lo : -1;
}

// Document j afterwards: its length and the (signed) source row its rows start at.  The new doc_ptr is the exclusive
// scan of len, as in the remove form.
AMDR_RC_HD inline void rs_seg_entry(const long long* doc_ptr, const long long* add_ptr, const long long* replace_ids,
                                    long n_rep, long long j, long long* len, long long* start) {
  const long i = rs_find(replace_ids, n_rep, j);
  if (i < 0) {
    rc_seg_entry(doc_ptr, j, len, start);
  } else {
    *start = ~add_ptr[i];
    *len = add_ptr[i + 1] - add_ptr[i];
  }
}

// The (signed) source row of new row t of document j: rows of a document are consecutive in either source.
AMDR_RC_HD inline long long rs_seg_src(const long long* new_ptr, const long long* start, long j, long long t) {
  const long long s = start[j], off = t - new_ptr[j];
  return s >= 0 ? s + off : s - off;  // ~(~s + off)
}

}  // namespace amdr

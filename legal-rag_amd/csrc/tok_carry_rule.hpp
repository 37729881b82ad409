// The rules of the carrying updates (amdr_bm25_add_carry, amdr_bm25_remove_carry, amdr_bm25_replace_carry; the kernel is
// tok_carry_kernel in bm25_update.hip) that are plain C++: the host validation of the add's token arrays, where a document of
// the NEW stream takes its text from, how a token of the old stream is rewritten through the term map, and what is an error.
// The kernel and the host check (check_tok_carry.cpp, which carries streams on the CPU with the same functions) share this
// one source, in the style of bm25_remove_rule.hpp.  The tile (here kBmTile consecutive NEW tokens) and the search of a
// token's document in the new tok_ptr are those of bm25_tile_rule.hpp: a document is to the stream what a term is to the
// postings.
#pragma once
#include <cstdint>

#include "bm25_tile_rule.hpp"
#include "phrase_rule.hpp"

namespace amdr {

enum TokCarryMode { kTcAdd = 0, kTcRemove = 1, kTcReplace = 2 };

// The add's token arrays (amdr_bm25_add_carry, amdr_bm25_replace_carry) against the lengths of the call and the NEW term
// table: ph_validate_stream, with `tok_add` allowed to be null where the arrays hold no token.  Reads the call's arrays
// only: O(n_add + the add's tokens).  Returns a PhError.
inline int tc_validate_add(const int64_t* tok_ptr_add, const int32_t* tok_add, const int32_t* doc_len_add, int64_t n_add,
                           int64_t n_terms_new) {
  static const int32_t none = 0;  // never read: stands for the empty array
  if (n_add < 0 || n_terms_new < 0) return kPhSizes;
  if (!tok_ptr_add) return kPhNull;
  const int32_t* tok = tok_add ? tok_add : (tok_ptr_add[n_add] == 0 ? &none : nullptr);
  return ph_validate_stream(tok_ptr_add, tok, doc_len_add, n_add, n_terms_new);
}

// What one carry reads.  Every array is named with the count the rule compares an index against before it reads.
struct TcArgs {
  int mode;               // TokCarryMode
  long n_docs_new;        // documents of the new stream
  long n_docs_old;        // documents of the old stream: old_ptr[n_docs_old + 1]
  long n_add;             // documents of the add's stream (add, replace; 0 in a remove): add_ptr[n_add + 1]
  const long long* old_ptr;
  const int* old_tok;
  long long n_tok_old;    // old_tok[n_tok_old]
  const long long* add_ptr;
  const int* add_tok;
  long long n_tok_add;    // add_tok[n_tok_add]
  const int* kept_old;    // remove: kept_old[n_docs_new], the old id of survivor d (the document-map pass writes it)
  const long long* replace_ids;  // replace: replace_ids[n_add], strictly ascending
  const int* term_map;    // remove, replace: term_map[n_terms_old] or null (the identity); null in an add
  long n_terms_old, n_terms_new;
};

// Where new document d takes its text from: the document of the old stream, or (*from_add) the local document of the
// add's stream.  The caller compares the result with the source's count.
AMDR_HD inline long tc_source_doc(const TcArgs& a, long d, bool* from_add) {
  *from_add = false;
  if (a.mode == kTcAdd) {
    if (d < a.n_docs_old) return d;
    *from_add = true;
    return d - a.n_docs_old;
  }
  if (a.mode == kTcRemove) return (long)a.kept_old[d];
  long lo = 0, hi = a.n_add;  // first index with replace_ids[index] >= d
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if (a.replace_ids[mid] < (long long)d)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo < a.n_add && a.replace_ids[lo] == (long long)d) {
    *from_add = true;
    return lo;
  }
  return d;
}

// Old token t over the new term table (a null map is the identity), or -1: t outside the old table, or a token of a
// surviving document whose term has no new id.
AMDR_HD inline int tc_map_token(const int* term_map, int t, long n_terms_old, long n_terms_new) {
  if (t < 0 || (long)t >= n_terms_old) return -1;
  const int m = term_map ? term_map[t] : t;
  return (m < 0 || (long)m >= n_terms_new) ? -1 : m;
}

// Token `off` of new document d (0 <= off < the document's new length), or -1 with *bad raised: a source document outside
// its stream, a position outside the source document or the source array, a token outside its term table, or a token whose
// term is mapped to -1.  Every index is compared with its array's count before the read.  (Every writer of *bad stores the
// same 1.)
AMDR_HD inline int tc_token_at(const TcArgs& a, long d, long long off, int* bad) {
  bool from_add;
  const long s = tc_source_doc(a, d, &from_add);
  const long n_src = from_add ? a.n_add : a.n_docs_old;
  int out = -1;
  if (s >= 0 && s < n_src && off >= 0) {
    const long long* sp = from_add ? a.add_ptr : a.old_ptr;
    const long long pos = sp[s] + off, n_src_tok = from_add ? a.n_tok_add : a.n_tok_old;
    if (pos >= 0 && pos < sp[s + 1] && pos < n_src_tok) {
      const int t = (from_add ? a.add_tok : a.old_tok)[pos];
      if (from_add)
        out = (t >= 0 && (long)t < a.n_terms_new) ? t : -1;
      else
        out = tc_map_token(a.term_map, t, a.n_terms_old, a.n_terms_new);
    }
  }
  if (out < 0) *bad = 1;
  return out;
}

}  // namespace amdr

// Host check of the rules of the carrying updates (tok_carry_rule.hpp, bm25_tile_rule.hpp, compact.hpp), a program of its
// own (never part of the library):
//   check_tok_carry
// It builds corpora as one token sequence per document, edits them the three ways (an add with new terms and an empty
// document; a remove of the first, a middle and the last document under a map that drops the vanished terms and reverses
// the rest; a replace of the first, a middle and the last document with new terms under such a map) and carries the stream
// on the CPU the way the device does: the new lengths, the inverse document map written as the document-map pass writes it
// (kept_old[bm_rm_doc_new(d)] = d), the new tok_ptr by compact_scan_host, then tile by tile (host_tile_walk,
// check_bm25_common.hpp) the tile's documents by bm_tile_terms, a window of the NEW tok_ptr copied out exactly as the
// kernel's LDS window, and every token by bm_tile_term_of + tc_token_at.  The result is compared with a plain per-document
// rebuild.  Every array is a std::vector of exactly the size the call allocates, so with the host sanitizers
// (tests/test_tok_carry_rule_host.py) an access outside one is a failure.  Then every refusal of tc_validate_add is
// provoked once, and every condition that raises the device's flag once, on arrays of exact size.
// Build: c++ -std=c++17 check_tok_carry.cpp (plain host code; no HIP header is needed).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define AMDR_COMPACT_HOST_ONLY 1  // the host forms alone: this program has no device code
#include "bm25_remove_rule.hpp"
#include "check_bm25_common.hpp"
#include "compact.hpp"
#include "tok_carry_rule.hpp"

using namespace amdr;

namespace {

using Docs = std::vector<std::vector<int32_t>>;

struct Stream {
  std::vector<long long> ptr;
  std::vector<int32_t> tok;
};

Stream stream_of(const Docs& docs) {
  Stream s;
  s.ptr.assign(1, 0);
  for (const auto& d : docs) {
    s.tok.insert(s.tok.end(), d.begin(), d.end());
    s.ptr.push_back((long long)s.tok.size());
  }
  return s;
}

long long total_of(const Docs& docs) {
  long long n = 0;
  for (const auto& d : docs) n += (long long)d.size();
  return n;
}

std::vector<int32_t> random_doc(long len, long v) {
  std::vector<int32_t> d((size_t)len);
  for (auto& t : d) t = (int32_t)(rnd() % (uint32_t)v);
  return d;
}

// One edit, as the call receives it.
struct Edit {
  int mode;
  Docs add;                    // add, replace: the new documents over the NEW term table
  std::vector<long long> ids;  // remove, replace: strictly ascending
  std::vector<int> map;        // remove, replace: old term -> new id or -1 (empty: the null map)
  long v_new;
};

// What the device leaves: the new stream and the flag.
struct Carried {
  Stream s;
  int bad = 0;
  long windows_global = 0;
};

// The carry on arrays of the call's sizes.  `kept_override`, when given, stands for a corrupt inverse map (validation).
Carried carry(const Stream& old, long n_old, long v_old, const Edit& e, const std::vector<int>* kept_override = nullptr) {
  const Stream add = stream_of(e.add);
  const long n_add = (long)e.add.size();
  // the new lengths, as the index passes leave them in the new doc_len
  std::vector<int> len_new, kept_old;
  if (e.mode == kTcAdd) {
    for (long d = 0; d < n_old; ++d) len_new.push_back((int)(old.ptr[(size_t)d + 1] - old.ptr[(size_t)d]));
    for (long i = 0; i < n_add; ++i) len_new.push_back((int)e.add[(size_t)i].size());
  } else if (e.mode == kTcRemove) {
    const long n_new = n_old - (long)e.ids.size();
    len_new.assign((size_t)n_new, -1);
    kept_old.assign((size_t)n_new, -1);
    for (long d = 0; d < n_old; ++d) {  // bm25_rm_docmap_kernel, thread d
      const int nd = bm_rm_doc_new(e.ids.data(), (long)e.ids.size(), d);
      if (nd >= 0) {
        len_new.at((size_t)nd) = (int)(old.ptr[(size_t)d + 1] - old.ptr[(size_t)d]);
        kept_old.at((size_t)nd) = (int)d;
      }
    }
  } else {
    for (long d = 0; d < n_old; ++d) len_new.push_back((int)(old.ptr[(size_t)d + 1] - old.ptr[(size_t)d]));
    for (long i = 0; i < n_add; ++i) len_new.at((size_t)e.ids[(size_t)i]) = (int)e.add[(size_t)i].size();
  }
  if (kept_override) kept_old = *kept_override;
  const long n_new = (long)len_new.size();
  std::vector<long long> len64(len_new.begin(), len_new.end());  // tok_len_i64_kernel
  Carried c;
  c.s.ptr.resize((size_t)n_new + 1);
  compact_scan_host(len64.data(), n_new, c.s.ptr.data());
  const long long n_tok_new = c.s.ptr.back();
  c.s.tok.assign((size_t)n_tok_new, -7);
  TcArgs a = {};
  a.mode = e.mode;
  a.n_docs_new = n_new, a.n_docs_old = n_old, a.n_add = n_add;
  a.old_ptr = old.ptr.data(), a.old_tok = old.tok.data(), a.n_tok_old = (long long)old.tok.size();
  a.add_ptr = add.ptr.data(), a.add_tok = add.tok.data(), a.n_tok_add = (long long)add.tok.size();
  a.kept_old = kept_old.data();
  a.replace_ids = e.ids.data();
  a.term_map = e.map.empty() ? nullptr : e.map.data();
  a.n_terms_old = v_old, a.n_terms_new = e.v_new;
  if (n_tok_new == 0) return c;
  c.windows_global = host_tile_walk(c.s.ptr, n_new, [&](long long q, const HostTileWindow& w) {
    const long d = w.term_of(q);
    CHECK(c.s.ptr[(size_t)d] <= q && q < c.s.ptr[(size_t)d + 1], "token %lld put in document %ld", q, d);
    const int t = tc_token_at(a, d, q - w.start_of(d), &c.bad);
    CHECK(c.s.tok.at((size_t)q) == -7, "token %lld written twice", q);
    if (t >= 0) c.s.tok.at((size_t)q) = t;
  });
  return c;
}

// The plain per-document rebuild: the edited corpus over the new term table.
Docs rebuilt(const Docs& docs, const Edit& e) {
  auto mapped = [&](const std::vector<int32_t>& d) {
    std::vector<int32_t> out;
    for (int32_t t : d) out.push_back(e.map.empty() ? t : (int32_t)e.map[(size_t)t]);
    return out;
  };
  Docs out;
  if (e.mode == kTcAdd) {
    out = docs;
    out.insert(out.end(), e.add.begin(), e.add.end());
  } else if (e.mode == kTcRemove) {
    for (size_t d = 0; d < docs.size(); ++d)
      if (!std::binary_search(e.ids.begin(), e.ids.end(), (long long)d)) out.push_back(mapped(docs[d]));
  } else {
    for (size_t d = 0; d < docs.size(); ++d) {
      const auto it = std::lower_bound(e.ids.begin(), e.ids.end(), (long long)d);
      if (it != e.ids.end() && *it == (long long)d)
        out.push_back(e.add[(size_t)(it - e.ids.begin())]);
      else
        out.push_back(mapped(docs[d]));
    }
  }
  return out;
}

// The map a re-fit of the survivors gives: the terms the surviving documents still use, in REVERSE order (a permutation
// that is not monotone), the others dropped.  Returns the number of kept terms.
long refit_map(const Docs& docs, const std::vector<long long>& gone, long v_old, std::vector<int>* map) {
  std::vector<char> used((size_t)v_old, 0);
  for (size_t d = 0; d < docs.size(); ++d)
    if (!std::binary_search(gone.begin(), gone.end(), (long long)d))
      for (int32_t t : docs[d]) used[(size_t)t] = 1;
  long kept = 0;
  for (long t = 0; t < v_old; ++t) kept += used[(size_t)t];
  map->assign((size_t)v_old, -1);
  long next = kept;
  for (long t = 0; t < v_old; ++t)
    if (used[(size_t)t]) (*map)[(size_t)t] = (int)--next;
  return kept;
}

Edit make_edit(int mode, const Docs& docs, long v_old) {
  const long n = (long)docs.size();
  Edit e;
  e.mode = mode;
  if (mode == kTcAdd) {
    e.v_new = v_old + 3;  // new terms behind the old ones
    e.add = {random_doc(9, e.v_new), {}, random_doc(40, e.v_new), {(int32_t)(e.v_new - 1)}, random_doc(3, e.v_new)};
  } else if (mode == kTcRemove) {
    e.ids = {0, 3, n - 1};  // the first, a middle and the last document
    e.v_new = refit_map(docs, e.ids, v_old, &e.map);
  } else {
    e.ids = {0, 4, n - 1};
    const long kept = refit_map(docs, e.ids, v_old, &e.map);
    e.v_new = kept + 2;  // two new terms behind the kept ones
    e.add = {random_doc(30, e.v_new), {}, {(int32_t)(e.v_new - 1), (int32_t)(e.v_new - 2), 0}};
  }
  return e;
}

// A corpus of `lens` (document 1 is the one that is stretched), edited the three ways.  new_total > 0: document 1 grows
// until the NEW stream holds exactly that many tokens.  Document 3 alone holds the last term, so the remove drops it.
struct Expect {
  long long new_total = 0;   // exact token count of the new stream
  long span_doc = -1;        // an old document that must span at least three tiles of the new stream (-1: none)
  bool want_global = false;  // a tile's window must be searched in the table itself
};

void family(const char* what, std::vector<long> lens, long v_old, const Expect& x) {
  const char* const names[3] = {"add", "remove", "replace"};
  long long totals[3];
  long globals = 0, spans = 0;
  for (int mode = 0; mode < 3; ++mode) {
    Docs docs;
    for (size_t d = 0; d < lens.size(); ++d) docs.push_back(random_doc(lens[d], v_old - 1));
    CHECK(docs.size() >= 8, "%s: the edits name documents 0, 1, 3, 4 and n - 1", what);
    docs[3].push_back((int32_t)(v_old - 1));
    Edit e = make_edit(mode, docs, v_old);
    if (x.new_total > 0) {
      const long long have = total_of(rebuilt(docs, e));
      CHECK(have <= x.new_total, "%s/%s: %lld tokens before the stretch, %lld wanted", what, names[mode], have, x.new_total);
      const auto more = random_doc((long)(x.new_total - have), v_old - 1);
      docs[1].insert(docs[1].end(), more.begin(), more.end());
      e = make_edit(mode, docs, v_old);  // (the map of a re-fit sees the stretched document)
    }
    const Docs want_docs = rebuilt(docs, e);
    const Stream want = stream_of(want_docs), old = stream_of(docs), add = stream_of(e.add);
    if (mode != kTcRemove) {
      std::vector<int32_t> add_len;
      for (const auto& d : e.add) add_len.push_back((int32_t)d.size());
      const int bad = tc_validate_add((const int64_t*)add.ptr.data(), add.tok.data(), add_len.data(), (int64_t)e.add.size(), e.v_new);
      CHECK(bad == kPhValid, "%s/%s: a generated stream is refused: %s", what, names[mode], ph_error_text(bad));
    }
    const Carried c = carry(old, (long)docs.size(), v_old, e);
    CHECK(c.bad == 0, "%s/%s: the flag was raised", what, names[mode]);
    CHECK(c.s.ptr == want.ptr, "%s/%s: tok_ptr differs", what, names[mode]);
    CHECK(c.s.tok == want.tok, "%s/%s: tokens differ", what, names[mode]);
    if (x.new_total > 0) CHECK(c.s.ptr.back() == x.new_total, "%s/%s: %lld tokens, %lld wanted", what, names[mode], c.s.ptr.back(), x.new_total);
    if (x.span_doc >= 0) {
      const long d = mode == kTcRemove ? x.span_doc - 1 : x.span_doc;  // (document 0 is removed before it)
      const long long first = c.s.ptr[(size_t)d] / kBmTile, last = (c.s.ptr[(size_t)d + 1] - 1) / kBmTile;
      CHECK(last - first >= 2, "%s/%s: document %ld spans tiles %lld .. %lld", what, names[mode], d, first, last);
      spans += last - first >= 2;
    }
    globals += c.windows_global;
    totals[mode] = c.s.ptr.back();
  }
  if (x.want_global) CHECK(globals >= 3, "%s: %ld window(s) searched in the table itself", what, globals);
  std::printf("carry ok: %s: %zu docs, %ld terms, new streams of %lld / %lld / %lld tokens (add / remove / replace), %ld "
              "document(s) across three tiles, %ld window(s) searched in the table itself\n", what, lens.size(), v_old, totals[0],
              totals[1], totals[2], spans, globals);
}

std::vector<long> small_lens(long n) {
  std::vector<long> lens;
  for (long d = 0; d < n; ++d) lens.push_back(d % 7 == 5 ? 0 : 1 + (long)(rnd() % 23));
  return lens;
}

void validate_cases() {
  const int64_t ptr[4] = {0, 2, 2, 5}, ptr_off[4] = {1, 2, 2, 5}, ptr_down[4] = {0, 3, 2, 5}, ptr_none[4] = {0, 0, 0, 0};
  const int32_t tok[5] = {0, 6, 1, 2, 3}, tok_neg[5] = {0, 6, 1, -1, 3}, tok_big[5] = {0, 7, 1, 2, 3};
  const int32_t len[3] = {2, 0, 3}, len_other[3] = {2, 1, 2}, len_none[3] = {0, 0, 0};
  CHECK(tc_validate_add(ptr, tok, len, 3, 7) == kPhValid, "the good stream");
  CHECK(tc_validate_add(ptr_none, nullptr, len_none, 3, 7) == kPhValid, "empty documents only, tok_add null");
  CHECK(tc_validate_add(nullptr, tok, len, 3, 7) == kPhNull, "null tok_ptr_add");
  CHECK(tc_validate_add(ptr, nullptr, len, 3, 7) == kPhNull, "null tok_add with tokens");
  CHECK(tc_validate_add(ptr, tok, nullptr, 3, 7) == kPhNull, "null doc_len_add");
  CHECK(tc_validate_add(ptr, tok, len, -1, 7) == kPhSizes, "n_add < 0");
  CHECK(tc_validate_add(ptr_off, tok, len, 3, 7) == kPhDocPtr, "tok_ptr_add[0] != 0");
  CHECK(tc_validate_add(ptr_down, tok, len, 3, 7) == kPhDocPtr, "tok_ptr_add not monotone");
  CHECK(tc_validate_add(ptr, tok, len_other, 3, 7) == kPhDocLen, "lengths that disagree with doc_len_add");
  CHECK(tc_validate_add(ptr, tok_neg, len, 3, 7) == kPhToken, "a negative token");
  CHECK(tc_validate_add(ptr, tok_big, len, 3, 7) == kPhToken, "a token == n_terms_new");
  // what only the device sees, each on arrays of exact size: 4 documents over 3 terms
  const Docs docs = {{0, 1}, {2}, {1, 1, 0}, {0}};
  const Stream old = stream_of(docs);
  Edit rm;
  rm.mode = kTcRemove, rm.ids = {1}, rm.map = {1, 0, -1}, rm.v_new = 2;  // term 2 goes with document 1
  Carried c = carry(old, 4, 3, rm);
  CHECK(c.bad == 0 && c.s.tok == (std::vector<int32_t>{1, 0, 0, 0, 1, 1}), "the good remove");
  rm.map = {1, -1, 0};  // term 1 is still used by documents 0 and 2
  CHECK(carry(old, 4, 3, rm).bad == 1, "a token of a surviving document mapped to -1 raises the flag");
  rm.map = {1, 0, 2};   // (bm_rm_validate refuses this map; the device compares all the same)
  rm.ids = {3};
  CHECK(carry(old, 4, 3, rm).bad == 1, "a map value == n_terms_new raises the flag");
  rm.map = {1, 0, -1}, rm.ids = {1};
  const std::vector<int> kept_far = {0, 4, 3}, kept_neg = {0, -1, 3}, kept_short = {0, 1, 3};
  CHECK(carry(old, 4, 3, rm, &kept_far).bad == 1, "a source document == n_docs_old raises the flag without a read");
  CHECK(carry(old, 4, 3, rm, &kept_neg).bad == 1, "a negative source document raises the flag without a read");
  CHECK(carry(old, 4, 3, rm, &kept_short).bad == 1, "a position behind the source document's end raises the flag");
  Stream corrupt = old;
  corrupt.tok[3] = 3;  // a token outside the OLD table: no gather of the map
  CHECK(carry(corrupt, 4, 3, rm).bad == 1, "an old token == n_terms_old raises the flag without a gather");
  corrupt.tok[3] = -1;
  CHECK(carry(corrupt, 4, 3, rm).bad == 1, "a negative old token raises the flag without a gather");
  Edit ad;
  ad.mode = kTcAdd, ad.v_new = 4, ad.add = {{3, 0}};
  CHECK(carry(old, 4, 3, ad).bad == 0, "the good add");
  ad.add = {{4, 0}};
  CHECK(carry(old, 4, 3, ad).bad == 1, "an added token == n_terms_new raises the flag");
  Edit rp;
  rp.mode = kTcReplace, rp.ids = {1, 3}, rp.map = {1, 0, -1}, rp.v_new = 3, rp.add = {{2, 2}, {}};
  c = carry(old, 4, 3, rp);
  CHECK(c.bad == 0 && c.s.tok == (std::vector<int32_t>{1, 0, 2, 2, 0, 0, 1}), "the good replace");
  rp.map = {-1, 0, 1};
  CHECK(carry(old, 4, 3, rp).bad == 1, "a kept document's token mapped to -1 raises the flag in a replace");
  std::printf("validate ok: every refusal of tc_validate_add and every condition of the device's flag\n");
}

}  // namespace

int main() {
  const long long T = kBmTile;
  Expect x;
  x.new_total = T - 100;
  family("one tile", small_lens(40), 50, x);
  x.new_total = 2 * T - 100;
  family("two tiles", small_lens(90), 50, x);
  x.new_total = 4 * T - 100;
  family("four tiles", small_lens(300), 400, x);
  for (long long total : {T - 1, T, T + 1, 2 * T + 1}) {
    char name[64];
    std::snprintf(name, sizeof name, "exactly %lld tokens", total);
    x.new_total = total;
    family(name, small_lens(60), 30, x);
  }
  {  // a document of 5 000 tokens: it starts in the first tile and ends in the third
    std::vector<long> lens = small_lens(20);
    lens[2] = 5000;
    Expect y;
    y.span_doc = 2;
    family("a document of 5000 tokens", lens, 30, y);
  }
  {  // 2 051 empty documents between two documents of one tile: the window does not fit the LDS copy
    std::vector<long> lens = small_lens(8);
    lens.insert(lens.end(), (size_t)kBmTile + 3, 0);
    const std::vector<long> tail = small_lens(8);
    lens.insert(lens.end(), tail.begin(), tail.end());
    lens.back() = 5, lens[lens.size() - 2] = 4;
    Expect y;
    y.want_global = true;
    family("a run of 2051 empty documents", lens, 30, y);
  }
  validate_cases();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("tok carry rule ok\n");
  return 0;
}

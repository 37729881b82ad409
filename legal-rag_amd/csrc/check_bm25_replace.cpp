// Host check of the rules of amdr_bm25_replace (bm25_replace_rule.hpp, bm25_remove_rule.hpp, bm25_tile_rule.hpp,
// compact.hpp), a program of its own (never part of the library):
//   check_bm25_replace
// It builds random term-major indexes (check_bm25_common.hpp: Zipfian lists, terms without postings, totals at and around
// multiples of the tile), replaces documents by new ones — which drop old terms, keep others and bring new terms — and
// merges on the CPU the way the kernels do: the document map by bm_rp_doc_entry, tile by tile the keep flags and their
// ranks (compact_tile_scan_host), the tile bases and the new term table by compact_scan_host, every term by
// bm_rp_term_entry, then the old postings tile by tile (host_tile_walk) through bm_rp_dest_old and the add's postings tile
// by tile through bm_rp_dest_add — and compares the result with a brute-force edit: per term the surviving and the new
// (document, tf) pairs sorted by document, the terms reordered by their new ids.  Every array is a std::vector of exactly
// the size the call allocates, so with the host sanitizers (tests/test_bm25_replace_rule_host.py) an access outside one is
// a failure.  Then every refusal of bm_rp_validate is provoked once, and the device-side flag (a term mapped to -1 with a
// surviving posting) once.
// Build: c++ -std=c++17 check_bm25_replace.cpp (plain host code; no HIP header is needed).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <utility>
#include <vector>

#define AMDR_COMPACT_HOST_ONLY 1  // the host forms alone: this program has no device code
#include "bm25_replace_rule.hpp"
#include "check_bm25_common.hpp"
#include "compact.hpp"

using namespace amdr;

namespace {

// What the device computes up to the host's look at the total and the flag, on arrays of the call's sizes.
struct Counted {
  std::vector<int> doc_keep, doc_len;
  std::vector<unsigned short> tile_rank;
  std::vector<long long> tile_base, rank_at, new_ptr;
  int bad = 0;
};

Counted count_passes(const Csr& o, long v_old, long n, const std::vector<int>& len_old, const std::vector<long long>& ids,
                     const std::vector<int>& len_add, const Csr& add, long v_new, const int* map, const std::vector<int>& inv) {
  Counted c;
  const long long nnz = o.ptr.back();
  const long tiles = (long)((nnz + kBmTile - 1) / kBmTile);
  c.doc_keep.resize((size_t)n);
  c.doc_len.resize((size_t)n);
  for (long d = 0; d < n; ++d)
    bm_rp_doc_entry(ids.data(), (long)ids.size(), len_old.data(), len_add.data(), d, c.doc_keep.data(), c.doc_len.data());
  c.tile_rank.resize((size_t)nnz);
  std::vector<long long> tile_cnt((size_t)tiles);
  for (long tile = 0; tile < tiles; ++tile) {
    const long long p0 = (long long)tile * kBmTile;
    const int cnt = (int)std::min<long long>(kBmTile, nnz - p0);
    std::vector<unsigned char> keep((size_t)cnt);
    for (int i = 0; i < cnt; ++i) keep[(size_t)i] = c.doc_keep.at((size_t)o.doc[(size_t)(p0 + i)]) >= 0;
    tile_cnt[(size_t)tile] = compact_tile_scan_host(keep.data(), cnt, c.tile_rank.data() + p0);
  }
  c.tile_base.resize((size_t)tiles + 1);
  compact_scan_host(tile_cnt.data(), tiles, c.tile_base.data());
  c.rank_at.resize((size_t)v_old + 1);
  std::vector<long long> df((size_t)v_new, -1);
  for (long e = 0; e < std::max(v_old + 1, v_new); ++e)
    bm_rp_term_entry(e, v_old, v_new, o.ptr.data(), nnz, c.tile_base.data(), c.tile_rank.data(), map, inv.data(),
                     add.ptr.data(), c.rank_at.data(), df.data(), &c.bad);
  for (long u = 0; u < v_new; ++u) CHECK(df[(size_t)u] >= 0, "df_new[%ld] was not written", u);
  c.new_ptr.resize((size_t)v_new + 1);
  compact_scan_host(df.data(), v_new, c.new_ptr.data());
  return c;
}

// which: 0 = documents whose id is a multiple of `step`; 1 = the first and the last document; 2 = every document;
//        3 = the documents at the first and the last posting of every tile of the head list (term 0 holds every document)
// mode:  0 = the null map (new terms behind the old, emptied terms keep their ids); 1 = emptied terms dropped and all
//        terms in REVERSE order (new terms in front, not monotone); 2 = dropped, order kept
// fresh: the number of new term ids on offer; rich: old terms a new document draws (0: the head term or nothing)
void merge_case(const char* what, long v, long n, long hole, long empty_run, long long pad_to, int which, long step, int mode,
                long fresh, int rich) {
  Csr o = make_csr(v, n, hole, empty_run, pad_to);
  const long v_old = (long)o.ptr.size() - 1;
  const long long nnz = o.ptr.back();
  if (pad_to > 0) CHECK(nnz == pad_to, "case did not reach %lld postings (%lld)", pad_to, nnz);
  std::vector<long long> ids;
  for (long d = 0; d < n; ++d) {
    const bool edge = d % kBmTile == 0 || d % kBmTile == kBmTile - 1;
    if (which == 0 ? d % step == 0 : which == 1 ? (d == 0 || d == n - 1) : which == 2 ? true : edge) ids.push_back(d);
  }
  const long n_rep = (long)ids.size();
  CHECK(n_rep >= 1, "%s: replaces nothing", what);
  std::vector<int> len_old((size_t)n), len_add((size_t)n_rep);
  for (int& x : len_old) x = (int)(1 + rnd() % 50);
  for (int& x : len_add) x = (int)(100 + rnd() % 50);
  // the new documents over the terms 0 .. v_old + fresh - 1 ("pre-map" ids): local document i draws its terms
  const long v_pre = v_old + fresh;
  std::vector<std::vector<std::pair<int, int>>> add_of((size_t)v_pre);  // per term: (local document, tf), ascending
  for (long i = 0; i < n_rep; ++i) {
    std::vector<long> terms;
    if (rnd() % 2) terms.push_back(0);
    for (int j = 0; j < rich; ++j) terms.push_back((long)(rnd() % (uint32_t)v_old));
    if (fresh && rnd() % 3 == 0) terms.push_back(v_old + (long)(rnd() % (uint32_t)fresh));
    if (i == 0 && fresh) terms.push_back(v_old);  // at least one new term is used
    std::sort(terms.begin(), terms.end());
    terms.erase(std::unique(terms.begin(), terms.end()), terms.end());
    for (long t : terms) add_of[(size_t)t].push_back({(int)i, (int)(1 + rnd() % 9)});
  }
  // expected, plainly: per pre-map term the surviving old pairs and the new pairs, sorted by document
  std::vector<char> gone((size_t)n, 0);
  for (long long d : ids) gone[(size_t)d] = 1;
  std::vector<std::vector<std::pair<int, int>>> want((size_t)v_pre);
  for (long t = 0; t < v_pre; ++t) {
    if (t < v_old)
      for (long long p = o.ptr[(size_t)t]; p < o.ptr[(size_t)t + 1]; ++p)
        if (!gone[(size_t)o.doc[(size_t)p]]) want[(size_t)t].push_back({o.doc[(size_t)p], o.tf[(size_t)p]});
    for (auto [i, tf] : add_of[(size_t)t]) want[(size_t)t].push_back({(int)ids[(size_t)i], tf});
    std::sort(want[(size_t)t].begin(), want[(size_t)t].end());
  }
  // the new id of every pre-map term
  std::vector<long> new_of((size_t)v_pre, -1);
  long v_new = 0;
  if (mode == 0) {
    for (long t = 0; t < v_pre; ++t) new_of[(size_t)t] = t;
    v_new = v_pre;
  } else {
    for (long t = 0; t < v_pre; ++t)
      if (!want[(size_t)t].empty()) new_of[(size_t)t] = v_new++;
    if (mode == 1)
      for (long t = 0; t < v_pre; ++t)
        if (new_of[(size_t)t] >= 0) new_of[(size_t)t] = v_new - 1 - new_of[(size_t)t];
  }
  std::vector<long> pre_of((size_t)v_new, -1);
  for (long t = 0; t < v_pre; ++t)
    if (new_of[(size_t)t] >= 0) pre_of[(size_t)new_of[(size_t)t]] = t;
  std::vector<int> map((size_t)v_old);
  for (long t = 0; t < v_old; ++t) map[(size_t)t] = (int)new_of[(size_t)t];
  Csr add;  // the call's CSR over the new ids
  add.ptr.assign(1, 0);
  std::vector<long long> eptr(1, 0);
  std::vector<int32_t> ed, et;
  for (long u = 0; u < v_new; ++u) {
    const long t = pre_of[(size_t)u];
    for (auto [i, tf] : add_of[(size_t)t]) add.doc.push_back(i), add.tf.push_back(tf);
    add.ptr.push_back((long long)add.doc.size());
    for (auto [d, tf] : want[(size_t)t]) ed.push_back(d), et.push_back(tf);
    eptr.push_back((long long)ed.size());
  }
  long emptied = 0, added_terms = 0, add_only = 0;
  for (long t = 0; t < v_old; ++t) emptied += o.ptr[(size_t)t + 1] > o.ptr[(size_t)t] && want[(size_t)t].empty();
  for (long t = v_old; t < v_pre; ++t) added_terms += !want[(size_t)t].empty();
  for (long t = 0; t < v_old; ++t)
    add_only += !want[(size_t)t].empty() && want[(size_t)t].size() == add_of[(size_t)t].size();
  const long long nnz_add = add.ptr.back();
  std::vector<double> idf((size_t)v_new, 1.0);
  std::vector<int> inv((size_t)v_new);
  const int* map_arg = mode == 0 ? nullptr : map.data();
  const int bad = bm_rp_validate((const int64_t*)ids.data(), n_rep, (const int64_t*)add.ptr.data(), add.doc.data(),
                                 add.tf.data(), len_add.data(), map_arg, v_new, idf.data(), 7.5, v_old, n, inv.data());
  CHECK(bad == kBmRpOk, "%s: a generated replace is refused: %s", what, bm_rp_error_text(bad));
  for (long u = 0; u < v_new; ++u)
    CHECK(inv[(size_t)u] == (pre_of[(size_t)u] < v_old ? (int)pre_of[(size_t)u] : -1), "%s: inv[%ld] = %d", what, u, inv[(size_t)u]);
  Counted c = count_passes(o, v_old, n, len_old, ids, len_add, add, v_new, map_arg, inv);
  CHECK(c.bad == 0, "%s: the flag was raised", what);
  for (long d = 0; d < n; ++d) {
    CHECK(c.doc_keep[(size_t)d] == (gone[(size_t)d] ? -1 : (int)d), "%s: doc_keep[%ld]", what, d);
    const long i = (long)(std::lower_bound(ids.begin(), ids.end(), (long long)d) - ids.begin());
    CHECK(c.doc_len[(size_t)d] == (gone[(size_t)d] ? len_add[(size_t)i] : len_old[(size_t)d]), "%s: doc_len[%ld]", what, d);
  }
  CHECK(c.new_ptr == eptr, "%s: new term table differs", what);
  const long long nnz_new = c.tile_base.back() + nnz_add;
  CHECK(nnz_new == (long long)ed.size() && nnz_new == c.new_ptr.back(), "%s: nnz_new %lld, expected %zu", what, nnz_new, ed.size());
  std::vector<int32_t> gd((size_t)nnz_new, -1), gt((size_t)nnz_new, -1);
  long windows_global = 0;
  if (nnz > 0)
    windows_global += host_tile_walk(o.ptr, v_old, [&](long long p, const HostTileWindow& w) {
      const int doc = c.doc_keep.at((size_t)o.doc[(size_t)p]);
      if (doc < 0) return;
      const long t = w.term_of(p);
      CHECK(o.ptr[(size_t)t] <= p && p < o.ptr[(size_t)t + 1], "posting %lld put in term %ld", p, t);
      const long long dst = bm_rp_dest_old(p, doc, t, nnz, c.tile_base.data(), c.tile_rank.data(), c.rank_at.data(),
                                           c.new_ptr.data(), map_arg, add.ptr.data(), add.doc.data(), ids.data());
      CHECK(dst >= 0 && dst < nnz_new && gd.at((size_t)dst) == -1, "old posting %lld goes to %lld", p, dst);
      gd.at((size_t)dst) = doc;
      gt.at((size_t)dst) = o.tf[(size_t)p];
    });
  if (nnz_add > 0)
    windows_global += host_tile_walk(add.ptr, v_new, [&](long long q, const HostTileWindow& w) {
      const long u = w.term_of(q);
      CHECK(add.ptr[(size_t)u] <= q && q < add.ptr[(size_t)u + 1], "add posting %lld put in term %ld", q, u);
      const long long doc = ids.at((size_t)add.doc[(size_t)q]);
      const long long dst = bm_rp_dest_add(q, doc, u, inv.data(), o.ptr.data(), o.doc.data(), nnz, c.tile_base.data(),
                                           c.tile_rank.data(), c.rank_at.data(), c.new_ptr.data(), add.ptr.data());
      CHECK(dst >= 0 && dst < nnz_new && gd.at((size_t)dst) == -1, "add posting %lld goes to %lld", q, dst);
      gd.at((size_t)dst) = (int32_t)doc;
      gt.at((size_t)dst) = add.tf[(size_t)q];
    });
  CHECK(gd == ed && gt == et, "%s: merged postings differ", what);
  std::printf("merge ok: %s: %ld of %ld docs, %ld->%ld terms (%ld emptied, %ld new, %ld from the add alone), %lld-%lld+%lld "
              "postings, %ld window(s) searched in the table itself\n", what, n_rep, n, v_old, v_new, emptied, added_terms,
              add_only, nnz, nnz - c.tile_base.back(), nnz_add, windows_global);
}

void validate_cases() {
  const int64_t ids[2] = {1, 3};
  const int64_t ptr[4] = {0, 1, 3, 3};
  const int32_t doc[3] = {0, 0, 1}, tf[3] = {2, 1, 1}, len[2] = {4, 5};
  const int32_t map[3] = {1, -1, 0};
  const double idf[3] = {1.0, 0.5, 2.0};
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  int32_t inv[4];
  auto v = [&](const int64_t* r, int64_t nr, const int64_t* tp, const int32_t* pd, const int32_t* pt, const int32_t* dl,
               const int32_t* m, int64_t vn, const double* i, double avg, int64_t vo = 3, int64_t no = 5) {
    return bm_rp_validate(r, nr, tp, pd, pt, dl, m, vn, i, avg, vo, no, inv);
  };
  CHECK(v(ids, 2, ptr, doc, tf, len, map, 3, idf, 4.5) == kBmRpOk, "the good replace");
  CHECK(inv[0] == 2 && inv[1] == 0 && inv[2] == -1, "its inverse map: %d %d %d", inv[0], inv[1], inv[2]);
  CHECK(v(ids, 2, ptr, doc, tf, len, nullptr, 3, idf, 4.5) == kBmRpOk, "the good replace without a map");
  CHECK(inv[0] == 0 && inv[1] == 1 && inv[2] == 2, "the identity's inverse");
  CHECK(v(ids, 2, ptr, doc, tf, len, nullptr, 3, idf, 4.5, 2, 5) == kBmRpOk, "a new term behind the old");
  CHECK(inv[2] == -1, "the new term has no old one");
  CHECK(v(nullptr, 2, ptr, doc, tf, len, map, 3, idf, 4.5) == kBmRpNull, "null replace_ids");
  CHECK(v(ids, 2, nullptr, doc, tf, len, map, 3, idf, 4.5) == kBmRpNull, "null term_ptr_add");
  CHECK(v(ids, 2, ptr, nullptr, tf, len, map, 3, idf, 4.5) == kBmRpNull, "null post_doc_add");
  CHECK(v(ids, 2, ptr, doc, nullptr, len, map, 3, idf, 4.5) == kBmRpNull, "null post_tf_add");
  CHECK(v(ids, 2, ptr, doc, tf, nullptr, map, 3, idf, 4.5) == kBmRpNull, "null doc_len_add");
  CHECK(v(ids, 2, ptr, doc, tf, len, map, 3, nullptr, 4.5) == kBmRpNull, "null idf");
  CHECK(v(ids, -1, ptr, doc, tf, len, map, 3, idf, 4.5) == kBmRpSizes, "n_rep < 0");
  CHECK(v(ids, 2, ptr, doc, tf, len, map, 3, idf, 4.5, 3, 1) == kBmRpSizes, "n_rep > n_docs");
  CHECK(v(ids, 2, ptr, doc, tf, len, nullptr, 2, idf, 4.5) == kBmRpSizes, "no map and n_terms_new below n_terms");
  CHECK(v(ids, 2, ptr, doc, tf, len, map, -1, idf, 4.5) == kBmRpSizes, "n_terms_new < 0");
  const int64_t r1[2] = {1, 5}, r2[2] = {-1, 3}, r3[2] = {3, 3}, r4[2] = {3, 1};
  CHECK(v(r1, 2, ptr, doc, tf, len, map, 3, idf, 4.5) == kBmRpIdRange, "id n_docs");
  CHECK(v(r2, 2, ptr, doc, tf, len, map, 3, idf, 4.5) == kBmRpIdRange, "id -1");
  CHECK(v(r3, 2, ptr, doc, tf, len, map, 3, idf, 4.5) == kBmRpIdOrder, "a repeated id");
  CHECK(v(r4, 2, ptr, doc, tf, len, map, 3, idf, 4.5) == kBmRpIdOrder, "descending ids");
  for (double bad : {0.0, -1.0, inf, nan}) CHECK(v(ids, 2, ptr, doc, tf, len, map, 3, idf, bad) == kBmRpAvgdl, "avgdl %g", bad);
  const double i1[3] = {1.0, inf, 1.0}, i2[3] = {nan, 0.5, 1.0};
  CHECK(v(ids, 2, ptr, doc, tf, len, map, 3, i1, 4.5) == kBmRpIdf, "infinite idf");
  CHECK(v(ids, 2, ptr, doc, tf, len, map, 3, i2, 4.5) == kBmRpIdf, "NaN idf");
  const int32_t m1[3] = {1, 3, 0}, m2[3] = {1, -2, 0}, m3[3] = {1, 1, 0};
  CHECK(v(ids, 2, ptr, doc, tf, len, m1, 3, idf, 4.5) == kBmRpMapRange, "map value n_terms_new");
  CHECK(v(ids, 2, ptr, doc, tf, len, m2, 3, idf, 4.5) == kBmRpMapRange, "map value -2");
  CHECK(v(ids, 2, ptr, doc, tf, len, m3, 3, idf, 4.5) == kBmRpMapTwice, "two terms on one new id");
  const int64_t p1[4] = {1, 1, 3, 3}, p2[4] = {0, 2, 1, 3};
  CHECK(v(ids, 2, p1, doc, tf, len, map, 3, idf, 4.5) == kBmRpPtrStart, "term_ptr_add[0] != 0");
  CHECK(v(ids, 2, p2, doc, tf, len, map, 3, idf, 4.5) == kBmRpPtrOrder, "term_ptr_add falls");
  const int32_t d1[3] = {0, 0, 2}, d2[3] = {0, -1, 1}, d3[3] = {0, 1, 1}, d4[3] = {0, 1, 0};
  CHECK(v(ids, 2, ptr, d1, tf, len, map, 3, idf, 4.5) == kBmRpDocRange, "local document n_rep");
  CHECK(v(ids, 2, ptr, d2, tf, len, map, 3, idf, 4.5) == kBmRpDocRange, "local document -1");
  CHECK(v(ids, 2, ptr, d3, tf, len, map, 3, idf, 4.5) == kBmRpDocOrder, "a repeated local document");
  CHECK(v(ids, 2, ptr, d4, tf, len, map, 3, idf, 4.5) == kBmRpDocOrder, "descending local documents");
  // what only the counting passes see: term 1 is mapped to -1 but document 0 survives in its list
  Csr o;
  o.ptr = {0, 2, 3, 4};
  o.doc = {0, 1, 0, 3};
  o.tf = {1, 1, 2, 1};
  Csr add;
  add.ptr.assign(ptr, ptr + 4);
  add.doc.assign(doc, doc + 3);
  add.tf.assign(tf, tf + 3);
  const std::vector<int> len_old(5, 3), len_add(len, len + 2);
  CHECK(v(ids, 2, ptr, doc, tf, len, map, 3, idf, 4.5) == kBmRpOk, "the good replace again");
  Counted c = count_passes(o, 3, 5, len_old, {1, 3}, len_add, add, 3, map, std::vector<int>(inv, inv + 3));
  CHECK(c.bad == 1, "a dropped term with a surviving posting raises the flag");
  const int32_t ok_map[3] = {1, 0, -1};  // term 2's only document (3) is replaced
  CHECK(v(ids, 2, ptr, doc, tf, len, ok_map, 3, idf, 4.5) == kBmRpOk, "the other map");
  c = count_passes(o, 3, 5, len_old, {1, 3}, len_add, add, 3, ok_map, std::vector<int>(inv, inv + 3));
  CHECK(c.bad == 0 && c.tile_base.back() == 2 && c.new_ptr.back() == 5, "a dropped term without survivors does not");
}

}  // namespace

int main() {
  const long long T = kBmTile;
  merge_case("smallest index, its one document", 1, 1, 0, 0, 0, 2, 1, 0, 1, 0);
  merge_case("every 40th document, null map", 400, 1500, 0, 0, 0, 0, 40, 0, 5, 3);
  merge_case("every 40th document, terms dropped and reversed", 400, 1500, 0, 0, 0, 0, 40, 1, 5, 3);
  merge_case("one document", 400, 1500, 0, 0, 0, 0, 5000, 2, 1, 6);
  merge_case("the first and the last document", 400, 1500, 0, 0, 0, 1, 1, 1, 3, 4);
  merge_case("every document", 60, 300, 0, 0, 0, 2, 1, 1, 20, 2);
  merge_case("every document, null map", 60, 300, 0, 0, 0, 2, 1, 0, 20, 2);
  merge_case("every other document, one-token replacements", 300, 64, 7, 0, 0, 0, 2, 2, 0, 0);
  merge_case("terms without postings", 400, 64, 7, 0, 0, 0, 3, 2, 4, 2);
  merge_case("short lists: many terms per tile", 5000, 3, 2, 0, 0, 1, 1, 1, 50, 40);
  merge_case("the tile edges of a head list of 3 tiles and more", 6, 3 * T + 100, 0, 0, 0, 3, 1, 1, 2, 2);
  merge_case("the tile edges, null map", 6, 3 * T + 100, 0, 0, 0, 3, 1, 0, 2, 2);
  merge_case("a tile less one", 10, 600, 0, 0, T - 1, 0, 9, 1, 3, 3);
  merge_case("a tile exactly", 10, 600, 0, 0, T, 0, 9, 2, 3, 3);
  merge_case("a tile and one more", 10, 600, 0, 0, T + 1, 0, 9, 0, 3, 3);
  merge_case("3 tiles and five more", 10, 2000, 0, 0, 3 * T + 5, 0, 7, 1, 3, 3);
  merge_case("an add of more than a tile", 30, 3000, 0, 0, 0, 0, 2, 1, 9, 3);
  merge_case("a wide run of empty terms", 12, 300, 0, kBmTile + 50, 0, 0, 2, 1, 4, 2);
  merge_case("a wide run of empty terms, null map", 12, 300, 0, kBmTile + 50, 0, 0, 4, 0, 4, 2);
  validate_cases();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("bm25 replace rule ok\n");
  return 0;
}

// Host check of the rules of amdr_bm25_add (bm25_add_rule.hpp, bm25_tile_rule.hpp), a program of its own (never part of
// the library):
//   check_bm25_add
// It builds random term-major indexes and adds (Zipfian lists, terms without postings, new terms, a total that is an
// exact multiple of the merge tile and one more), merges them on the CPU the way bm25_merge_kernel does — tile by tile
// (host_tile_walk, check_bm25_common.hpp), the tile's terms by bm_tile_terms, a window of the term table copied out
// exactly as the kernel's LDS window, every posting by bm_tile_term_of + bm_add_source — and compares the result with a
// plain per-term concatenation.  Every array is a std::vector of exactly the size the ABI promises, so with the host
// sanitizers (tests/test_bm25_add_rule_host.py) an access outside one is a failure.  Then every refusal of
// bm_add_validate is provoked once, on arrays of exact size.
// Build: c++ -std=c++17 check_bm25_add.cpp (plain host code; no HIP header is read).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "bm25_add_rule.hpp"
#include "check_bm25_common.hpp"

using namespace amdr;

namespace {

void merge_case(long v_old, long n_old, long v_new, long n_add, long hole, long long pad_to) {
  Csr o = make_csr(v_old, n_old, hole, 0, 0), a = make_csr(v_new, n_add, hole, 0, 0);
  // pad_to: further new terms behind the add's table, each holding up to every added document, until the index has
  // exactly pad_to postings
  for (long long total = o.ptr.back() + a.ptr.back(); total < pad_to; ++v_new) {
    const long df = pad_to - total < n_add ? (long)(pad_to - total) : n_add;
    for (long j = 0; j < df; ++j) {
      a.doc.push_back((int32_t)j);
      a.tf.push_back(1);
    }
    a.ptr.push_back((long long)a.doc.size());
    total += df;
  }
  std::vector<double> idf((size_t)v_new, 1.0);
  std::vector<int32_t> dl((size_t)n_add, 3);
  const int bad = bm_add_validate((const int64_t*)a.ptr.data(), a.doc.data(), a.tf.data(), idf.data(), dl.data(), v_new, n_add, 7.5, v_old, n_old);
  CHECK(bad == kBmAddOk, "a generated add is refused: %s", bm_add_error_text(bad));
  std::vector<long long> nptr((size_t)v_new + 1);
  for (long t = 0; t <= v_new; ++t) nptr[(size_t)t] = bm_add_term_ptr(o.ptr.data(), v_old, a.ptr.data(), t);
  // expected: per term, the old list, then the add's with n_old added
  std::vector<int32_t> ed, et;
  for (long t = 0; t < v_new; ++t) {
    CHECK(nptr[(size_t)t] == (long long)ed.size(), "term_ptr[%ld] = %lld, expected %zu", t, nptr[(size_t)t], ed.size());
    if (t < v_old)
      for (long long p = o.ptr[t]; p < o.ptr[t + 1]; ++p) ed.push_back(o.doc[(size_t)p]), et.push_back(o.tf[(size_t)p]);
    for (long long p = a.ptr[t]; p < a.ptr[t + 1]; ++p) ed.push_back(a.doc[(size_t)p] + (int32_t)n_old), et.push_back(a.tf[(size_t)p]);
  }
  const long long nnz = nptr[(size_t)v_new];
  CHECK(nnz == (long long)ed.size(), "nnz %lld, expected %zu", nnz, ed.size());
  if (pad_to > 0) CHECK(nnz == pad_to, "case did not reach %lld postings (%lld)", pad_to, nnz);
  std::vector<int32_t> gd((size_t)nnz, -1), gt((size_t)nnz, -1);
  const long windows_global = host_tile_walk(nptr, v_new, [&](long long p, const HostTileWindow& w) {
    const long t = w.term_of(p);
    CHECK(nptr[(size_t)t] <= p && p < nptr[(size_t)t + 1], "posting %lld put in term %ld", p, t);
    bool from_add;
    const long long src = bm_add_source(p, w.start_of(t), t, o.ptr.data(), v_old, a.ptr.data(), &from_add);
    gd[(size_t)p] = from_add ? a.doc.at((size_t)src) + (int32_t)n_old : o.doc.at((size_t)src);
    gt[(size_t)p] = from_add ? a.tf.at((size_t)src) : o.tf.at((size_t)src);
  });
  CHECK(gd == ed && gt == et, "merged postings differ (v_old %ld n_old %ld v_new %ld n_add %ld hole %ld)", v_old, n_old, v_new, n_add, hole);
  std::printf("merge ok: %ld+%ld docs, %ld->%ld terms, %lld postings, %ld window(s) searched in the table itself\n", n_old,
              n_add, v_old, v_new, nnz, windows_global);
}

void validate_cases() {
  const int64_t ptr[4] = {0, 2, 2, 3};
  const int32_t doc[3] = {0, 1, 1}, tf[3] = {1, 2, 3}, dl[2] = {4, 5};
  const double idf[3] = {1.0, 0.5, 2.0};
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  auto v = [&](const int64_t* p, const int32_t* d, const int32_t* t, const double* i, const int32_t* l, int64_t nt, int64_t na,
               double avg, int64_t vo = 2, int64_t no = 10) { return bm_add_validate(p, d, t, i, l, nt, na, avg, vo, no); };
  CHECK(v(ptr, doc, tf, idf, dl, 3, 2, 4.5) == kBmAddOk, "the good add");
  CHECK(v(ptr, doc, tf, idf, dl, 3, -1, 4.5) == kBmAddSizes, "n_add < 0");
  CHECK(v(ptr, doc, tf, idf, dl, 3, 2, 4.5, 4) == kBmAddSizes, "n_terms below the handle's");
  CHECK(v(ptr, doc, tf, idf, dl, 3, 2, 4.5, 2, (1ll << 31) - 2) == kBmAddSizes, "2^31 documents");
  CHECK(v(ptr, doc, tf, idf, dl, 3, 2, 4.5, 2, (1ll << 31) - 3) == kBmAddOk, "2^31 - 1 documents");
  CHECK(v(nullptr, doc, tf, idf, dl, 3, 2, 4.5) == kBmAddNull, "null term_ptr_add");
  CHECK(v(ptr, nullptr, tf, idf, dl, 3, 2, 4.5) == kBmAddNull, "null post_doc_add");
  CHECK(v(ptr, doc, nullptr, idf, dl, 3, 2, 4.5) == kBmAddNull, "null post_tf_add");
  CHECK(v(ptr, doc, tf, nullptr, dl, 3, 2, 4.5) == kBmAddNull, "null idf");
  CHECK(v(ptr, doc, tf, idf, nullptr, 3, 2, 4.5) == kBmAddNull, "null doc_len_add");
  for (double bad : {0.0, -1.0, inf, nan}) CHECK(v(ptr, doc, tf, idf, dl, 3, 2, bad) == kBmAddAvgdl, "avgdl %g", bad);
  const int64_t p1[4] = {1, 2, 2, 3}, p2[4] = {0, 2, 1, 3};
  CHECK(v(p1, doc, tf, idf, dl, 3, 2, 4.5) == kBmAddPtrStart, "term_ptr_add[0] != 0");
  CHECK(v(p2, doc, tf, idf, dl, 3, 2, 4.5) == kBmAddPtrOrder, "term_ptr_add not monotone");
  const double i1[3] = {1.0, inf, 2.0}, i2[3] = {1.0, 0.5, nan};
  CHECK(v(ptr, doc, tf, i1, dl, 3, 2, 4.5) == kBmAddIdf, "infinite idf");
  CHECK(v(ptr, doc, tf, i2, dl, 3, 2, 4.5) == kBmAddIdf, "NaN idf");
  const int32_t d1[3] = {0, 2, 1}, d2[3] = {-1, 1, 1}, d3[3] = {1, 1, 1}, d4[3] = {1, 0, 1};
  CHECK(v(ptr, d1, tf, idf, dl, 3, 2, 4.5) == kBmAddDocRange, "document n_add");
  CHECK(v(ptr, d2, tf, idf, dl, 3, 2, 4.5) == kBmAddDocRange, "document -1");
  CHECK(v(ptr, d3, tf, idf, dl, 3, 2, 4.5) == kBmAddDocOrder, "a repeated document");
  CHECK(v(ptr, d4, tf, idf, dl, 3, 2, 4.5) == kBmAddDocOrder, "descending documents");
  const int64_t p0[4] = {0, 0, 0, 0};  // an add of documents without a token: no posting array is read
  CHECK(v(p0, nullptr, nullptr, idf, dl, 3, 2, 4.5) == kBmAddOk, "empty documents");
}

}  // namespace

int main() {
  merge_case(1, 1, 2, 1, 0, 0);                             // smallest index
  merge_case(400, 1500, 420, 600, 0, 0);
  merge_case(400, 64, 420, 37, 7, 0);                       // terms without postings
  merge_case(5000, 3, 9000, 2, 2, 0);                       // mostly short lists: many terms per tile
  merge_case(3, 40, 3 * kBmTile, 50, 0, 0);              // new terms, almost all without postings ...
  merge_case(40, 2000, 60, 2000, 0, 10ll * kBmTile);      // exactly a multiple of the tile
  merge_case(40, 2000, 60, 2000, 0, 10ll * kBmTile + 1);  // and one more
  {  // a window that does not fit: one posting, then > tile terms without any, then one posting
    const long v = kBmTile + 50;
    std::vector<long long> optr((size_t)3, 0), aptr((size_t)v + 1, 0);
    optr[1] = optr[2] = 1;  // old: term 0 has one posting, term 1 none
    aptr[(size_t)v] = 1;    // add: the last term has one
    std::vector<long long> nptr((size_t)v + 1);
    for (long t = 0; t <= v; ++t) nptr[(size_t)t] = bm_add_term_ptr(optr.data(), 2, aptr.data(), t);
    long t0, t1;
    bm_tile_terms(nptr.data(), v, 0, 2, &t0, &t1);
    CHECK(t0 == 0 && t1 == v - 1 && !bm_tile_window_fits(t0, t1), "wide window: terms %ld .. %ld", t0, t1);
    CHECK(bm_tile_term_of(nptr.data(), 0, t0, t1, 0) == 0 && bm_tile_term_of(nptr.data(), 0, t0, t1, 1) == v - 1, "wide window search");
    bool fa;
    CHECK(bm_add_source(1, nptr[(size_t)v - 1], v - 1, optr.data(), 2, aptr.data(), &fa) == 0 && fa, "wide window source");
  }
  validate_cases();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("bm25 add rule ok\n");
  return 0;
}

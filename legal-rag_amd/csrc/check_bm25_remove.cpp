// Host check of the rules of amdr_bm25_remove (bm25_remove_rule.hpp, bm25_tile_rule.hpp, compact.hpp), a program of its
// own (never part of the library):
//   check_bm25_remove
// It builds random term-major indexes (Zipfian lists, terms without postings, a total that is an exact multiple of the
// tile and one more), removes documents and compacts on the CPU the way the kernels do — the document map by
// bm_rm_doc_new, tile by tile the keep flags and their ranks (compact_tile_scan_host), the tile bases and the new term
// table by compact_scan_host, every term by bm_rm_term_entry, then tile by tile again (host_tile_walk,
// check_bm25_common.hpp) the tile's terms by bm_tile_terms, a window of the OLD term table copied out exactly as the
// kernel's LDS window, every surviving posting by bm_tile_term_of + bm_rm_dest — and compares the result with a plain
// per-term filter followed by a stable reorder by new term id.  Every array is a std::vector of exactly the size the call
// allocates, so with the host sanitizers (tests/test_bm25_remove_rule_host.py) an access outside one is a failure.  Then
// every refusal of bm_rm_validate is provoked once, on arrays of exact size, and the device-side flag (a term mapped to -1
// with a surviving posting) once.
// Build: c++ -std=c++17 check_bm25_remove.cpp (plain host code; no HIP header is needed).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#define AMDR_COMPACT_HOST_ONLY 1  // the host forms alone: this program has no device code
#include "bm25_remove_rule.hpp"
#include "check_bm25_common.hpp"
#include "compact.hpp"

using namespace amdr;

namespace {

// What the device computes up to the host's look at the total and the flag, on arrays of the call's sizes.
struct Counted {
  std::vector<int> doc_new;
  std::vector<unsigned short> tile_rank;
  std::vector<long long> tile_base, rank_at, new_ptr;
  int bad = 0;
};

Counted count_passes(const Csr& o, long v_old, long n_old, const std::vector<long long>& rm, const int* map, long v_new) {
  Counted c;
  const long long nnz = o.ptr.back();
  const long tiles = (long)((nnz + kBmTile - 1) / kBmTile);
  c.doc_new.resize((size_t)n_old);
  for (long d = 0; d < n_old; ++d) c.doc_new[(size_t)d] = bm_rm_doc_new(rm.data(), (long)rm.size(), d);
  c.tile_rank.resize((size_t)nnz);
  std::vector<long long> tile_cnt((size_t)tiles);
  for (long tile = 0; tile < tiles; ++tile) {
    const long long p0 = (long long)tile * kBmTile;
    const int n = (int)std::min<long long>(kBmTile, nnz - p0);
    std::vector<unsigned char> keep((size_t)n);
    for (int i = 0; i < n; ++i) keep[(size_t)i] = c.doc_new.at((size_t)o.doc[(size_t)(p0 + i)]) >= 0;
    tile_cnt[(size_t)tile] = compact_tile_scan_host(keep.data(), n, c.tile_rank.data() + p0);
  }
  c.tile_base.resize((size_t)tiles + 1);
  compact_scan_host(tile_cnt.data(), tiles, c.tile_base.data());
  c.rank_at.resize((size_t)v_old + 1);
  std::vector<long long> df((size_t)v_new, -1);
  for (long t = 0; t <= v_old; ++t)
    bm_rm_term_entry(t, v_old, o.ptr.data(), nnz, c.tile_base.data(), c.tile_rank.data(), map, c.rank_at.data(), df.data(), &c.bad);
  for (long m = 0; m < v_new; ++m) CHECK(df[(size_t)m] >= 0, "df_new[%ld] was not written", m);
  c.new_ptr.resize((size_t)v_new + 1);
  compact_scan_host(df.data(), v_new, c.new_ptr.data());
  return c;
}

// mode 0: the null map; 1: emptied terms dropped, the rest in REVERSE order (not monotone); 2: dropped, order kept
void compact_case(const char* what, long v, long n_old, long hole, long empty_run, long long pad_to, long long nnz_new_want,
                  int keep_mod, int keep_from, int mode) {
  Csr o = make_csr(v, n_old, hole, empty_run, pad_to);
  const long v_old = (long)o.ptr.size() - 1;
  const long long nnz = o.ptr.back();
  if (pad_to > 0) CHECK(nnz == pad_to, "case did not reach %lld postings (%lld)", pad_to, nnz);
  // removed: documents below keep_from, and of the rest those whose id is not a multiple of keep_mod; keep_from < 0: the
  // last document only
  std::vector<long long> rm;
  for (long d = 0; d < n_old; ++d)
    if (keep_from < 0 ? d == n_old - 1 : (d < keep_from || (keep_mod > 1 && d % keep_mod != 0))) rm.push_back(d);
  if (nnz_new_want > 0) {  // remove further documents from the end until at most that many postings survive, then
    std::vector<long> per_doc((size_t)n_old, 0);  // (the lists being what they are) check that it was hit exactly
    for (int32_t d : o.doc) ++per_doc[(size_t)d];
    long long left = 0;
    std::vector<char> gone((size_t)n_old, 0);
    for (long long d : rm) gone[(size_t)d] = 1;
    for (long d = 0; d < n_old; ++d) left += gone[(size_t)d] ? 0 : per_doc[(size_t)d];
    for (long d = n_old - 1; d > 0 && left - per_doc[(size_t)d] >= nnz_new_want; --d)
      if (!gone[(size_t)d]) gone[(size_t)d] = 1, left -= per_doc[(size_t)d];
    rm.clear();
    for (long d = 0; d < n_old; ++d)
      if (gone[(size_t)d]) rm.push_back(d);
  }
  CHECK(!rm.empty() && (long)rm.size() < n_old, "%s: removes %zu of %ld", what, rm.size(), n_old);
  // expected, plainly: per old term the surviving postings with the documents renumbered
  std::vector<int> renum((size_t)n_old, -1);
  {
    size_t j = 0;
    int next = 0;
    for (long d = 0; d < n_old; ++d) {
      if (j < rm.size() && rm[j] == d)
        ++j;
      else
        renum[(size_t)d] = next++;
    }
  }
  std::vector<std::vector<int32_t>> fd((size_t)v_old), ft((size_t)v_old);
  for (long t = 0; t < v_old; ++t)
    for (long long p = o.ptr[(size_t)t]; p < o.ptr[(size_t)t + 1]; ++p)
      if (renum[(size_t)o.doc[(size_t)p]] >= 0) fd[(size_t)t].push_back(renum[(size_t)o.doc[(size_t)p]]), ft[(size_t)t].push_back(o.tf[(size_t)p]);
  std::vector<int> map((size_t)v_old, -1);
  long v_new = 0;
  if (mode == 0) {
    for (long t = 0; t < v_old; ++t) map[(size_t)t] = (int)t;
    v_new = v_old;
  } else {
    for (long t = 0; t < v_old; ++t)
      if (!fd[(size_t)t].empty()) map[(size_t)t] = (int)v_new++;
    if (mode == 1)
      for (long t = 0; t < v_old; ++t)
        if (map[(size_t)t] >= 0) map[(size_t)t] = (int)(v_new - 1) - map[(size_t)t];
  }
  std::vector<long> old_of((size_t)v_new, -1);  // the stable reorder by new term id
  for (long t = 0; t < v_old; ++t)
    if (map[(size_t)t] >= 0) old_of[(size_t)map[(size_t)t]] = t;
  std::vector<long long> eptr(1, 0);
  std::vector<int32_t> ed, et;
  for (long m = 0; m < v_new; ++m) {
    const long t = old_of[(size_t)m];
    ed.insert(ed.end(), fd[(size_t)t].begin(), fd[(size_t)t].end());
    et.insert(et.end(), ft[(size_t)t].begin(), ft[(size_t)t].end());
    eptr.push_back((long long)ed.size());
  }
  std::vector<double> idf((size_t)v_new, 1.0);
  const int* map_arg = mode == 0 ? nullptr : map.data();
  const int bad = bm_rm_validate((const int64_t*)rm.data(), (int64_t)rm.size(), map_arg, v_new, idf.data(), 7.5, v_old, n_old);
  CHECK(bad == kBmRmOk, "%s: a generated remove is refused: %s", what, bm_rm_error_text(bad));
  Counted c = count_passes(o, v_old, n_old, rm, map_arg, v_new);
  CHECK(c.bad == 0, "%s: the flag was raised", what);
  CHECK(c.doc_new == renum, "%s: document map differs", what);
  CHECK(c.new_ptr == eptr, "%s: new term table differs", what);
  const long long nnz_new = c.tile_base.back();
  CHECK(nnz_new == (long long)ed.size(), "%s: nnz_new %lld, expected %zu", what, nnz_new, ed.size());
  if (nnz_new_want > 0) CHECK(nnz_new == nnz_new_want, "%s: case did not leave %lld postings (%lld)", what, nnz_new_want, nnz_new);
  std::vector<int32_t> gd((size_t)nnz_new, -1), gt((size_t)nnz_new, -1);
  long zero_tiles = 0;
  for (size_t tile = 0; tile + 1 < c.tile_base.size(); ++tile) zero_tiles += c.tile_base[tile + 1] == c.tile_base[tile];
  const long windows_global = host_tile_walk(o.ptr, v_old, [&](long long p, const HostTileWindow& w) {
    const int doc = c.doc_new.at((size_t)o.doc[(size_t)p]);
    if (doc < 0) return;
    const long t = w.term_of(p);
    CHECK(o.ptr[(size_t)t] <= p && p < o.ptr[(size_t)t + 1], "posting %lld put in term %ld", p, t);
    const long long dst = bm_rm_dest(p, t, nnz, c.tile_base.data(), c.tile_rank.data(), c.rank_at.data(), c.new_ptr.data(), map_arg);
    CHECK(dst >= 0 && dst < nnz_new && gd.at((size_t)dst) == -1, "posting %lld goes to %lld", p, dst);
    gd.at((size_t)dst) = doc;
    gt.at((size_t)dst) = o.tf[(size_t)p];
  });
  CHECK(gd == ed && gt == et, "%s: compacted postings differ", what);
  bool monotone = true;
  long last = -1;
  for (long t = 0; t < v_old; ++t)
    if (map[(size_t)t] >= 0) monotone = monotone && map[(size_t)t] > last, last = map[(size_t)t];
  if (mode == 1 && v_new > 1) CHECK(!monotone, "%s: the map is monotone", what);
  std::printf("compact ok: %s: %ld-%zu docs, %ld->%ld terms, %lld->%lld postings, %ld tile(s) without a survivor, %ld window(s) "
              "searched in the table itself\n", what, n_old, rm.size(), v_old, v_new, nnz, nnz_new, zero_tiles, windows_global);
}

void validate_cases() {
  const int64_t ids[2] = {1, 3};
  const int32_t map[3] = {1, -1, 0};
  const double idf[3] = {1.0, 0.5, 2.0};
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  auto v = [&](const int64_t* r, int64_t nr, const int32_t* m, int64_t vn, const double* i, double avg, int64_t vo = 3,
               int64_t no = 5) { return bm_rm_validate(r, nr, m, vn, i, avg, vo, no); };
  CHECK(v(ids, 2, map, 2, idf, 4.5) == kBmRmOk, "the good remove");
  CHECK(v(ids, 2, nullptr, 3, idf, 4.5) == kBmRmOk, "the good remove without a map");
  CHECK(v(nullptr, 2, map, 2, idf, 4.5) == kBmRmNull, "null remove_ids");
  CHECK(v(ids, 2, map, 2, nullptr, 4.5) == kBmRmNull, "null idf");
  CHECK(v(ids, -1, map, 2, idf, 4.5) == kBmRmSizes, "n_remove < 0");
  CHECK(v(ids, 2, map, 2, idf, 4.5, 3, 2) == kBmRmSizes, "n_remove == n_docs");
  CHECK(v(ids, 2, nullptr, 2, idf, 4.5) == kBmRmSizes, "no map and n_terms_new != n_terms");
  CHECK(v(ids, 2, map, 4, idf, 4.5) == kBmRmSizes, "n_terms_new above n_terms");
  CHECK(v(ids, 2, map, -1, idf, 4.5) == kBmRmSizes, "n_terms_new < 0");
  const int64_t r1[2] = {1, 5}, r2[2] = {-1, 3}, r3[2] = {3, 3}, r4[2] = {3, 1};
  CHECK(v(r1, 2, map, 2, idf, 4.5) == kBmRmIdRange, "id n_docs");
  CHECK(v(r2, 2, map, 2, idf, 4.5) == kBmRmIdRange, "id -1");
  CHECK(v(r3, 2, map, 2, idf, 4.5) == kBmRmIdOrder, "a repeated id");
  CHECK(v(r4, 2, map, 2, idf, 4.5) == kBmRmIdOrder, "descending ids");
  for (double bad : {0.0, -1.0, inf, nan}) CHECK(v(ids, 2, map, 2, idf, bad) == kBmRmAvgdl, "avgdl %g", bad);
  const double i1[2] = {1.0, inf}, i2[2] = {nan, 0.5};
  CHECK(v(ids, 2, map, 2, i1, 4.5) == kBmRmIdf, "infinite idf");
  CHECK(v(ids, 2, map, 2, i2, 4.5) == kBmRmIdf, "NaN idf");
  const int32_t m1[3] = {1, 2, 0}, m2[3] = {1, -2, 0}, m3[3] = {1, 1, 0}, m4[3] = {1, -1, -1};
  CHECK(v(ids, 2, m1, 2, idf, 4.5) == kBmRmMapRange, "map value n_terms_new");
  CHECK(v(ids, 2, m2, 2, idf, 4.5) == kBmRmMapRange, "map value -2");
  CHECK(v(ids, 2, m3, 2, idf, 4.5) == kBmRmMapTwice, "two terms on one new id");
  CHECK(v(ids, 2, m4, 2, idf, 4.5) == kBmRmMapMissing, "a new id no term maps to");
  const int32_t m5[3] = {-1, -1, -1};  // every term dropped: no idf is read
  CHECK(v(ids, 2, m5, 0, nullptr, 4.5) == kBmRmOk, "all terms dropped");
  // what only the counting passes see: term 1 is mapped to -1 but document 0 survives in its list
  Csr o;
  o.ptr = {0, 2, 3, 4};
  o.doc = {0, 1, 0, 3};
  o.tf = {1, 1, 2, 1};
  Counted c = count_passes(o, 3, 5, {1, 3}, map, 2);
  CHECK(c.bad == 1, "a dropped term with a surviving posting raises the flag");
  const int32_t ok_map[3] = {1, 0, -1};  // term 2's only document (3) is removed
  c = count_passes(o, 3, 5, {1, 3}, ok_map, 2);
  CHECK(c.bad == 0 && c.tile_base.back() == 2, "a dropped term without survivors does not");
}

}  // namespace

int main() {
  const long long T = kBmTile;
  compact_case("smallest index", 1, 2, 0, 0, 0, 0, 1, 1, 2);
  compact_case("every other document, null map", 400, 1500, 0, 0, 0, 0, 2, 0, 0);
  compact_case("every third kept, terms dropped and reversed", 400, 1500, 0, 0, 0, 0, 3, 0, 1);
  compact_case("terms without postings", 400, 64, 7, 0, 0, 0, 1, 5, 2);
  compact_case("short lists: many terms per tile", 5000, 3, 2, 0, 0, 0, 1, 1, 1);
  compact_case("first tile of the head list removed", 6, 4100, 0, 0, 0, 0, 1, 2100, 1);
  compact_case("last document only", 6, 4100, 0, 0, 0, 0, 1, -1, 0);
  compact_case("3 tiles exactly", 10, 2000, 0, 0, 3 * T, 0, 2, 0, 1);
  compact_case("3 tiles and one more", 10, 2000, 0, 0, 3 * T + 1, 0, 2, 0, 0);
  compact_case("2 tiles survive exactly", 1, T, 0, 0, 4 * T, 2 * T, 1, 1, 1);
  compact_case("a wide run of empty terms", 12, 300, 0, kBmTile + 50, 0, 0, 2, 0, 1);
  compact_case("a wide run of empty terms, null map", 12, 300, 0, kBmTile + 50, 0, 0, 4, 10, 0);
  validate_cases();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("bm25 remove rule ok\n");
  return 0;
}

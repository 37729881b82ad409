// Host check of the rules of amdr_facet_counts (facet_rule.hpp), a program of its own:
//   check_facets
// It counts generated scope tables cell by cell as the kernels of facet.hip do — per (constraint, tile of kFcTile rows,
// field) the tile's part of the scope by fc_tile_range, per row the bin by fc_row_ok / fc_bin, a block histogram of exactly
// n_codes + 1 bins when the field fits LDS and the non-zero bins added to the constraint's counters, the counters
// themselves otherwise; then per (constraint, field) the keys of the non-zero counters, ordered, and the slots of the list
// by fc_slot_code / fc_slot_count — and compares every output with a naive count.  Every array has exactly the size the
// header promises (allocated at that size), so with the host sanitizers (tests/test_facet_rule_host.py) an access outside
// one is a failure.  Then the written-out cases and every refusal of fc_check_args and fc_validate.
// Build: c++ -std=c++17 check_facets.cpp (plain host code; no HIP header is needed).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <vector>

#include "facet_rule.hpp"

using namespace amdr;

namespace {

int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      ++failures;                        \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
    }                                    \
  } while (0)

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  long below(long n) { return (long)(next() % (uint32_t)n); }
};

template <class T>
std::vector<T> exact(const std::vector<T>& v) {  // capacity == size: the sanitizer sees the promised size
  return std::vector<T>(v.begin(), v.end());
}

struct Case {
  std::vector<int64_t> scope_ptr, rows;  // [n_cons + 1], [scope_ptr[n_cons]]
  std::vector<int32_t> codes;            // [n_fields, n_rows]
  std::vector<int64_t> n_codes;          // [n_fields]
  int64_t n_rows = 0, rows_max = 0;
  int top = 10;
  int64_t n_cons() const { return (int64_t)scope_ptr.size() - 1; }
  int n_fields() const { return (int)n_codes.size(); }
};

struct Result {
  std::vector<int64_t> total, missing, count;  // [n_cons], [n_cons, F], [n_cons, F, top]
  std::vector<int32_t> distinct, code;         // [n_cons, F], [n_cons, F, top]
};

// What facet_count_kernel and facet_select_kernel do, block by block.
Result run(const Case& c) {
  FcFields F;
  long long cells = 0, work = 0;
  Result r;
  const int64_t n = c.n_cons();
  const int nf = c.n_fields();
  r.total.assign((size_t)n, -7), r.missing.assign((size_t)n * nf, -7), r.distinct.assign((size_t)n * nf, -7);
  r.code.assign((size_t)n * nf * c.top, -7), r.count.assign((size_t)n * nf * c.top, -7);
  r.total = exact(r.total), r.missing = exact(r.missing), r.distinct = exact(r.distinct), r.code = exact(r.code), r.count = exact(r.count);
  const int bad = fc_check_args(c.scope_ptr.data(), c.rows.data(), n, c.rows_max, c.codes.data(), c.n_rows, nf, c.n_codes.data(),
                                c.top, r.total.data(), r.missing.data(), r.distinct.data(), r.code.data(), r.count.data(), &F, &cells);
  CHECK(bad == kFcValid, "generated arguments are valid (%s)", fc_error_text(bad));
  CHECK(fc_work_bytes(n, F, &work) && work == n * F.stride * 4, "work bytes");
  if (bad != kFcValid) return r;
  const long long tiles = fc_tiles(c.rows_max, c.n_rows), rows_max = fc_rows_max(c.rows_max, c.n_rows);
  CHECK(cells == n * tiles, "cells");
  std::vector<int> counters((size_t)(work / 4), 0);  // the memset
  // count
  for (long long cell = 0; cell < cells; ++cell)
    for (int f = 0; f < nf; ++f) {
      const long long p = cell / tiles, tile = cell - p * tiles;
      const long long b = c.scope_ptr[p];
      long long lo, hi;
      if (!fc_tile_range(c.scope_ptr[p + 1] - b, rows_max, tile, &lo, &hi)) continue;
      CHECK(lo < hi && hi - lo <= kFcTile && b + hi <= c.scope_ptr[p + 1], "a tile inside its scope");
      const long long nc = F.n_codes[f];
      int* mine = counters.data() + p * F.stride + F.off[f];
      const int32_t* col = c.codes.data() + (size_t)f * c.n_rows;
      std::vector<int> bins(fc_in_lds(nc) ? (size_t)nc + 1 : 0, 0);  // exactly the bins a block clears
      CHECK(bins.size() <= (size_t)kFcBins + 1, "the bins fit LDS");
      for (long long i = lo; i < hi; ++i) {
        const long long row = c.rows[b + i];
        if (!fc_row_ok(row, c.n_rows)) continue;
        const long long bin = fc_bin(col[row], nc);
        CHECK(bin >= 0 && bin <= nc, "a bin inside the field");
        if (fc_in_lds(nc))
          bins[(size_t)bin] += 1;
        else
          mine[bin] += 1;
      }
      for (size_t i = 0; i < bins.size(); ++i)
        if (bins[i]) mine[i] += bins[i];
    }
  // select
  for (long long pf = 0; pf < n * nf; ++pf) {
    const long long p = pf / nf;
    const int f = (int)(pf - p * nf);
    const long long nc = F.n_codes[f];
    const int* mine = counters.data() + p * F.stride + F.off[f];
    std::vector<unsigned long long> keys;
    long long sum = 0;
    for (long long code = 0; code < nc; ++code) {
      if (mine[code] > 0) keys.push_back(fc_key(mine[code], code));
      sum += mine[code];
    }
    std::sort(keys.begin(), keys.end(), std::greater<unsigned long long>());
    const int distinct = (int)keys.size();
    const int kept = distinct < c.top ? distinct : c.top;
    keys.resize((size_t)kept);
    keys = exact(keys);
    for (int j = 0; j < c.top; ++j) {
      r.code[(size_t)pf * c.top + j] = fc_slot_code(keys.data(), kept, j);
      r.count[(size_t)pf * c.top + j] = fc_slot_count(keys.data(), kept, j);
    }
    r.distinct[(size_t)pf] = distinct, r.missing[(size_t)pf] = mine[nc];
    if (f == 0) r.total[(size_t)p] = sum + mine[nc];
  }
  return r;
}

void compare(const Case& c, const char* what) {
  const Result r = run(c);
  const int nf = c.n_fields();
  for (int64_t p = 0; p < c.n_cons(); ++p) {
    long long valid = 0;
    for (int64_t i = c.scope_ptr[p]; i < c.scope_ptr[p + 1]; ++i) valid += fc_row_ok(c.rows[i], c.n_rows) ? 1 : 0;
    CHECK(r.total[p] == valid, "%s: total of constraint %lld is %lld, want %lld", what, (long long)p, (long long)r.total[p], valid);
    for (int f = 0; f < nf; ++f) {
      std::map<int, long long> by;
      long long missing = 0;
      for (int64_t i = c.scope_ptr[p]; i < c.scope_ptr[p + 1]; ++i) {
        if (!fc_row_ok(c.rows[i], c.n_rows)) continue;
        const int code = c.codes[(size_t)f * c.n_rows + c.rows[i]];
        if (code >= 0 && code < c.n_codes[f])
          by[code] += 1;
        else
          missing += 1;
      }
      std::vector<std::pair<long long, int>> order;  // (-count, code) ascending
      for (const auto& kv : by) order.push_back({-kv.second, kv.first});
      std::sort(order.begin(), order.end());
      const size_t pf = (size_t)p * nf + f;
      CHECK(r.missing[pf] == missing && r.distinct[pf] == (int)order.size(), "%s: constraint %lld field %d: missing %lld "
            "distinct %d, want %lld and %zu", what, (long long)p, f, (long long)r.missing[pf], r.distinct[pf], missing, order.size());
      for (int j = 0; j < c.top; ++j) {
        const int want_code = j < (int)order.size() ? order[j].second : -1;
        const long long want_count = j < (int)order.size() ? -order[j].first : 0;
        CHECK(r.code[pf * c.top + j] == want_code && r.count[pf * c.top + j] == want_count,
              "%s: constraint %lld field %d slot %d: (%d, %lld), want (%d, %lld)", what, (long long)p, f, j,
              r.code[pf * c.top + j], (long long)r.count[pf * c.top + j], want_code, want_count);
      }
    }
  }
}

enum Fill { kRandom, kSame, kDistinct, kNone, kStray };

// Scopes of the given lengths, each a random strictly ascending subset of [0, n_rows); one code column per n_codes entry.
Case make_case(const std::vector<long>& lens, long n_rows, const std::vector<int64_t>& n_codes, Fill fill, int top, uint64_t seed) {
  Rng g{seed};
  Case c;
  c.n_rows = n_rows, c.top = top;
  std::vector<int64_t> sp(1, 0), rows;
  for (long len : lens) {
    // every row with probability len / remaining, corrected so that exactly len are taken
    long need = len;
    for (long r = 0; r < n_rows && need > 0; ++r)
      if (g.below(n_rows - r) < need) rows.push_back(r), --need;
    sp.push_back((int64_t)rows.size());
    c.rows_max = std::max<int64_t>(c.rows_max, len);
  }
  std::vector<int32_t> codes;
  for (int64_t nc : n_codes)
    for (long r = 0; r < n_rows; ++r) {
      int code = -1;
      switch (fill) {
        case kRandom: code = nc > 0 && g.below(8) ? (int)(g.next() % (uint64_t)nc) : -1; break;
        case kSame: code = nc > 0 ? (int)(nc - 1) : -1; break;
        case kDistinct: code = (int)(r % (nc > 0 ? nc : 1)); break;
        case kNone: code = -1; break;
        case kStray: {
          const int stray[5] = {(int)nc, (int)nc + 3, -5, 0x7fffffff, (int)0x80000000u};
          code = g.below(3) == 0 ? stray[g.below(5)] : nc > 0 ? (int)g.below((long)std::min<int64_t>(nc, 1 << 30)) : -1;
          break;
        }
      }
      codes.push_back(code);
    }
  c.scope_ptr = exact(sp), c.rows = exact(rows), c.codes = exact(codes), c.n_codes = exact(n_codes);
  return c;
}

void family(const char* name, const Case& c) {
  const int before = failures;
  std::printf("facets %s:", name);
  CHECK(fc_validate(c.scope_ptr.data(), c.rows.data(), c.n_cons(), c.rows_max, c.n_rows) == kFcValid, "%s: a valid table", name);
  compare(c, name);
  std::printf(" %s\n", failures == before ? "family ok" : "family FAILED");
}

void written_out() {
  // six rows; chapter codes 0 0 1 - 1 2 (row 3 has none)
  Case c;
  c.n_rows = 6, c.top = 2, c.rows_max = 6;
  c.scope_ptr = exact(std::vector<int64_t>{0, 6, 6, 9});
  c.rows = exact(std::vector<int64_t>{0, 1, 2, 3, 4, 5, 2, 3, 5});
  c.codes = exact(std::vector<int32_t>{0, 0, 1, -1, 1, 2});
  c.n_codes = exact(std::vector<int64_t>{3});
  const Result r = run(c);
  CHECK((r.total == std::vector<int64_t>{6, 0, 3}), "totals");
  CHECK((r.missing == std::vector<int64_t>{1, 0, 1}), "missing");
  CHECK((r.distinct == std::vector<int32_t>{3, 0, 2}), "distinct");
  // the tie between codes 0 and 1 (two rows each) goes to the smaller code; code 2 falls behind the cut
  CHECK((r.code == std::vector<int32_t>{0, 1, -1, -1, 1, 2}), "codes");
  CHECK((r.count == std::vector<int64_t>{2, 2, 0, 0, 1, 1}), "counts");
  // the key: count first, then the smaller code
  CHECK(fc_key(2, 0) > fc_key(2, 1) && fc_key(3, 9) > fc_key(2, 0) && fc_key(1, 0x7ffffffe) > 0, "key order");
  CHECK(fc_key_code(fc_key(5, 123)) == 123 && fc_key_count(fc_key(5, 123)) == 5, "key round trip");
  CHECK(fc_key_count(fc_key(0x7fffffff, 0x7ffffffe)) == 0x7fffffff && fc_key_code(fc_key(0x7fffffff, 0x7ffffffe)) == 0x7ffffffe, "key limits");
  // rows outside [0, n_rows) — only the "_device" form meets them — are counted nowhere
  Case d = c;
  d.rows = exact(std::vector<int64_t>{0, 1, -1, 6, 4, 1LL << 40, 2, 3, 5});
  const Result s = run(d);
  CHECK((s.total == std::vector<int64_t>{3, 0, 3}) && (s.missing == std::vector<int64_t>{0, 0, 1}), "stray rows are not counted");
  CHECK(s.code[0] == 0 && s.count[0] == 2 && s.code[1] == 1 && s.count[1] == 1, "stray rows: the list");
  // a rows_max below a scope's length: the rows beyond it are not read
  Case e = c;
  e.rows_max = 2;
  const Result t = run(e);
  CHECK((t.total == std::vector<int64_t>{2, 0, 2}), "rows beyond rows_max are not read");
  // tiles and cells
  CHECK(fc_tiles(0, 10) == 1 && fc_tiles(1, 10) == 1 && fc_tiles(kFcTile, 1 << 20) == 1 && fc_tiles(kFcTile + 1, 1 << 20) == 2, "tiles");
  CHECK(fc_tiles(1LL << 40, 3 * kFcTile) == 3, "rows_max counts up to n_rows");
  long long lo, hi, cells;
  CHECK(!fc_tile_range(0, 10, 0, &lo, &hi) && !fc_tile_range(-3, 10, 0, &lo, &hi) && !fc_tile_range(kFcTile, kFcTile, 1, &lo, &hi),
        "tiles past the end leave");
  CHECK(fc_tile_range(kFcTile + 1, kFcTile + 1, 1, &lo, &hi) && lo == kFcTile && hi == kFcTile + 1, "the last tile's one row");
  CHECK(fc_cells(kFcMaxCells, 1, &cells) && cells == kFcMaxCells && !fc_cells(kFcMaxCells + 1, 1, &cells) &&
            !fc_cells(1LL << 20, 1 << 10, &cells) && !fc_cells(-1, 1, &cells),
        "cells");
  CHECK(fc_in_lds(kFcBins) && !fc_in_lds(kFcBins + 1), "the LDS threshold");
  std::printf("written-out ok\n");
}

void validation() {
  const std::vector<int64_t> sp = {0, 2, 2, 3}, rows = {1, 4, 0}, nc = {3, 5};
  const std::vector<int32_t> codes(10, 0);
  int64_t o64[64];
  int32_t o32[64];
  FcFields F;
  long long cells;
  auto args = [&](const void* a_sp, const void* a_rows, int64_t n_cons, int64_t rows_max, const void* a_codes, int64_t n_rows,
                  int32_t n_fields, const int64_t* a_nc, int32_t top, const void* out) {
    return fc_check_args(a_sp, a_rows, n_cons, rows_max, a_codes, n_rows, n_fields, a_nc, top, out, out, out ? o32 : nullptr,
                         out ? o32 : nullptr, out, &F, &cells);
  };
  CHECK(args(sp.data(), rows.data(), 3, 2, codes.data(), 5, 2, nc.data(), 10, o64) == kFcValid, "valid");
  CHECK(F.stride == 10 && F.off[1] == 4 && cells == 3, "layout");
  CHECK(args(sp.data(), nullptr, 0, 0, nullptr, 5, 2, nc.data(), 10, nullptr) == kFcValid, "no constraint touches no array");
  CHECK(args(nullptr, rows.data(), 3, 2, codes.data(), 5, 2, nc.data(), 10, o64) == kFcNull, "null scope_ptr");
  CHECK(args(sp.data(), nullptr, 3, 2, codes.data(), 5, 2, nc.data(), 10, o64) == kFcNull, "null rows");
  CHECK(args(sp.data(), rows.data(), 3, 2, nullptr, 5, 2, nc.data(), 10, o64) == kFcNull, "null codes");
  CHECK(args(sp.data(), rows.data(), 3, 2, codes.data(), 5, 2, nullptr, 10, o64) == kFcNull, "null n_codes");
  CHECK(args(sp.data(), rows.data(), 3, 2, codes.data(), 5, 2, nc.data(), 10, nullptr) == kFcNull, "null outputs");
  CHECK(args(sp.data(), rows.data(), -1, 2, codes.data(), 5, 2, nc.data(), 10, o64) == kFcSizes, "negative n_cons");
  CHECK(args(sp.data(), rows.data(), 3, -1, codes.data(), 5, 2, nc.data(), 10, o64) == kFcSizes, "negative rows_max");
  CHECK(args(sp.data(), rows.data(), 3, 2, codes.data(), -1, 2, nc.data(), 10, o64) == kFcSizes, "negative n_rows");
  CHECK(args(sp.data(), rows.data(), 3, 2, codes.data(), 1LL << 31, 2, nc.data(), 10, o64) == kFcSizes, "n_rows 2^31");
  CHECK(args(sp.data(), rows.data(), 3, 2, codes.data(), 5, 0, nc.data(), 10, o64) == kFcSizes, "no field");
  CHECK(args(sp.data(), rows.data(), 3, 2, codes.data(), 5, 9, nc.data(), 10, o64) == kFcSizes, "nine fields");
  CHECK(args(sp.data(), rows.data(), 3, 2, codes.data(), 5, 2, nc.data(), 0, o64) == kFcSizes, "top 0");
  CHECK(args(sp.data(), rows.data(), 3, 2, codes.data(), 5, 2, nc.data(), 65, o64) == kFcSizes, "top 65");
  const std::vector<int64_t> neg = {3, -1}, wide = {3, 1LL << 31};
  CHECK(args(sp.data(), rows.data(), 3, 2, codes.data(), 5, 2, neg.data(), 10, o64) == kFcSizes, "negative n_codes");
  CHECK(args(sp.data(), rows.data(), 3, 2, codes.data(), 5, 2, wide.data(), 10, o64) == kFcSizes, "n_codes 2^31");
  CHECK(args(sp.data(), rows.data(), kFcMaxCells + 1, 2, codes.data(), 5, 2, nc.data(), 10, o64) == kFcSizes, "too many cells");
  CHECK(args(sp.data(), rows.data(), kFcMaxCells / 2 + 1, 2, codes.data(), 5, 2, nc.data(), 10, o64) == kFcSizes,
        "too many (constraint, field) blocks");
  long long bytes;
  CHECK(fc_work_bytes(3, F, &bytes) && bytes == 120 && fc_work_bytes(0, F, &bytes) && bytes == 0 && !fc_work_bytes(-1, F, &bytes), "work");
  // the contents of a host table
  CHECK(fc_validate(sp.data(), rows.data(), 3, 2, 5) == kFcValid, "a valid table");
  CHECK(fc_validate(sp.data(), rows.data(), 0, 0, 5) == kFcValid, "no constraint");
  CHECK(fc_validate(nullptr, rows.data(), 3, 2, 5) == kFcNull && fc_validate(sp.data(), nullptr, 3, 2, 5) == kFcNull, "null tables");
  const std::vector<int64_t> from1 = {1, 2}, back = {0, 2, 1};
  CHECK(fc_validate(from1.data(), rows.data(), 1, 2, 5) == kFcPtr && fc_validate(back.data(), rows.data(), 2, 2, 5) == kFcPtr, "scope_ptr");
  CHECK(fc_validate(sp.data(), rows.data(), 3, 1, 5) == kFcRowsMax, "a scope longer than rows_max");
  const std::vector<int64_t> same = {1, 1, 0}, down = {4, 1, 0}, below = {-1, 4, 0}, past = {1, 5, 0};
  for (const auto* bad : {&same, &down, &below, &past}) CHECK(fc_validate(sp.data(), bad->data(), 3, 2, 5) == kFcRows, "rows");
  const std::vector<int64_t> empty = {0, 0};
  CHECK(fc_validate(empty.data(), nullptr, 1, 0, 5) == kFcValid, "an empty scope reads no row");
  for (int e : {kFcNull, kFcSizes, kFcPtr, kFcRowsMax, kFcRows}) CHECK(fc_error_text(e)[0] != 'o', "error text %d", e);
  std::printf("validate ok\n");
}

}  // namespace

int main() {
  const long T = kFcTile, B = kFcBins;
  const std::vector<long> lens = {0, 1, T - 1, T, T + 1, 3 * T + 7};
  const long n_rows = 4 * T + 3;
  for (int64_t nc : {(int64_t)1, (int64_t)B - 1, (int64_t)B, (int64_t)B + 1, (int64_t)3 * B + 5}) {
    char name[64];
    std::snprintf(name, sizeof name, "n_codes=%lld", (long long)nc);
    family(name, make_case(lens, n_rows, {nc}, kRandom, 10, 11 + (uint64_t)nc));
  }
  family("same", make_case(lens, n_rows, {7, B + 9}, kSame, 3, 21));
  family("distinct", make_case(lens, n_rows, {n_rows, 5}, kDistinct, 64, 22));
  family("none", make_case(lens, n_rows, {4, 0}, kNone, 5, 23));
  family("stray", make_case(lens, n_rows, {6, B + 2}, kStray, 8, 24));
  family("fields", make_case(lens, n_rows, {3, B, 2 * B + 1}, kRandom, 1, 25));
  // all 220 rows, code = row % 40: codes 0 .. 19 count 6 and the rest 5, so the cut at 7 falls among equal counts
  family("ties", make_case({220, 40}, 220, {40}, kDistinct, 7, 26));
  family("many", make_case(std::vector<long>(300, 1), 97, {5}, kRandom, 2, 27));
  written_out();
  validation();
  if (failures) {
    std::printf("%d FAILURES\n", failures);
    return 1;
  }
  std::printf("facet rule ok\n");
  return 0;
}

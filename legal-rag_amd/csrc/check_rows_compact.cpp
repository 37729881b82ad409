// Host check of the rules of amdr_dense_remove and amdr_maxsim_remove (rows_compact.hpp, and the host scan of
// compact.hpp), a program of its own (never part of the library):
//   check_rows_compact
// It compacts generated matrices on the CPU the way the kernels do — slab by slab, every "thread" a run of consecutive
// new rows whose sources come from one search and the walk (rc_src_range; rc_seg_doc + rc_seg_walk) — and compares with a
// plain filter of the rows by a removed flag.  Uniform rows, and documents of 1 / 31 / 32 / 33 / 64 / 220 token rows; the
// removal patterns first, last, one adjacent run, alternating, all but one, everything (uniform only) and a single id.
// src range by range is also compared with src row by row (rc_src), for ranges of every length the kernels use and at
// every start.  Every array is a std::vector of exactly the size the call allocates, so with the host sanitizers
// (tests/test_rows_compact_rule_host.py) an access outside one is a failure.  Then every refusal of rc_validate is
// provoked once, on arrays of exact size.
// Build: c++ -std=c++17 check_rows_compact.cpp (plain host code; no HIP header is needed).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#define AMDR_COMPACT_HOST_ONLY 1  // the host forms alone: this program has no device code
#include "compact.hpp"
#include "rows_compact.hpp"

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

struct Pattern {
  const char* name;
  std::vector<long long> ids;
};

// the removal patterns over n rows (`everything` only where the caller allows an empty result)
std::vector<Pattern> patterns(long n, bool everything) {
  std::vector<Pattern> p;
  p.push_back({"first", {0}});
  p.push_back({"last", {n - 1}});
  if (n >= 8) {
    Pattern run{"one adjacent run", {}};
    for (long i = n / 3; i < n / 3 + 5; ++i) run.ids.push_back(i);
    p.push_back(run);
  }
  Pattern alt{"alternating", {}};
  for (long i = 1; i < n; i += 2) alt.ids.push_back(i);
  if (!alt.ids.empty()) p.push_back(alt);
  if (n >= 2) {
    Pattern abo{"all but one", {}};
    for (long i = 0; i < n; ++i)
      if (i != n / 2) abo.ids.push_back(i);
    p.push_back(abo);
  }
  if (everything) {
    Pattern all{"everything", {}};
    for (long i = 0; i < n; ++i) all.ids.push_back(i);
    p.push_back(all);
  }
  p.push_back({"a single id", {n / 2}});
  return p;
}

std::vector<long long> plain_survivors(long n, const std::vector<long long>& rm) {
  std::vector<char> gone((size_t)n, 0);
  for (long long r : rm) gone[(size_t)r] = 1;
  std::vector<long long> keep;
  for (long i = 0; i < n; ++i)
    if (!gone[(size_t)i]) keep.push_back(i);
  return keep;
}

// src over [0, n_new) cut into ranges of `run` rows (one search, then the walk), against src row by row
void check_ranges(const char* what, const std::vector<long long>& rm, long n_new, const std::vector<long long>& keep) {
  const long n_rm = (long)rm.size();
  for (long j = 0; j < n_new; ++j)
    CHECK(rc_src(rm.data(), n_rm, j) == keep[(size_t)j], "%s: src(%ld) = %lld, expected %lld", what, j,
          rc_src(rm.data(), n_rm, j), keep[(size_t)j]);
  for (long run : {1L, 3L, 4L, 8L, 64L, 2048L}) {
    std::vector<long long> got((size_t)n_new, -1);
    for (long j0 = 0; j0 < n_new; j0 += run) {
      const long cnt = std::min(run, n_new - j0);
      std::vector<long long> out((size_t)cnt, -1);  // exactly the range
      rc_src_range(rm.data(), n_rm, j0, cnt, out.data());
      std::copy(out.begin(), out.end(), got.begin() + j0);
    }
    CHECK(got == keep, "%s: src in ranges of %ld differs from src row by row", what, run);
  }
  // a walk may start from any earlier row's answer, not only the previous row's
  if (n_new > 0) {
    const long r0 = rc_removed_upto(rm.data(), n_rm, 0);
    for (long j = 0; j < n_new; j += 7)
      CHECK(j + rc_walk(rm.data(), n_rm, r0, j) == keep[(size_t)j], "%s: the walk from row 0 to row %ld", what, j);
  }
}

// the uniform kernel's slabs: rows_per_slab rows a block, `per` consecutive rows a thread
void uniform_case(long n, int units_per_row, const Pattern& p) {
  const std::string what = "uniform n=" + std::to_string(n) + " units=" + std::to_string(units_per_row) + " " + p.name;
  const std::vector<long long>& rm = p.ids;
  const long n_rm = (long)rm.size(), n_new = n - n_rm;
  CHECK(rc_validate((const int64_t*)rm.data(), n_rm, n) == kRcOk, "%s: a generated list is refused", what.c_str());
  std::vector<uint32_t> X((size_t)n * units_per_row * 4);
  for (size_t i = 0; i < X.size(); ++i) X[i] = (uint32_t)(i * 2654435761u + 17u);
  const std::vector<long long> keep = plain_survivors(n, rm);
  CHECK((long)keep.size() == n_new, "%s: %zu survivors", what.c_str(), keep.size());
  std::vector<uint32_t> want;
  for (long long s : keep) want.insert(want.end(), X.begin() + s * units_per_row * 4, X.begin() + (s + 1) * units_per_row * 4);
  check_ranges(what.c_str(), rm, n_new, keep);
  constexpr int kThreads = 256, kSlabUnits = 2048;
  const int rows_per_slab = kSlabUnits / units_per_row, per = (rows_per_slab + kThreads - 1) / kThreads;
  std::vector<uint32_t> got((size_t)n_new * units_per_row * 4, 0xdeadbeefu);
  for (long j0 = 0; j0 < n_new; j0 += rows_per_slab) {
    const int rows = (int)std::min<long>(rows_per_slab, n_new - j0);
    std::vector<long long> row_src((size_t)rows, -1);
    for (int t = 0; t < kThreads; ++t) {
      const int a = t * per;
      if (a < rows) rc_src_range(rm.data(), n_rm, j0 + a, std::min(per, rows - a), row_src.data() + a);
    }
    for (int u = 0; u < rows * units_per_row; ++u) {
      const int row = u / units_per_row, c = u - row * units_per_row;
      const long long s = row_src.at((size_t)row);
      CHECK(s >= 0 && s < n, "%s: source row %lld", what.c_str(), s);
      for (int w = 0; w < 4; ++w)
        got.at((size_t)((j0 * units_per_row + u) * 4 + w)) = X.at((size_t)((s * units_per_row + c) * 4 + w));
    }
  }
  CHECK(got == want, "%s: compacted rows differ", what.c_str());
  std::printf("uniform ok: %s: %ld -> %ld rows\n", what.c_str(), n, n_new);
}

// the segmented form: the doc_ptr rebuild, then slabs of 64 token rows, 4 consecutive rows a thread
void segment_case(const std::vector<long>& lens, const Pattern& p) {
  const long n = (long)lens.size();
  const std::string what = "segments n=" + std::to_string(n) + " " + p.name;
  const std::vector<long long>& rm = p.ids;
  const long n_rm = (long)rm.size(), n_new = n - n_rm;
  CHECK(rc_validate((const int64_t*)rm.data(), n_rm, n) == kRcOk && n_new >= 1, "%s: a generated list is refused", what.c_str());
  std::vector<long long> ptr((size_t)n + 1, 0);
  for (long i = 0; i < n; ++i) ptr[(size_t)i + 1] = ptr[(size_t)i] + lens[(size_t)i];
  std::vector<long long> tok((size_t)ptr.back());  // a token row's identity
  for (size_t i = 0; i < tok.size(); ++i) tok[i] = (long long)(i * 1000003u + 5u);
  const std::vector<long long> keep = plain_survivors(n, rm);
  std::vector<long long> want_ptr(1, 0), want_tok;
  for (long long s : keep) {
    want_tok.insert(want_tok.end(), tok.begin() + ptr[(size_t)s], tok.begin() + ptr[(size_t)s + 1]);
    want_ptr.push_back((long long)want_tok.size());
  }
  check_ranges(what.c_str(), rm, n_new, keep);
  std::vector<long long> len((size_t)n_new, -1), start((size_t)n_new, -1), new_ptr((size_t)n_new + 1, -1);
  for (long j = 0; j < n_new; ++j) rc_seg_entry(ptr.data(), rc_src(rm.data(), n_rm, j), &len[(size_t)j], &start[(size_t)j]);
  compact_scan_host(len.data(), n_new, new_ptr.data());
  CHECK(new_ptr == want_ptr, "%s: new doc_ptr differs", what.c_str());
  const long long rows_new = new_ptr.back();
  constexpr int kSlabRows = 64, kRun = 4;
  std::vector<long long> got((size_t)rows_new, -1);
  for (long long t0 = 0; t0 < rows_new; t0 += kSlabRows) {
    const int rows = (int)std::min<long long>(kSlabRows, rows_new - t0);
    std::vector<long long> row_src((size_t)rows, -1);
    for (int a = 0; a < rows; a += kRun) {
      long j = rc_seg_doc(new_ptr.data(), n_new, t0 + a);
      for (int i = 0; i < kRun && a + i < rows; ++i) {
        j = rc_seg_walk(new_ptr.data(), n_new, j, t0 + a + i);
        CHECK(j == rc_seg_doc(new_ptr.data(), n_new, t0 + a + i), "%s: the walk and the search disagree at row %lld",
              what.c_str(), t0 + a + i);
        row_src.at((size_t)(a + i)) = rc_seg_src(new_ptr.data(), start.data(), j, t0 + a + i);
      }
    }
    for (int r = 0; r < rows; ++r) got.at((size_t)(t0 + r)) = tok.at((size_t)row_src[(size_t)r]);
  }
  CHECK(got == want_tok, "%s: compacted token rows differ", what.c_str());
  std::printf("segments ok: %s: %ld -> %ld documents, %lld -> %lld rows\n", what.c_str(), n, n_new, ptr.back(), rows_new);
}

void validate_cases() {
  const int64_t ok[2] = {1, 3}, desc[2] = {3, 1}, dup[2] = {3, 3}, neg[2] = {-1, 3}, top[2] = {1, 5};
  CHECK(rc_validate(ok, 2, 5) == kRcOk, "the good list");
  CHECK(rc_validate(ok, 0, 5) == kRcOk && rc_validate(nullptr, 0, 5) == kRcOk, "the empty list reads nothing");
  CHECK(rc_validate(nullptr, 2, 5) == kRcNull, "null list");
  CHECK(rc_validate(ok, -1, 5) == kRcSizes, "n_remove < 0");
  CHECK(rc_validate(ok, 2, 1) == kRcSizes, "n_remove > n");
  CHECK(rc_validate(desc, 2, 5) == kRcIdOrder, "descending ids");
  CHECK(rc_validate(dup, 2, 5) == kRcIdOrder, "a repeated id");
  CHECK(rc_validate(neg, 2, 5) == kRcIdRange, "id -1");
  CHECK(rc_validate(top, 2, 5) == kRcIdRange, "id n");
  const int64_t all[3] = {0, 1, 2};
  CHECK(rc_validate(all, 3, 3) == kRcOk, "everything (the callers decide whether an empty result is allowed)");
  std::printf("validate ok\n");
}

}  // namespace

int main() {
  // uniform rows: 16 B (2 048 rows a slab, 8 a thread), 48 B (682 rows a slab, 3 a thread: not a power of two), 512 B and
  // 4 096 B (8 rows a slab); fewer rows than a slab, exactly one slab's, and several slabs with a short last one
  const struct { long n; int units; } shapes[] = {{37, 1}, {2048, 1}, {5000, 1}, {300, 3}, {1500, 3}, {300, 32}, {300, 256}, {37, 256}, {1, 8}};
  for (const auto& s : shapes)
    for (const Pattern& p : patterns(s.n, true)) uniform_case(s.n, s.units, p);
  // segments: the lengths in turn, 40 documents (the last one 33 rows) and a store of one-row documents
  const long cycle[6] = {1, 31, 32, 33, 64, 220};
  std::vector<long> lens;
  for (int i = 0; i < 40; ++i) lens.push_back(cycle[i % 6]);
  lens.back() = 33;
  for (const Pattern& p : patterns((long)lens.size(), false)) segment_case(lens, p);
  std::vector<long> ones(300, 1);
  for (const Pattern& p : patterns(300, false)) segment_case(ones, p);
  std::vector<long> two = {220, 1};
  segment_case(two, {"first", {0}});
  segment_case(two, {"last", {1}});
  validate_cases();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("rows compact rule ok\n");
  return 0;
}

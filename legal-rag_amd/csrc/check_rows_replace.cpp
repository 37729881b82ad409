// Host check of the replace rules of rows_compact.hpp (rs_*: amdr_dense_replace, amdr_maxsim_replace), a program of its
// own (never part of the library):
//   check_rows_replace
// It edits generated stores on the CPU the way the kernels do and compares with a brute-force edit, byte for byte.
// Uniform rows: staged row i written over row replace_ids[i], unit by unit as rows_scatter_kernel divides them.  Token
// stores: the doc_ptr rebuild (rs_seg_entry per document, compact_scan_host), then slabs of 64 token rows, 4 consecutive
// rows a thread (rc_seg_doc, rc_seg_walk, rs_seg_src), each row copied from the old store or from the staged rows.
// Documents of 1 / 2 / 31 / 32 / 33 / 64 / 220 token rows grow, shrink and keep their length; the patterns are the first,
// the last, one adjacent run, alternating, all but one, every document and a single id.  Every array is a std::vector of
// exactly the size the call allocates, so with the host sanitizers (tests/test_rows_replace_rule_host.py) an access
// outside one is a failure.
// Build: c++ -std=c++17 check_rows_replace.cpp (plain host code; no HIP header is needed).
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

std::vector<Pattern> patterns(long n) {
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
  Pattern all{"every row", {}};
  for (long i = 0; i < n; ++i) all.ids.push_back(i);
  p.push_back(all);
  p.push_back({"a single id", {n / 2}});
  return p;
}

constexpr int kWords = 4;  // a 16-byte unit

void find_case(long n, const Pattern& p) {
  std::vector<long> where((size_t)n, -1);
  for (size_t i = 0; i < p.ids.size(); ++i) where[(size_t)p.ids[i]] = (long)i;
  for (long j = 0; j < n; ++j)
    CHECK(rs_find(p.ids.data(), (long)p.ids.size(), j) == where[(size_t)j], "n=%ld %s: rs_find(%ld)", n, p.name, j);
}

// the dense form: the scatter in place
void uniform_case(long n, int units_per_row, const Pattern& p) {
  const std::string what = "uniform n=" + std::to_string(n) + " units=" + std::to_string(units_per_row) + " " + p.name;
  const long n_rep = (long)p.ids.size();
  CHECK(rc_validate((const int64_t*)p.ids.data(), n_rep, n) == kRcOk, "%s: a generated list is refused", what.c_str());
  const size_t row = (size_t)units_per_row * kWords;
  std::vector<uint32_t> X((size_t)n * row), R((size_t)n_rep * row);
  for (size_t i = 0; i < X.size(); ++i) X[i] = (uint32_t)(i * 2654435761u + 17u);
  for (size_t i = 0; i < R.size(); ++i) R[i] = (uint32_t)(i * 40503u + 0x80000000u);
  std::vector<uint32_t> want = X;
  for (long i = 0; i < n_rep; ++i) std::copy(R.begin() + i * row, R.begin() + (i + 1) * row, want.begin() + p.ids[(size_t)i] * row);
  const long long units = (long long)n_rep * units_per_row;
  for (long long u = 0; u < units; ++u) {  // rows_scatter_kernel: unit u of the staged rows
    const long long i = u / units_per_row;
    const long long dst = p.ids.at((size_t)i) * units_per_row + (u - i * units_per_row);
    for (int w = 0; w < kWords; ++w) X.at((size_t)(dst * kWords + w)) = R.at((size_t)(u * kWords + w));
  }
  CHECK(X == want, "%s: scattered rows differ", what.c_str());
  std::printf("uniform ok: %s: %ld of %ld rows\n", what.c_str(), n_rep, n);
}

// the token store: grow = how the new length of a replaced document follows from its old one
void segment_case(const std::vector<long>& lens, const std::vector<long>& new_lens, const Pattern& p, const char* how) {
  const long n = (long)lens.size(), n_rep = (long)p.ids.size();
  const std::string what = std::string("segments n=") + std::to_string(n) + " " + p.name + ", " + how;
  constexpr int kRow = 32 * kWords;  // a token row: 32 units
  std::vector<long long> ptr((size_t)n + 1, 0), add_ptr((size_t)n_rep + 1, 0);
  for (long i = 0; i < n; ++i) ptr[(size_t)i + 1] = ptr[(size_t)i] + lens[(size_t)i];
  for (long i = 0; i < n_rep; ++i) add_ptr[(size_t)i + 1] = add_ptr[(size_t)i] + new_lens[(size_t)(p.ids[(size_t)i] % (long long)new_lens.size())];
  std::vector<uint32_t> D((size_t)ptr.back() * kRow), A((size_t)add_ptr.back() * kRow);
  for (size_t i = 0; i < D.size(); ++i) D[i] = (uint32_t)(i * 2654435761u + 17u);
  for (size_t i = 0; i < A.size(); ++i) A[i] = (uint32_t)(i * 40503u + 0x80000000u);
  // the brute-force edit
  std::vector<long long> want_ptr(1, 0);
  std::vector<uint32_t> want;
  for (long j = 0, i = 0; j < n; ++j) {
    if (i < n_rep && p.ids[(size_t)i] == j) {
      want.insert(want.end(), A.begin() + add_ptr[(size_t)i] * kRow, A.begin() + add_ptr[(size_t)i + 1] * kRow);
      ++i;
    } else {
      want.insert(want.end(), D.begin() + ptr[(size_t)j] * kRow, D.begin() + ptr[(size_t)j + 1] * kRow);
    }
    want_ptr.push_back((long long)(want.size() / kRow));
  }
  // the kernels' way
  std::vector<long long> len((size_t)n), start((size_t)n), new_ptr((size_t)n + 1);
  for (long j = 0; j < n; ++j)
    rs_seg_entry(ptr.data(), add_ptr.data(), p.ids.data(), n_rep, j, &len[(size_t)j], &start[(size_t)j]);
  compact_scan_host(len.data(), n, new_ptr.data());
  CHECK(new_ptr == want_ptr, "%s: doc_ptr differs", what.c_str());
  const long long rows_new = new_ptr.back();
  constexpr int kThreads = 256, kSlabRows = 64, kRun = 4;
  std::vector<uint32_t> got((size_t)rows_new * kRow, 0xdeadbeefu);
  for (long long t0 = 0; t0 < rows_new; t0 += kSlabRows) {
    const int rows = (int)std::min<long long>(kSlabRows, rows_new - t0);
    std::vector<long long> row_src((size_t)rows, 0);
    for (int t = 0; t < kThreads; ++t) {
      const int a = t * kRun;
      if (a >= rows) continue;
      long j = rc_seg_doc(new_ptr.data(), n, t0 + a);
      for (int i = 0; i < kRun && a + i < rows; ++i) {
        j = rc_seg_walk(new_ptr.data(), n, j, t0 + a + i);
        row_src.at((size_t)(a + i)) = rs_seg_src(new_ptr.data(), start.data(), j, t0 + a + i);
      }
    }
    for (int r = 0; r < rows; ++r) {
      const long long s = row_src[(size_t)r];
      const std::vector<uint32_t>& from = s >= 0 ? D : A;
      const long long srow = s >= 0 ? s : ~s;
      CHECK(srow >= 0 && (size_t)(srow + 1) * kRow <= from.size(), "%s: source row %lld", what.c_str(), s);
      for (int w = 0; w < kRow; ++w) got.at((size_t)((t0 + r) * kRow + w)) = from.at((size_t)(srow * kRow + w));
    }
  }
  CHECK(got == want, "%s: spliced rows differ", what.c_str());
  std::printf("segments ok: %s: %ld of %ld documents, %lld -> %lld token rows\n", what.c_str(), n_rep, n, ptr.back(), rows_new);
}

}  // namespace

int main() {
  for (long n : {1L, 2L, 31L, 32L, 33L, 65L, 1025L})
    for (const Pattern& p : patterns(n)) {
      find_case(n, p);
      for (int units : {1, 32, 192}) uniform_case(n, units, p);
    }
  const std::vector<long> edge = {1, 2, 31, 32, 33, 64, 220};
  for (long n : {1L, 7L, 40L, 300L}) {
    std::vector<long> lens;
    for (long i = 0; i < n; ++i) lens.push_back(edge[(size_t)(i * 5 % 7)]);
    for (const Pattern& p : patterns(n)) {
      segment_case(lens, {1, 2, 31, 32, 33, 64, 220}, p, "new lengths in another order");  // grow, shrink and keep
      segment_case(lens, {1}, p, "one-token replacements");
      segment_case(lens, {220}, p, "long replacements");
      segment_case(lens, {33, 32}, p, "around a tile of 32");
    }
  }
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("rows replace rule ok\n");
  return 0;
}

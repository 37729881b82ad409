// Host check of the rules of amdr_term_scope (term_scope_rule.hpp, and the host scans of compact.hpp), a program of its
// own (never part of the library):
//   check_term_scope
// It resolves generated constraints over generated postings on the CPU the way the kernels do — per constraint the driver,
// then tile by tile of kTsTile candidates the keep flags (ts_qualifies), one count per (constraint, tile), ONE scan over
// the flattened counts, the rank inside the tile, the write clamped to rows_cap and the status words — and compares with a
// plain filter: every document of the corpus tested against a dense term x document bit matrix, which shares nothing with
// posting_has or the driver choice.  Families: MUST only, ANY only (the iota form), NOT only, all three, multi-token
// groups, a repeated term, unknown terms in each kind, a base scope shorter / longer than the rarest list, driver ties,
// and the two overflow bounds one below what is needed.  Every array is a std::vector of exactly the size the call
// promises, so with the host sanitizers (tests/test_term_scope_rule_host.py) an access outside one is a failure.  Then
// every refusal of ts_validate is provoked once, on arrays of exact size.
// Build: c++ -std=c++17 check_term_scope.cpp (plain host code; no HIP header is needed).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#define AMDR_COMPACT_HOST_ONLY 1  // the host forms alone: this program has no device code
#include "compact.hpp"
#include "term_scope_rule.hpp"

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
  bool chance(double p) { return (next() & 0xffffff) < p * 0x1000000; }
};

struct Corpus {
  long n_docs, n_terms;
  std::vector<std::vector<char>> has;  // [term][doc]: the plain filter's own form
  std::vector<long long> term_ptr;
  std::vector<int> post_doc;
};

// term t holds a document with probability dens[t]; term 0 holds every document, term 1 none, term 2 document 0 and the
// last one alone
Corpus make_corpus(long n_docs, const std::vector<double>& dens, uint64_t seed) {
  Corpus c;
  c.n_docs = n_docs;
  c.n_terms = (long)dens.size();
  Rng r{seed};
  c.has.assign(c.n_terms, std::vector<char>(n_docs, 0));
  for (long t = 0; t < c.n_terms; ++t)
    for (long d = 0; d < n_docs; ++d)
      c.has[t][d] = t == 0 ? 1 : t == 1 ? 0 : t == 2 ? (d == 0 || d == n_docs - 1) : r.chance(dens[t]);
  c.term_ptr.assign(c.n_terms + 1, 0);
  for (long t = 0; t < c.n_terms; ++t) {
    for (long d = 0; d < n_docs; ++d)
      if (c.has[t][d]) c.post_doc.push_back((int)d);
    c.term_ptr[t + 1] = (long long)c.post_doc.size();
  }
  return c;
}

struct Group {
  int kind;
  std::vector<int> terms;
};
struct Constraint {
  std::vector<Group> groups;
  int base;  // -1: none
};
struct Batch {
  std::vector<Constraint> cons;
  std::vector<std::vector<long long>> bases;
};

struct Packed {
  std::vector<long long> grp_ptr, grp_term_ptr, base_ptr, base_rows;
  std::vector<int> grp_kind, grp_terms, cons_base;
  TsCons view(int n_base) const {
    return TsCons{grp_ptr.data(), grp_kind.data(), grp_term_ptr.data(), grp_terms.data(), base_ptr.data(), base_rows.data(),
                  cons_base.data(), n_base};
  }
};
Packed pack(const Batch& b) {
  Packed p;
  p.grp_ptr.push_back(0);
  p.grp_term_ptr.push_back(0);
  for (const Constraint& c : b.cons) {
    for (const Group& g : c.groups) {
      p.grp_kind.push_back(g.kind);
      for (int t : g.terms) p.grp_terms.push_back(t);
      p.grp_term_ptr.push_back((long long)p.grp_terms.size());
    }
    p.grp_ptr.push_back((long long)p.grp_kind.size());
    p.cons_base.push_back(c.base);
  }
  p.base_ptr.push_back(0);
  for (const auto& rows : b.bases) {
    for (long long r : rows) p.base_rows.push_back(r);
    p.base_ptr.push_back((long long)p.base_rows.size());
  }
  return p;
}

// the plain filter
bool plain_group(const Corpus& c, const Group& g, long d) {
  for (int t : g.terms)
    if (t < 0 || t >= c.n_terms || !c.has[t][d]) return false;
  return true;
}
std::vector<long long> plain(const Corpus& c, const Batch& b, const Constraint& k) {
  std::vector<long long> out;
  for (long d = 0; d < c.n_docs; ++d) {
    bool ok = true, any_seen = false, any_ok = false;
    for (const Group& g : k.groups) {
      const bool has = plain_group(c, g, d);
      if (g.kind == kTsMust && !has) ok = false;
      if (g.kind == kTsNot && has) ok = false;
      if (g.kind == kTsAny) any_seen = true, any_ok = any_ok || has;
    }
    if (any_seen && !any_ok) ok = false;
    if (ok && k.base >= 0) ok = std::binary_search(b.bases[k.base].begin(), b.bases[k.base].end(), (long long)d);
    if (ok) out.push_back(d);
  }
  return out;
}

struct Result {
  std::vector<long long> scope_ptr, rows;
  std::vector<int> status;
};

// the three launches on the CPU, on arrays of the sizes amdr_term_scope_plan / the caller promise
Result resolve(const Corpus& c, const Packed& p, int n_base, long n_cons, long long cand_max, long long rows_cap) {
  const TsIndex I{c.term_ptr.data(), c.post_doc.data(), c.n_terms, c.n_docs};
  const TsCons C = p.view(n_base);
  const long long tiles = ts_tiles(cand_max);
  std::vector<long long> counts((size_t)n_cons * tiles), offsets((size_t)n_cons * tiles + 1);
  std::vector<unsigned char> keep((size_t)n_cons * tiles * kTsTile, 0);
  Result r;
  r.scope_ptr.assign(n_cons + 1, -1);
  r.rows.assign((size_t)rows_cap, -1);
  r.status.assign(n_cons, -1);
  for (long k = 0; k < n_cons; ++k) {  // count
    const TsDriver D = ts_driver(I, C, k);
    const bool over = D.len > cand_max;
    r.status[k] = over ? kTsCandOverflow : kTsOk;
    for (long long tile = 0; tile < tiles; ++tile) {
      const size_t cell = (size_t)k * tiles + tile;
      long long cnt = 0;
      if (!over)
        for (long long i = tile * kTsTile; i < (tile + 1) * kTsTile && i < D.len; ++i) {
          const bool q = ts_qualifies(I, C, k, D, ts_candidate(I, C, D, i));
          keep[cell * kTsTile + (size_t)(i - tile * kTsTile)] = q;
          cnt += q;
        }
      counts[cell] = cnt;
    }
  }
  compact_scan_host(counts.data(), (long)(n_cons * tiles), offsets.data());  // scan
  for (long k = 0; k < n_cons; ++k) {  // write
    const TsDriver D = ts_driver(I, C, k);
    const long long b = offsets[(size_t)k * tiles], e = offsets[(size_t)(k + 1) * tiles];
    r.scope_ptr[k] = std::min(b, rows_cap);
    if (k == n_cons - 1) r.scope_ptr[n_cons] = std::min(e, rows_cap);
    if (e > b && e > rows_cap) r.status[k] = kTsRowsOverflow;
    if (D.len > cand_max) continue;
    for (long long tile = 0; tile < tiles && tile * kTsTile < D.len; ++tile) {
      const size_t cell = (size_t)k * tiles + tile;
      std::vector<unsigned short> rank(kTsTile);
      compact_tile_scan_host(&keep[cell * kTsTile], kTsTile, rank.data());
      for (int j = 0; j < kTsTile; ++j) {
        if (!keep[cell * kTsTile + j]) continue;
        const long long at = offsets[cell] + rank[j];
        if (at < rows_cap) r.rows[(size_t)at] = ts_candidate(I, C, D, tile * kTsTile + j);
      }
    }
  }
  return r;
}

// a family: resolved with exact bounds and compared with the plain filter; then with each bound one below
void family(const char* name, const Corpus& c, const Batch& b) {
  const Packed p = pack(b);
  const int n_base = (int)b.bases.size();
  const long n_cons = (long)b.cons.size();
  CHECK(ts_validate((const int64_t*)p.grp_ptr.data(), p.grp_kind.data(), (const int64_t*)p.grp_term_ptr.data(),
                    (const int64_t*)p.base_ptr.data(), (const int64_t*)p.base_rows.data(), p.cons_base.data(), n_base, n_cons,
                    (int64_t)p.grp_kind.size(), c.n_docs) == kTsValid,
        "%s: valid operands refused", name);
  const TsIndex I{c.term_ptr.data(), c.post_doc.data(), c.n_terms, c.n_docs};
  const TsCons C = p.view(n_base);
  long long cand_max = 0, rows_cap = 0, total = 0;
  long longest = 0;
  std::vector<std::vector<long long>> want;
  bool proper = false;  // some constraint is non-empty and smaller than the corpus
  for (long k = 0; k < n_cons; ++k) {
    const long long len = ts_driver(I, C, k).len;
    if (len > cand_max) cand_max = len, longest = k;
    rows_cap += len;
    want.push_back(plain(c, b, b.cons[k]));
    CHECK((long long)want[k].size() <= len, "%s: constraint %ld: %zu rows from %lld candidates", name, k, want[k].size(), len);
    total += (long long)want[k].size();
    proper = proper || (!want[k].empty() && (long)want[k].size() < c.n_docs);
  }
  CHECK(proper, "%s: no constraint is non-empty and smaller than the corpus", name);
  auto compare = [&](const Result& r, long skip_from, long empty_one, const char* what) {
    for (long k = 0; k < n_cons; ++k) {
      if (k == empty_one) {
        CHECK(r.scope_ptr[k + 1] == r.scope_ptr[k] && r.status[k] == kTsCandOverflow, "%s (%s): constraint %ld not emptied", name, what, k);
        continue;
      }
      if (skip_from >= 0 && k >= skip_from) continue;
      const std::vector<long long> got(r.rows.begin() + r.scope_ptr[k], r.rows.begin() + r.scope_ptr[k + 1]);
      CHECK(got == want[k] && r.status[k] == kTsOk, "%s (%s): constraint %ld differs (%zu rows, %zu wanted, status %d)", name,
            what, k, got.size(), want[k].size(), r.status[k]);
    }
  };
  const Result exact = resolve(c, p, n_base, n_cons, cand_max, rows_cap);
  compare(exact, -1, -1, "exact bounds");
  CHECK(exact.scope_ptr[n_cons] == total, "%s: total %lld, wanted %lld", name, exact.scope_ptr[n_cons], total);
  const Result tight = resolve(c, p, n_base, n_cons, cand_max, total);  // rows_cap = what is written: nothing dropped
  compare(tight, -1, -1, "rows_cap = total");
  if (cand_max > 0) {  // one candidate short: exactly the first longest constraint is emptied, the others are exact
    bool unique = true;
    for (long k = 0; k < n_cons; ++k) unique = unique && (k == longest || ts_driver(I, C, k).len < cand_max);
    if (unique) compare(resolve(c, p, n_base, n_cons, cand_max - 1, rows_cap), -1, longest, "cand_max - 1");
  }
  if (total > 0) {  // one row short: status 2 from the first constraint that does not fit, the ones before it exact
    const Result r = resolve(c, p, n_base, n_cons, cand_max, total - 1);
    long first = 0;
    while (exact.scope_ptr[first + 1] <= total - 1) ++first;
    compare(r, first, -1, "rows_cap - 1");
    for (long k = first; k < n_cons; ++k)
      CHECK(r.status[k] == (want[k].empty() ? kTsOk : kTsRowsOverflow), "%s: rows_cap - 1: status[%ld] = %d", name, k, r.status[k]);
    CHECK(r.scope_ptr[n_cons] == total - 1, "%s: rows_cap - 1: scope_ptr not clamped", name);
    const std::vector<long long> head(r.rows.begin() + r.scope_ptr[first], r.rows.end());
    CHECK(std::equal(head.begin(), head.end(), want[first].begin()), "%s: rows_cap - 1: the rows that fit differ", name);
  }
  std::printf("%s: %ld constraints, %lld rows, longest driver %lld: family ok\n", name, n_cons, total, cand_max);
}

Constraint cons(std::vector<Group> g, int base = -1) { return Constraint{std::move(g), base}; }

void validation() {
  // one valid set: two constraints, three groups, one base scope of rows {1, 4} in a corpus of 6
  const std::vector<int64_t> gp{0, 2, 3}, gtp{0, 1, 3, 4}, bp{0, 2}, br{1, 4};
  const std::vector<int32_t> gk{0, 1, 2}, cb{0, -1};
  auto run = [&](const std::vector<int64_t>& a, const std::vector<int32_t>& k, const std::vector<int64_t>& t,
                 const std::vector<int64_t>& p, const std::vector<int64_t>& r, const std::vector<int32_t>& c) {
    return ts_validate(a.data(), k.data(), t.data(), p.data(), r.data(), c.data(), (int64_t)p.size() - 1, (int64_t)c.size(),
                       (int64_t)k.size(), 6);
  };
  CHECK(run(gp, gk, gtp, bp, br, cb) == kTsValid, "valid set refused");
  CHECK(run({1, 2, 3}, gk, gtp, bp, br, cb) == kTsGrpPtr, "grp_ptr[0] != 0");
  CHECK(run({0, 3, 2}, gk, gtp, bp, br, cb) == kTsGrpPtr, "grp_ptr not monotone");
  CHECK(run({0, 2, 2}, gk, gtp, bp, br, cb) == kTsGrpPtr, "grp_ptr does not end at n_groups");
  CHECK(run(gp, gk, {1, 1, 3, 4}, bp, br, cb) == kTsTermPtr, "grp_term_ptr[0] != 0");
  CHECK(run(gp, gk, {0, 3, 1, 4}, bp, br, cb) == kTsTermPtr, "grp_term_ptr not monotone");
  CHECK(run(gp, gk, {0, 1, 1, 4}, bp, br, cb) == kTsEmptyGroup, "an empty group");
  CHECK(run(gp, {0, 3, 2}, gtp, bp, br, cb) == kTsKind, "kind 3");
  CHECK(run(gp, {0, -1, 2}, gtp, bp, br, cb) == kTsKind, "kind -1");
  CHECK(run(gp, gk, gtp, {-1, 2}, br, cb) == kTsBasePtr, "base_ptr negative");
  CHECK(run(gp, gk, gtp, {0, 2, 1}, br, {0, 1}) == kTsBasePtr, "base_ptr not monotone");
  CHECK(run(gp, gk, gtp, bp, {1, 6}, cb) == kTsBaseRange, "a base row = n_docs");
  CHECK(run(gp, gk, gtp, bp, {-1, 4}, cb) == kTsBaseRange, "a base row < 0");
  CHECK(run(gp, gk, gtp, bp, {4, 4}, cb) == kTsBaseOrder, "base rows repeated");
  CHECK(run(gp, gk, gtp, bp, {4, 1}, cb) == kTsBaseOrder, "base rows descending");
  CHECK(run(gp, gk, gtp, bp, br, {1, -1}) == kTsConsBase, "cons_base = n_base");
  CHECK(run(gp, gk, gtp, bp, br, {0, -2}) == kTsConsBase, "cons_base = -2");
  CHECK(ts_validate(gp.data(), gk.data(), gtp.data(), bp.data(), br.data(), cb.data(), 1, -1, 3, 6) == kTsSizes, "n_cons < 0");
  CHECK(ts_validate(nullptr, gk.data(), gtp.data(), bp.data(), br.data(), cb.data(), 1, 2, 3, 6) == kTsNull, "null grp_ptr");
  CHECK(ts_validate(gp.data(), gk.data(), gtp.data(), bp.data(), nullptr, cb.data(), 1, 2, 3, 6) == kTsNull, "null base_rows");
  for (int e = kTsValid; e <= kTsConsBase; ++e) CHECK(ts_error_text(e)[0] != 0, "error text %d", e);
  // posting_has never dereferences an unknown term: the arrays are null
  CHECK(!posting_has(nullptr, nullptr, 5, -1, 0) && !posting_has(nullptr, nullptr, 5, 5, 0), "unknown term");
  std::printf("validate ok\n");
}

}  // namespace

int main() {
  // terms: 0 every document, 1 none, 2 {first, last}, 3 .. dense to rare
  const std::vector<double> dens{1, 0, 0, 0.6, 0.5, 0.3, 0.25, 0.1, 0.05, 0.02, 0.5, 0.5};
  const int M = kTsMust, A = kTsAny, N = kTsNot;
  for (long n : {1L, 2L, 1023L, 1024L, 1025L, 2049L, 4100L}) {
    const Corpus c = make_corpus(n, dens, 0x9e3779b97f4a7c15ull + (uint64_t)n);
    const std::string at = " n=" + std::to_string(n);
    std::vector<long long> every(n), odd, few;
    for (long d = 0; d < n; ++d) every[d] = d;
    for (long d = 1; d < n; d += 2) odd.push_back(d);
    for (long d = 0; d < n; d += 97) few.push_back(d);
    if (few.back() != n - 1) few.push_back(n - 1);
    if (n < 1023) {  // the tiny corpora: the iota form and the edges alone (term 0 keeps a family "proper" only from n = 2)
      Batch b;
      b.cons = {cons({{A, {0}}}), cons({{M, {2}}}), cons({{N, {1}}}), cons({{M, {0}}, {N, {2}}})};
      if (n >= 2) b.bases = {{n - 1}}, b.cons.push_back(cons({{A, {0}}}, 0));
      const Packed p = pack(b);
      const TsIndex I{c.term_ptr.data(), c.post_doc.data(), c.n_terms, c.n_docs};
      long long cm = 0, cap = 0;
      for (size_t k = 0; k < b.cons.size(); ++k) cm = std::max(cm, ts_driver(I, p.view((int)b.bases.size()), (long)k).len), cap += ts_driver(I, p.view((int)b.bases.size()), (long)k).len;
      const Result r = resolve(c, p, (int)b.bases.size(), (long)b.cons.size(), cm, cap);
      for (size_t k = 0; k < b.cons.size(); ++k) {
        const std::vector<long long> got(r.rows.begin() + r.scope_ptr[k], r.rows.begin() + r.scope_ptr[k + 1]);
        CHECK(got == plain(c, b, b.cons[k]) && r.status[k] == 0, "tiny n=%ld constraint %zu", n, k);
      }
      std::printf("tiny%s ok\n", at.c_str());
      continue;
    }
    family(("must only" + at).c_str(), c,
           Batch{{cons({{M, {5}}}), cons({{M, {3}}, {M, {7}}}), cons({{M, {0}}}), cons({{M, {2}}}), cons({{M, {1}}})}, {}});
    family(("any only (iota)" + at).c_str(), c, Batch{{cons({{A, {8}}, {A, {9}}}), cons({{A, {2}}}), cons({{A, {0}}})}, {}});
    family(("not only (iota)" + at).c_str(), c, Batch{{cons({{N, {3}}}), cons({{N, {1}}}), cons({{N, {4}}, {N, {5}}})}, {}});
    family(("all three" + at).c_str(), c,
           Batch{{cons({{M, {3}}, {A, {5}}, {A, {6}}, {N, {7}}}), cons({{M, {4}}, {M, {10}}, {A, {2}}, {A, {11}}, {N, {9}}})}, {}});
    family(("multi-token groups" + at).c_str(), c,
           Batch{{cons({{M, {3, 4}}}), cons({{A, {5, 6}}, {A, {7, 10}}}), cons({{M, {0}}, {N, {3, 4, 5}}}), cons({{M, {4, 3, 10}}})}, {}});
    family(("a repeated term" + at).c_str(), c,
           Batch{{cons({{M, {5, 5}}}), cons({{M, {5}}, {M, {5}}}), cons({{M, {4}}, {A, {6, 6}}, {N, {7, 7}}})}, {}});
    family(("unknown terms" + at).c_str(), c,
           Batch{{cons({{M, {5, -1}}}), cons({{M, {5}}, {A, {-1}}, {A, {6}}}), cons({{M, {5}}, {A, {-1}}}), cons({{M, {5}}, {N, {-1}}}),
                  cons({{M, {5}}, {N, {6, -1}}}), cons({{M, {(int)c.n_terms}}}), cons({{A, {-1}}, {A, {7}}})}, {}});
    family(("base scopes" + at).c_str(), c,
           Batch{{cons({{M, {9}}}, 0), cons({{M, {3}}}, 1), cons({{M, {3}}}, 2), cons({}, 1), cons({{N, {4}}}, 2), cons({{M, {2}}}, 0),
                  cons({{A, {5}}}, 3)},
                 {every, odd, few, {}}});
    {  // driver ties: terms 10 and 11 of one length by construction of a second corpus
      Corpus t = c;
      t.has[11] = t.has[10];
      std::reverse(t.has[11].begin(), t.has[11].end());
      t.post_doc.clear();
      for (long k = 0; k < t.n_terms; ++k) {
        for (long d = 0; d < n; ++d)
          if (t.has[k][d]) t.post_doc.push_back((int)d);
        t.term_ptr[k + 1] = (long long)t.post_doc.size();
      }
      std::vector<long long> same;  // a base as long as term 10's list
      for (long d = 0; d < n && (long long)same.size() < t.term_ptr[11] - t.term_ptr[10]; ++d) same.push_back(d);
      const Packed p = pack(Batch{{cons({{M, {10}}, {M, {11}}}), cons({{M, {11}}, {M, {10}}}), cons({{M, {10}}}, 0)}, {same}});
      const TsIndex I{t.term_ptr.data(), t.post_doc.data(), t.n_terms, t.n_docs};
      CHECK(ts_driver(I, p.view(1), 0).term == 10 && ts_driver(I, p.view(1), 1).term == 11, "tie between lists: not the first");
      CHECK(ts_driver(I, p.view(1), 2).kind == kTsDrvBase, "tie between base and list: not the base");
      family(("driver ties" + at).c_str(), t,
             Batch{{cons({{M, {10}}, {M, {11}}}), cons({{M, {11}}, {M, {10}}}), cons({{M, {10}}}, 0)}, {same}});
    }
  }
  validation();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("term scope rule ok\n");
  return 0;
}

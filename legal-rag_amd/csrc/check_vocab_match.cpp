// Host check of the rules of amdr_vocab_match (vocab_match_rule.hpp), a program of its own:
//   check_vocab_match
// It resolves generated patterns over generated vocabularies cell by cell as the kernels of vocab_match.hip do — per
// (pattern, tile of kVmTile terms) the pattern staged by vm_span_ok / vm_pattern_info, a bitmap of exactly kVmWords words
// set by vm_term_match, counted and parked; the scan; then per cell the parked words expanded by vm_expand_word into the
// fixed-stride rows, n_match and the padding by the block of tile 0 — and compares every output byte with a naive
// evaluation: a full-matrix optimal-string-alignment distance and a full-table wildcard match over code points decoded by
// a decoder of its own.  Every array has exactly the size the header promises (allocated at that size), so with the host
// sanitizers (tests/test_vocab_match_rule_host.py) an access outside one is a failure.  Then the written-out cases, every
// malformed device-side pattern (n_match 0) and every refusal of vm_check_args, vm_validate and vm_validate_vocab.
// Build: c++ -std=c++17 check_vocab_match.cpp (plain host code; no HIP header is needed).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#define AMDR_COMPACT_HOST_ONLY 1
#include "compact.hpp"
#include "vocab_match_rule.hpp"

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

using Cps = std::vector<uint32_t>;

void put_utf8(std::string& out, uint32_t c) {
  if (c < 0x80) {
    out += (char)c;
  } else if (c < 0x800) {
    out += (char)(0xC0 | (c >> 6)), out += (char)(0x80 | (c & 0x3F));
  } else if (c < 0x10000) {
    out += (char)(0xE0 | (c >> 12)), out += (char)(0x80 | ((c >> 6) & 0x3F)), out += (char)(0x80 | (c & 0x3F));
  } else {
    out += (char)(0xF0 | (c >> 18)), out += (char)(0x80 | ((c >> 12) & 0x3F)), out += (char)(0x80 | ((c >> 6) & 0x3F));
    out += (char)(0x80 | (c & 0x3F));
  }
}

// ---- the naive side ------------------------------------------------------------------------------------------------------
int naive_osa(const Cps& a, const Cps& b) {
  const size_t n = a.size(), m = b.size();
  std::vector<std::vector<int>> D(n + 1, std::vector<int>(m + 1, 0));
  for (size_t i = 0; i <= n; ++i) D[i][0] = (int)i;
  for (size_t j = 0; j <= m; ++j) D[0][j] = (int)j;
  for (size_t i = 1; i <= n; ++i)
    for (size_t j = 1; j <= m; ++j) {
      int v = std::min({D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1])});
      if (i > 1 && j > 1 && a[i - 1] == b[j - 2] && a[i - 2] == b[j - 1]) v = std::min(v, D[i - 2][j - 2] + 1);
      D[i][j] = v;
    }
  return D[n][m];
}

bool naive_wild(const Cps& pat, const Cps& t) {  // ok[i][j]: pat[i ..) names t[j ..)
  const size_t m = pat.size(), n = t.size();
  std::vector<std::vector<char>> ok(m + 1, std::vector<char>(n + 1, 0));
  ok[m][n] = 1;
  for (size_t i = m; i-- > 0;)
    for (size_t j = n + 1; j-- > 0;) {
      if (pat[i] == kVmAnyRun)
        ok[i][j] = ok[i + 1][j] || (j < n && ok[i][j + 1]);
      else
        ok[i][j] = j < n && (pat[i] == kVmAnyOne || pat[i] == t[j]) && ok[i + 1][j + 1];
    }
  return ok[0][0] != 0;
}

bool pattern_valid(const Cps& pat, int kind, int arg) {
  if (pat.empty() || pat.size() > (size_t)kVmMaxLen) return false;
  if (kind == kVmFuzzy) {
    if (arg < 1 || arg > 2) return false;
    for (uint32_t c : pat)
      if (c > 0x10FFFF) return false;
    return true;
  }
  if (kind != kVmWildcard || arg != 0) return false;
  int literals = 0;
  for (uint32_t c : pat) {
    if (c > 0x10FFFF && c != kVmAnyOne && c != kVmAnyRun) return false;
    literals += c <= 0x10FFFF;
  }
  return literals >= 1;
}

// ---- a case --------------------------------------------------------------------------------------------------------------
struct Case {
  std::vector<Cps> terms;
  std::vector<Cps> pats;
  std::vector<int32_t> kind, arg;
  int item_cap = 16;
};

struct Result {
  std::vector<int32_t> ids;
  std::vector<uint8_t> dist;
  std::vector<int64_t> n_match;
};

Result naive(const Case& c) {
  const size_t P = c.pats.size();
  Result r;
  r.ids.assign(P * c.item_cap, -1), r.dist.assign(P * c.item_cap, 255), r.n_match.assign(P, 0);
  for (size_t p = 0; p < P; ++p) {
    if (!pattern_valid(c.pats[p], c.kind[p], c.arg[p])) continue;
    int64_t n = 0;
    for (size_t t = 0; t < c.terms.size(); ++t) {
      if (c.terms[t].empty()) continue;
      int d = 0;
      bool hit;
      if (c.kind[p] == kVmFuzzy) {
        d = naive_osa(c.terms[t], c.pats[p]);
        hit = d <= c.arg[p];
      } else {
        hit = naive_wild(c.pats[p], c.terms[t]);
      }
      if (!hit) continue;
      if (n < c.item_cap) r.ids[p * c.item_cap + n] = (int32_t)t, r.dist[p * c.item_cap + n] = (uint8_t)d;
      ++n;
    }
    r.n_match[p] = n;
  }
  return r;
}

// What vm_count_kernel, the scan and vm_write_kernel do, block by block.  pat_ptr / cp_total may be given (garbage spans).
Result run(const Case& c, const std::vector<int64_t>* ptr_override = nullptr) {
  std::string blob;
  std::vector<long long> offs{0};
  for (const Cps& t : c.terms) {
    for (uint32_t cp : t) put_utf8(blob, cp);
    offs.push_back((long long)blob.size());
  }
  const long long n_terms = (long long)c.terms.size();
  std::vector<unsigned char> bytes(blob.begin(), blob.end());
  bytes.shrink_to_fit();
  std::vector<int32_t> cp_len((size_t)n_terms);
  std::vector<int64_t> offs64(offs.begin(), offs.end());
  CHECK(vm_validate_vocab(bytes.data(), offs64.data(), n_terms, cp_len.data()) == kVmValid, "vocabulary refused");
  for (long long t = 0; t < n_terms; ++t) CHECK(cp_len[t] == (int)c.terms[t].size(), "cp_len of term %lld", t);
  const VmVocab V{bytes.data(), offs.data(), cp_len.data(), n_terms};

  std::vector<uint32_t> pat_cp;
  std::vector<int64_t> pat_ptr{0};
  for (const Cps& p : c.pats) {
    pat_cp.insert(pat_cp.end(), p.begin(), p.end());
    pat_ptr.push_back((int64_t)pat_cp.size());
  }
  const long long cp_total = (long long)pat_cp.size();
  if (ptr_override) pat_ptr = *ptr_override;
  pat_cp.shrink_to_fit();
  const long long n_pat = (long long)c.pats.size(), cap = c.item_cap;
  long long cells = 0;
  CHECK(vm_cells(n_pat, n_terms, &cells), "cells");
  const long long tiles = vm_tiles(n_terms);
  const VmWork w = vm_work(cells);
  CHECK(w.total >= w.off_parked + cells * kVmWords * 4 && w.off_offsets >= cells * 8 && w.off_parked >= w.off_offsets + (cells + 1) * 8,
        "workspace layout");
  std::vector<long long> counts((size_t)cells), offsets((size_t)cells + 1);
  std::vector<unsigned> parked((size_t)cells * kVmWords);
  Result r;
  r.ids.assign((size_t)(n_pat * cap), 7), r.dist.assign((size_t)(n_pat * cap), 7), r.n_match.assign((size_t)n_pat, 7);
  auto stage = [&](long long p, std::vector<unsigned>& pat) {
    const long long b = pat_ptr[p], e = pat_ptr[p + 1];
    const int m = vm_span_ok(b, e, cp_total) ? (int)(e - b) : 0;
    for (int j = 0; j < m; ++j) pat[j] = pat_cp[(size_t)(b + j)];
    return vm_pattern_info(pat.data(), m, c.kind[p], c.arg[p]);
  };
  for (long long cell = 0; cell < cells; ++cell) {  // count
    const long long p = cell / tiles, tile = cell - p * tiles;
    std::vector<unsigned> bits(kVmWords, 0u), pat(kVmMaxLen, 0xdeadbeefu);
    const VmPat P = stage(p, pat);
    if (P.ok) {
      const long long base = tile * kVmTile, end = std::min(base + kVmTile, n_terms);
      for (long long term = base; term < end; ++term) {
        int dist;
        if (vm_term_match(V, pat.data(), P, term, &dist)) bits[(size_t)vm_bit_word(term, tile)] |= vm_bit_mask(term);
      }
    }
    long long total = 0;
    for (int j = 0; j < kVmWords; ++j) parked[(size_t)cell * kVmWords + j] = bits[j], total += vm_popcount(bits[j]);
    counts[(size_t)cell] = total;
  }
  compact_scan_host(counts.data(), (long)cells, offsets.data());
  for (long long cell = 0; cell < cells; ++cell) {  // write
    const long long p = cell / tiles, tile = cell - p * tiles;
    std::vector<unsigned> pat(kVmMaxLen, 0xdeadbeefu);
    const VmPat P = stage(p, pat);
    int32_t* ids_row = r.ids.data() + p * cap;
    uint8_t* dist_row = r.dist.data() + p * cap;
    const long long first = offsets[(size_t)(p * tiles)];
    if (tile == 0) {
      const long long all = offsets[(size_t)((p + 1) * tiles)] - first;
      r.n_match[(size_t)p] = all;
      for (long long i = all; i < cap; ++i) ids_row[i] = -1, dist_row[i] = kVmNoDist;
    }
    long long at = offsets[(size_t)cell] - first;
    for (int j = 0; j < kVmWords; ++j)
      at += vm_expand_word(parked[(size_t)cell * kVmWords + j], tile, j, at, cap, V, pat.data(), P, ids_row, dist_row);
  }
  return r;
}

void compare(const char* name, const Case& c) {
  const Result got = run(c), want = naive(c);
  CHECK(got.n_match == want.n_match, "%s: n_match", name);
  CHECK(got.ids == want.ids, "%s: ids", name);
  CHECK(got.dist == want.dist, "%s: dist", name);
}

const uint32_t kAlphabet[] = {'a', 'b', 'c', 'd', 0xE9 /* é */, 0x4E2D /* 中 */, 0x56FD /* 国 */, 0x20000 /* 𠀀 */, '?'};
constexpr int kAlpha = (int)(sizeof kAlphabet / sizeof kAlphabet[0]);

Cps random_term(Rng& g, int alpha, int max_len) {
  Cps t((size_t)g.below(max_len + 1));
  for (uint32_t& c : t) c = kAlphabet[g.below(alpha)];
  return t;
}

Cps edited(Rng& g, Cps t, int edits, int alpha) {
  for (int k = 0; k < edits; ++k) {
    const long op = g.below(4), at = t.empty() ? 0 : g.below((long)t.size());
    if (op == 0 || t.empty())
      t.insert(t.begin() + at, kAlphabet[g.below(alpha)]);
    else if (op == 1 && t.size() > 1)
      t.erase(t.begin() + at);
    else if (op == 2)
      t[(size_t)at] = kAlphabet[g.below(alpha)];
    else if (at + 1 < (long)t.size())
      std::swap(t[(size_t)at], t[(size_t)at + 1]);
  }
  return t;
}

Cps wild_of(Rng& g, Cps t) {
  if (t.empty()) t.push_back('a');
  Cps out;
  for (size_t i = 0; i < t.size(); ++i) {
    const long k = g.below(6);
    if (k == 0)
      out.push_back(kVmAnyOne);
    else if (k == 1) {
      out.push_back(kVmAnyRun);
      i += (size_t)g.below(3);
    } else {
      out.push_back(t[i]);
    }
  }
  if (g.below(4) == 0) out.push_back(kVmAnyRun);
  bool lit = false;
  for (uint32_t c : out) lit = lit || c <= 0x10FFFF;
  if (!lit) out.push_back(t[0]);
  return out;
}

Case random_case(Rng& g, long n_terms, int n_pats, int alpha, int max_len, int kind, int cap) {
  Case c;
  c.item_cap = cap;
  for (long t = 0; t < n_terms; ++t) c.terms.push_back(random_term(g, alpha, max_len));
  for (int p = 0; p < n_pats; ++p) {
    Cps src = c.terms.empty() ? Cps{'a'} : c.terms[(size_t)g.below(n_terms)];
    if (src.empty()) src.push_back('b');
    const int k = kind < 0 ? (int)g.below(2) : kind;
    if (k == kVmFuzzy) {
      const int e = 1 + (int)g.below(2);
      Cps q = edited(g, src, (int)g.below(4), alpha);
      if (q.empty()) q.push_back('c');
      c.pats.push_back(q), c.kind.push_back(kVmFuzzy), c.arg.push_back(e);
    } else {
      c.pats.push_back(wild_of(g, src)), c.kind.push_back(kVmWildcard), c.arg.push_back(0);
    }
  }
  return c;
}

Cps cps(const char* ascii) {
  Cps out;
  for (const char* p = ascii; *p; ++p) out.push_back(*p == '?' ? kVmAnyOne : *p == '*' ? kVmAnyRun : (uint32_t)(unsigned char)*p);
  return out;
}
Cps lit(const char* ascii) {
  Cps out;
  for (const char* p = ascii; *p; ++p) out.push_back((uint32_t)(unsigned char)*p);
  return out;
}

int banded(const Cps& pat, int e, const Cps& t) {
  std::string s;
  for (uint32_t c : t) put_utf8(s, c);
  std::vector<unsigned char> b(s.begin(), s.end());
  b.shrink_to_fit();
  std::vector<unsigned> p(pat.begin(), pat.end());
  p.shrink_to_fit();
  return vm_osa_banded(p.data(), (int)p.size(), e, b.data(), 0, (long long)b.size());
}
bool wild(const Cps& pat, const Cps& t) {
  std::string s;
  for (uint32_t c : t) put_utf8(s, c);
  std::vector<unsigned char> b(s.begin(), s.end());
  b.shrink_to_fit();
  std::vector<unsigned> p(pat.begin(), pat.end());
  p.shrink_to_fit();
  return vm_wild_match(p.data(), (int)p.size(), b.data(), 0, (long long)b.size());
}

}  // namespace

int main() {
  Rng g{20260317};
  // ---- families ----
  struct Family {
    const char* name;
    int kind, alpha, max_len, rounds;
  };
  const Family families[] = {{"fuzzy-ascii", kVmFuzzy, 3, 7, 60},    {"fuzzy-unicode", kVmFuzzy, kAlpha, 6, 60},
                             {"wildcard-ascii", kVmWildcard, 3, 8, 60}, {"wildcard-unicode", kVmWildcard, kAlpha, 6, 60},
                             {"mixed", -1, 4, 10, 40}};
  for (const Family& f : families) {
    const int before = failures;
    for (int r = 0; r < f.rounds; ++r) compare(f.name, random_case(g, 1 + g.below(300), 1 + (int)g.below(12), f.alpha, f.max_len, f.kind, 8));
    std::printf("vocab_match %s: %d rounds\n", f.name, f.rounds);
    if (failures == before) std::printf("family ok\n");
  }
  {  // the vocabulary sizes around the tile, with matches at ids 0, T - 1, T and n - 1
    const int before = failures;
    const long T = kVmTile;
    for (long n : {1L, 63L, 64L, 65L, T - 1, T, T + 1, 3 * T + 7}) {
      Case c = random_case(g, n, 0, 2, 5, kVmFuzzy, 8);
      for (long at : {0L, T - 1, T, n - 1})
        if (at >= 0 && at < n) c.terms[(size_t)at] = lit("zebra");
      c.pats = {lit("zebra"), cps("z?b*"), lit("zbera"), lit("a")};
      c.kind = {kVmFuzzy, kVmWildcard, kVmFuzzy, kVmFuzzy}, c.arg = {1, 0, 1, 2};
      compare("sizes", c);
    }
    std::printf("vocab_match sizes: 8 vocabularies\n");
    if (failures == before) std::printf("family ok\n");
  }
  {  // truncation: cap - 1, cap and cap + 1 matches, spread over two tiles; and long patterns and terms
    const int before = failures;
    for (int extra = -1; extra <= 1; ++extra) {
      Case c = random_case(g, kVmTile + 40, 0, 2, 4, kVmFuzzy, 6);
      int put = 0;
      for (long at : {3L, 500L, (long)kVmTile - 1, (long)kVmTile, (long)kVmTile + 7, (long)kVmTile + 8, (long)kVmTile + 39})
        if (put < c.item_cap + extra) c.terms[(size_t)at] = lit("quorum"), ++put;
      c.pats = {lit("quorum"), cps("quo*"), lit("b")};
      c.kind = {kVmFuzzy, kVmWildcard, kVmFuzzy}, c.arg = {1, 0, 1};
      const Result got = run(c);
      CHECK(got.n_match[0] == c.item_cap + extra && got.n_match[1] == c.item_cap + extra, "cap%+d: the true count", extra);
      compare("cap", c);
    }
    Case c;
    c.item_cap = 4;
    Cps long63(63, 'x'), long64(64, 'x'), long300(300, 'x');
    long63[10] = 'y', long64[10] = 'y';
    c.terms = {long63, long64, Cps(65, 'x'), long300, lit("x"), Cps{}};
    c.pats = {long63, long64, lit("x"), cps("*y*"), cps("x*x")};
    c.kind = {kVmFuzzy, kVmFuzzy, kVmFuzzy, kVmWildcard, kVmWildcard}, c.arg = {1, 2, 1, 0, 0};
    compare("long", c);
    std::printf("vocab_match cap: 3 rows and the long ones\n");
    if (failures == before) std::printf("family ok\n");
  }
  // ---- written-out cases ----
  {
    const int before = failures;
    CHECK(naive_osa(lit("recieve"), lit("receive")) == 1 && banded(lit("recieve"), 1, lit("receive")) == 1, "recieve -> receive is 1");
    CHECK(banded(lit("recieve"), 1, lit("relieve")) == 1, "recieve -> relieve is 1");
    CHECK(naive_osa(lit("ca"), lit("abc")) == 3 && banded(lit("ca"), 2, lit("abc")) > 2, "OSA, not unrestricted Damerau");
    CHECK(banded(lit("warrenty"), 1, lit("warranty")) == 1 && banded(lit("warrenty"), 1, lit("warrant")) > 1, "warrenty");
    CHECK(banded(lit("ab"), 2, lit("ba")) == 1 && banded(lit("abc"), 1, lit("abc")) == 0, "transposition, identity");
    CHECK(banded(Cps{0x4E2D, 0x6587}, 1, Cps{0x56FD, 0x6587}) == 1, "one substitution of a 3-byte code point");
    CHECK(banded(lit("cafe"), 1, Cps{'c', 'a', 'f', 0xE9}) == 1, "e against é is one substitution");
    CHECK(wild(cps("a?c"), Cps{'a', 0x20000, 'c'}) && !wild(cps("a?c"), lit("ac")), "? is one code point of four bytes");
    CHECK(wild(cps("a*a"), lit("aa")) && !wild(cps("a*a"), lit("a")), "a*a");
    CHECK(wild(cps("*ab*ab?"), lit("abxababc")) && !wild(cps("*ab*ab?"), lit("abab")), "the backtrack");
    CHECK(wild(cps("**ee"), lit("lessee")) && wild(cps("s?ll*"), lit("seller")) && !wild(cps("s?ll*"), lit("sll")), "forms");
    CHECK(wild(Cps{'a', '?' /* a literal question mark cannot be written in a pattern: this is U+003F as a literal */}, lit("a?"))
              && !wild(Cps{'a', '?'}, lit("ab")), "a literal U+003F in a pattern is itself");
    CHECK(!wild(cps("*"), Cps{}) && banded(lit("a"), 1, Cps{}) > 1, "a term of zero bytes");
    unsigned cp = 0;
    const unsigned char cut[2] = {0xF0, 0xA0};  // a 4-byte sequence cut short by the term's end
    CHECK(vm_decode(cut, 0, 2, &cp) == 2, "the decoder stops at the end");
    if (failures == before) std::printf("written-out ok\n");
  }
  // ---- malformed device-side patterns: each names nothing ----
  {
    const int before = failures;
    Case c = random_case(g, 200, 0, 3, 4, kVmFuzzy, 5);
    c.terms[0] = lit("abc");
    c.pats = {lit("abc"), lit("abc"), lit("abc"), lit("abc"), cps("a?c"), cps("??*"), Cps{'a', 0x110002}, lit("abc"), lit("abc"), lit("abc")};
    c.kind = {2, -1, kVmFuzzy, kVmFuzzy, kVmFuzzy, kVmWildcard, kVmWildcard, kVmWildcard, kVmFuzzy, kVmFuzzy};
    c.arg = {0, 0, 0, 3, 1, 0, 0, 1, 1, 1};
    Result got = run(c);
    for (size_t p = 0; p + 2 < c.pats.size(); ++p) CHECK(got.n_match[p] == 0, "malformed pattern %zu names %lld terms", p, (long long)got.n_match[p]);
    CHECK(got.n_match[8] >= 1 && got.n_match[9] >= 1, "the valid ones beside them");
    compare("garbage", c);
    // spans: negative, reversed, too long, beyond cp_total
    Case d = c;
    d.pats = {lit("abc"), lit("abc"), Cps(70, 'a'), lit("abc")};
    d.kind = {kVmFuzzy, kVmFuzzy, kVmFuzzy, kVmFuzzy}, d.arg = {1, 1, 1, 1};
    const std::vector<int64_t> spans{-5, 6, 3, 3 + 70, 1000};
    got = run(d, &spans);
    for (size_t p = 0; p < 4; ++p) CHECK(got.n_match[p] == 0 && got.ids[p * d.item_cap] == -1, "garbage span %zu", p);
    if (failures == before) std::printf("garbage ok\n");
  }
  // ---- refusals ----
  {
    const int before = failures;
    const uint32_t cp[4] = {'a', 'b', kVmAnyOne, kVmAnyRun};
    const int64_t ptr[3] = {0, 2, 4};
    const int32_t kind[2] = {kVmFuzzy, kVmWildcard}, arg[2] = {1, 0};
    CHECK(vm_validate(cp, ptr, kind, arg, 2, 4) == kVmLiteral, "a wildcard of ?* has no literal");
    const int64_t ptr1[2] = {0, 3};
    const int32_t kw[1] = {kVmWildcard}, kf[1] = {kVmFuzzy}, a0[1] = {0}, a1[1] = {1}, a3[1] = {3}, k2[1] = {2};
    CHECK(vm_validate(cp, ptr1, kw, a0, 1, 3) == kVmValid && vm_validate(cp, ptr1, kf, a1, 1, 2) == kVmPtr, "valid; cp_total");
    CHECK(vm_validate(cp, ptr1, kf, a1, 1, 3) == kVmValue, "a reserved value in a fuzzy pattern");
    CHECK(vm_validate(cp, ptr1, kf, a3, 1, 3) == kVmKindArg && vm_validate(cp, ptr1, kf, a0, 1, 3) == kVmKindArg, "edits");
    CHECK(vm_validate(cp, ptr1, kw, a1, 1, 3) == kVmKindArg && vm_validate(cp, ptr1, k2, a0, 1, 3) == kVmKindArg, "kind, arg");
    const int64_t bad0[2] = {1, 3}, rev[3] = {0, 3, 2}, empty[3] = {0, 0, 3};
    CHECK(vm_validate(cp, bad0, kw, a0, 1, 3) == kVmPtr && vm_validate(cp, rev, kind, arg, 2, 2) == kVmPtr, "pat_ptr");
    CHECK(vm_validate(cp, empty, kind, arg, 2, 3) == kVmLength, "an empty pattern");
    std::vector<uint32_t> wide(65, 'a');
    const int64_t ptr65[2] = {0, 65};
    CHECK(vm_validate(wide.data(), ptr65, kf, a1, 1, 65) == kVmLength, "65 code points");
    const uint32_t odd[2] = {'a', 0x110002};
    const int64_t ptr2[2] = {0, 2};
    CHECK(vm_validate(odd, ptr2, kw, a0, 1, 2) == kVmValue, "a value that is neither");
    CHECK(vm_validate(nullptr, ptr1, kw, a0, 1, 3) == kVmNull && vm_validate(cp, ptr1, kw, a0, -1, 3) == kVmSizes, "null, sizes");
    CHECK(vm_validate(nullptr, nullptr, nullptr, nullptr, 0, 0) == kVmValid, "no pattern");
    long long cells = 0;
    int h = 0;
    int32_t ids[1];
    uint8_t dist[1];
    int64_t nm[1];
    CHECK(vm_check_args(&h, 10, cp, ptr1, kw, a0, 1, 3, 1, ids, dist, nm, &cells) == kVmValid && cells == 1, "valid arguments");
    CHECK(vm_check_args(nullptr, 10, cp, ptr1, kw, a0, 1, 3, 1, ids, dist, nm, &cells) == kVmNull, "null handle");
    CHECK(vm_check_args(&h, 10, cp, ptr1, kw, a0, 1, 3, 1, nullptr, dist, nm, &cells) == kVmNull, "null output");
    CHECK(vm_check_args(&h, 10, cp, ptr1, kw, a0, -1, 3, 1, ids, dist, nm, &cells) == kVmSizes, "negative n_pat");
    CHECK(vm_check_args(&h, 10, cp, ptr1, kw, a0, 1, -3, 1, ids, dist, nm, &cells) == kVmSizes, "negative cp_total");
    CHECK(vm_check_args(&h, 10, cp, ptr1, kw, a0, 1, 3, 0, ids, dist, nm, &cells) == kVmCap, "item_cap 0");
    CHECK(vm_check_args(&h, 10, cp, ptr1, kw, a0, 1, 3, kVmMaxCap + 1, ids, dist, nm, &cells) == kVmCap, "item_cap 4097");
    CHECK(vm_check_args(&h, 10, cp, ptr1, kw, a0, kVmMaxCells + 1, 3, 1, ids, dist, nm, &cells) == kVmCells, "too many cells");
    CHECK(vm_check_args(&h, 2 * kVmTile, cp, ptr1, kw, a0, kVmMaxCells / 2 + 1, 3, 1, ids, dist, nm, &cells) == kVmCells, "cells x tiles");
    CHECK(vm_check_args(&h, 10, nullptr, nullptr, nullptr, nullptr, 0, 0, 1, nullptr, nullptr, nullptr, &cells) == kVmValid, "empty call");
    CHECK(vm_work(0).total == 0 && vm_work(1).total == 256 + 256 + 1024 && vm_work(33).total == 512 + 512 + 33 * 1024, "plan");
    const unsigned char over[2] = {0xC0, 0x80}, sur[3] = {0xED, 0xA0, 0x80}, big[4] = {0xF4, 0x90, 0x80, 0x80}, cutoff[1] = {0xE4};
    const int64_t o2[2] = {0, 2}, o3[2] = {0, 3}, o4[2] = {0, 4}, o1[2] = {0, 1}, from1[2] = {1, 2}, down[3] = {0, 2, 1};
    CHECK(vm_validate_vocab(over, o2, 1, nullptr) == kVmUtf8 && vm_validate_vocab(sur, o3, 1, nullptr) == kVmUtf8, "overlong, surrogate");
    CHECK(vm_validate_vocab(big, o4, 1, nullptr) == kVmUtf8 && vm_validate_vocab(cutoff, o1, 1, nullptr) == kVmUtf8, "> 10FFFF, cut");
    const unsigned char split[3] = {0xE4, 0xB8, 0xAD};  // 中 cut between two terms
    const int64_t osplit[3] = {0, 1, 3};
    CHECK(vm_validate_vocab(split, osplit, 2, nullptr) == kVmUtf8 && vm_validate_vocab(split, o3, 1, nullptr) == kVmValid, "a term boundary inside a code point");
    CHECK(vm_validate_vocab(split, from1, 1, nullptr) == kVmOffsets && vm_validate_vocab(split, down, 2, nullptr) == kVmOffsets, "offsets");
    CHECK(vm_validate_vocab(nullptr, o3, 1, nullptr) == kVmNull && vm_validate_vocab(split, nullptr, 1, nullptr) == kVmNull, "null");
    CHECK(vm_validate_vocab(split, o3, -1, nullptr) == kVmSizes, "negative n_terms");
    if (failures == before) std::printf("validate ok\n");
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("vocab match rule ok\n");
  return 0;
}

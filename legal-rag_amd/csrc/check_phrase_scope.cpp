// Host check of the rules of amdr_phrase_lists (phrase_rule.hpp) and of amdr_term_scope_lists (term_scope_rule.hpp with
// virtual posting lists; the host scans of compact.hpp), a program of its own:
//   check_phrase_scope
// It resolves generated phrases tile by tile and lane by lane as the kernels of phrase_scope.hip do — the driver, the
// conjunction per candidate, one round of kPhLanes start positions after the other per surviving document, the counts,
// the scan, the write — then hands the lists to the term step resolved tile by tile as term_scope.hip does, and compares
// both with a naive scan of every document.  Every array has exactly the size the header promises (allocated at that
// size), so with the host sanitizers (tests/test_phrase_rule_host.py) an access outside one is a failure.  Then every
// refusal of ph_validate, ph_validate_stream and ts_validate_lists is provoked once.
// Build: c++ -std=c++17 check_phrase_scope.cpp (plain host code; no HIP header is needed).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#define AMDR_COMPACT_HOST_ONLY 1  // the host forms alone: this program has no device code
#include "compact.hpp"
#include "phrase_rule.hpp"

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

struct Corpus {
  long n_docs, n_terms;
  std::vector<std::vector<int>> docs;  // the naive scan's own form
  std::vector<long long> term_ptr, doc_ptr;
  std::vector<int> post_doc, tokens, doc_len;
  PhIndex index() const {
    return PhIndex{term_ptr.data(), post_doc.data(), n_terms, n_docs, doc_ptr.data(), tokens.data()};
  }
};

// n_docs documents over n_terms terms, term t drawn with weight 1 / (t + 1); the last term is in no document.  Lengths
// 0 .. 90, and the lane stride's edges (63 .. 65, 127 .. 129) and one long document among them.
Corpus make_corpus(long n_docs, long n_terms, uint64_t seed) {
  Corpus c;
  c.n_docs = n_docs, c.n_terms = n_terms;
  Rng r{seed};
  const long special[] = {63, 64, 65, 127, 128, 129, 4550, 0, 1};
  std::vector<long> cum;
  long total = 0;
  for (long t = 0; t + 1 < n_terms; ++t) cum.push_back(total += 1000 / (t + 1));
  for (long d = 0; d < n_docs; ++d) {
    const long len = d < 9 ? special[d] : r.below(91);
    std::vector<int> seq;
    for (long i = 0; i < len; ++i) {
      const long x = r.below(total);
      seq.push_back((int)(std::upper_bound(cum.begin(), cum.end(), x) - cum.begin()));
    }
    c.docs.push_back(seq);
  }
  std::vector<long long> tp(n_terms + 1, 0), dp(n_docs + 1, 0);
  std::vector<int> pd, tk, dl;
  for (long t = 0; t < n_terms; ++t) {
    for (long d = 0; d < n_docs; ++d)
      if (std::find(c.docs[d].begin(), c.docs[d].end(), (int)t) != c.docs[d].end()) pd.push_back((int)d);
    tp[t + 1] = (long long)pd.size();
  }
  for (long d = 0; d < n_docs; ++d) {
    tk.insert(tk.end(), c.docs[d].begin(), c.docs[d].end());
    dp[d + 1] = (long long)tk.size();
    dl.push_back((int)c.docs[d].size());
  }
  c.term_ptr = exact(tp), c.doc_ptr = exact(dp), c.post_doc = exact(pd), c.tokens = exact(tk), c.doc_len = exact(dl);
  return c;
}

bool naive_holds(const std::vector<int>& seq, const std::vector<int>& ph) {
  for (size_t p = 0; p + ph.size() <= seq.size(); ++p)
    if (std::equal(ph.begin(), ph.end(), seq.begin() + (long)p)) return true;
  return false;
}

std::vector<int> naive_list(const Corpus& c, const std::vector<int>& ph) {
  std::vector<int> out;
  for (int t : ph)
    if (t < 0 || t >= c.n_terms) return out;
  for (long d = 0; d < c.n_docs; ++d)
    if (naive_holds(c.docs[d], ph)) out.push_back((int)d);
  return out;
}

struct Lists {
  std::vector<long long> ptr;
  std::vector<int> docs, status;
};

// the three launches of phrase_scope.hip on the CPU, on arrays of the sizes amdr_phrase_lists_plan / the caller promise
Lists run_phrases(const Corpus& c, const std::vector<std::vector<int>>& phrases, long long cand_max, long long rows_cap) {
  const PhIndex I = c.index();
  const long n_phr = (long)phrases.size();
  std::vector<long long> pp(n_phr + 1, 0);
  std::vector<int> pt;
  for (long p = 0; p < n_phr; ++p) pt.insert(pt.end(), phrases[p].begin(), phrases[p].end()), pp[p + 1] = (long long)pt.size();
  const std::vector<int> terms_all = exact(pt);
  const long long tiles = ph_tiles(cand_max);
  const size_t cells = (size_t)n_phr * (size_t)tiles;
  std::vector<long long> counts(cells), offsets(cells + 1);
  std::vector<int> rank(cells * kPhTile, -7);
  Lists r;
  r.ptr.assign(n_phr + 1, -7), r.docs.assign((size_t)rows_cap, -7), r.status.assign(n_phr, -7);
  for (long p = 0; p < n_phr; ++p) {  // count
    const int* terms = terms_all.data() + pp[p];
    const long long L = pp[p + 1] - pp[p];
    const PhDriver D = ph_driver(I, terms, L);
    const bool over = D.len > cand_max;
    r.status[p] = over ? kTsCandOverflow : kTsOk;
    for (long long tile = 0; tile < tiles; ++tile) {
      const size_t cell = (size_t)p * tiles + tile;
      const long long i0 = tile * kPhTile;
      if (over || i0 >= D.len) {
        counts[cell] = 0;
        continue;
      }
      int run = 0;
      for (int t = 0; t < kPhTile; ++t) {
        const long long i = i0 + t;
        bool keep = false;
        if (i < D.len && ph_has_all(I, terms, (int)L, D, I.post_doc[D.begin + i])) {
          const long long doc = I.post_doc[D.begin + i], last = ph_last_start(I, doc, (int)L);
          for (long long base = I.doc_ptr[doc]; base <= last && !keep; base += kPhLanes)
            for (int lane = 0; lane < kPhLanes; ++lane) keep = ph_lane_hit(I, terms, (int)L, base, lane, last) || keep;
        }
        rank[cell * kPhTile + t] = keep ? run : -1;
        run += keep ? 1 : 0;
      }
      counts[cell] = run;
    }
  }
  compact_scan_host(counts.data(), (long)cells, offsets.data());
  for (long p = 0; p < n_phr; ++p) {  // write
    const int* terms = terms_all.data() + pp[p];
    const PhDriver D = ph_driver(I, terms, pp[p + 1] - pp[p]);
    const long long b = offsets[(size_t)p * tiles], e = offsets[(size_t)(p + 1) * tiles];
    r.ptr[p] = std::min(b, rows_cap);
    if (p == n_phr - 1) r.ptr[n_phr] = std::min(e, rows_cap);
    if (e > b && e > rows_cap) r.status[p] = kTsRowsOverflow;
    for (long long tile = 0; tile < tiles; ++tile) {
      const size_t cell = (size_t)p * tiles + tile;
      const long long i0 = tile * kPhTile;
      if (D.len > cand_max || i0 >= D.len) continue;
      for (int t = 0; t < kPhTile; ++t) {
        const int rk = rank[cell * kPhTile + t];
        if (rk < 0) continue;
        const long long at = offsets[cell] + rk;
        if (at < rows_cap) r.docs[(size_t)at] = I.post_doc[D.begin + i0 + t];
      }
    }
  }
  if (n_phr == 0) r.ptr[0] = 0;
  return r;
}

std::vector<std::vector<int>> make_phrases(const Corpus& c, long count, uint64_t seed) {
  Rng r{seed};
  std::vector<std::vector<int>> out;
  while ((long)out.size() < count) {
    const long k = (long)out.size();
    const long L = k % 7 == 6 ? kPhMaxLen : 2 + r.below(3);
    std::vector<int> ph;
    if (k % 3 == 2) {
      for (long j = 0; j < L; ++j) ph.push_back((int)r.below(c.n_terms));  // (the last term is in no document)
    } else {
      const std::vector<int>& seq = c.docs[r.below(c.n_docs)];
      if ((long)seq.size() < L) continue;
      const long s = k % 2 ? (long)seq.size() - L : r.below((long)seq.size() - L + 1);  // every other one at the end
      ph.assign(seq.begin() + s, seq.begin() + s + L);
    }
    if (k % 11 == 10) ph[r.below(L)] = k % 2 ? -1 : (int)c.n_terms;  // an id outside the vocabulary, at any position
    out.push_back(ph);
  }
  return out;
}

struct Cons {  // the operands of the term step, exact sizes
  std::vector<long long> grp_ptr, grp_term_ptr, base_ptr, base_rows;
  std::vector<int> grp_kind, grp_terms, cons_base;
  TsCons view() const {
    return TsCons{grp_ptr.data(), grp_kind.data(), grp_term_ptr.data(), grp_terms.data(),
                  base_ptr.data(), base_rows.data(), cons_base.data(), (int)base_ptr.size() - 1};
  }
};

// constraints whose terms are plain ids and virtual ids n_terms + p, p < n_x (and p == n_x: in no document)
Cons make_constraints(const Corpus& c, long n_x, long count, uint64_t seed) {
  Rng r{seed};
  std::vector<long long> gp{0}, gtp{0}, bp{0}, br;
  std::vector<int> gk, gt, cb;
  for (long d = 0; d < c.n_docs; d += 3) br.push_back(d);
  bp.push_back((long long)br.size());
  for (long k = 0; k < count; ++k) {
    const long groups = 1 + r.below(3);
    for (long g = 0; g < groups; ++g) {
      gk.push_back(g == 0 && k % 4 != 3 ? kTsMust : (int)r.below(3));
      const long n = 1 + r.below(2);
      for (long j = 0; j < n; ++j)
        gt.push_back(r.below(2) ? (int)(c.n_terms + r.below(n_x + 1)) : (int)r.below(c.n_terms));
      gtp.push_back((long long)gt.size());
    }
    gp.push_back((long long)gk.size());
    cb.push_back(k % 5 == 4 ? 0 : -1);
  }
  Cons o;
  o.grp_ptr = exact(gp), o.grp_term_ptr = exact(gtp), o.base_ptr = exact(bp), o.base_rows = exact(br);
  o.grp_kind = exact(gk), o.grp_terms = exact(gt), o.cons_base = exact(cb);
  return o;
}

bool naive_term_has(const Corpus& c, const std::vector<std::vector<int>>& lists, int t, long d) {
  if (t < 0) return false;
  if (t < c.n_terms) return std::find(c.docs[d].begin(), c.docs[d].end(), t) != c.docs[d].end();
  const long p = t - c.n_terms;
  return p < (long)lists.size() && std::binary_search(lists[p].begin(), lists[p].end(), (int)d);
}

bool naive_qualifies(const Corpus& c, const std::vector<std::vector<int>>& lists, const Cons& o, long k, long d) {
  bool any_seen = false, any_ok = false;
  for (long long g = o.grp_ptr[k]; g < o.grp_ptr[k + 1]; ++g) {
    bool has = true;
    for (long long j = o.grp_term_ptr[g]; j < o.grp_term_ptr[g + 1]; ++j) has = has && naive_term_has(c, lists, o.grp_terms[j], d);
    if (o.grp_kind[g] == kTsMust && !has) return false;
    if (o.grp_kind[g] == kTsNot && has) return false;
    if (o.grp_kind[g] == kTsAny) any_seen = true, any_ok = any_ok || has;
  }
  if (any_seen && !any_ok) return false;
  return o.cons_base[k] < 0 || d % 3 == 0;
}

// the term step tile by tile (term_scope.hip), the virtual lists on arrays of exact size
void run_term_step(const Corpus& c, const Lists& L, const std::vector<std::vector<int>>& naive, const Cons& o, const char* name) {
  const long n_x = (long)L.ptr.size() - 1;
  const std::vector<long long> x_ptr = exact(L.ptr);
  const std::vector<int> x_doc(L.docs.begin(), L.docs.begin() + L.ptr[n_x]);
  const TsIndex I{c.term_ptr.data(), c.post_doc.data(), c.n_terms, c.n_docs, x_ptr.data(), x_doc.data(), n_x};
  const TsCons C = o.view();
  const long n_cons = (long)o.cons_base.size();
  CHECK(ts_validate_lists((const int64_t*)x_ptr.data(), x_doc.data(), n_x, c.n_docs) == kTsValid, "%s: the phrase lists do not validate", name);
  for (long k = 0; k < n_cons; ++k) {
    const TsDriver D = ts_driver(I, C, k);
    std::vector<long long> got, want;
    for (long long tile = 0; tile < ts_tiles(D.len); ++tile)
      for (int j = 0; j < kTsTile; ++j) {
        const long long i = tile * kTsTile + j;
        if (i < D.len && ts_qualifies(I, C, k, D, ts_candidate(I, C, D, i))) got.push_back(ts_candidate(I, C, D, i));
      }
    for (long d = 0; d < c.n_docs; ++d)
      if (naive_qualifies(c, naive, o, k, d)) want.push_back(d);
    CHECK(got == want, "%s: constraint %ld: %zu rows, the plain filter has %zu (driver kind %d)", name, k, got.size(),
          want.size(), D.kind);
    // the bound: the driver is no longer than the shortest upper bound among its MUST terms
    for (long long g = o.grp_ptr[k]; g < o.grp_ptr[k + 1]; ++g)
      for (long long j = o.grp_term_ptr[g]; j < o.grp_term_ptr[g + 1] && o.grp_kind[g] == kTsMust; ++j) {
        const int t = o.grp_terms[j];
        if (t >= c.n_terms && t - c.n_terms < n_x) CHECK(D.len <= x_ptr[t - c.n_terms + 1] - x_ptr[t - c.n_terms], "%s: driver past a list", name);
      }
  }
}

void family(long n_docs, long n_phr, uint64_t seed) {
  const std::string name = "phrases n=" + std::to_string(n_docs) + " count=" + std::to_string(n_phr);
  const Corpus c = make_corpus(n_docs, 9, seed);
  const std::vector<std::vector<int>> phrases = make_phrases(c, n_phr, seed + 1);
  std::vector<std::vector<int>> want;
  long long cand_max = 0, total = 0, ub_sum = 0;
  const PhIndex I = c.index();
  for (const auto& ph : phrases) {
    want.push_back(naive_list(c, ph));
    const long long len = ph_driver(I, ph.data(), (long long)ph.size()).len;
    cand_max = std::max(cand_max, len), ub_sum += len, total += (long long)want.back().size();
    CHECK((long long)want.back().size() <= len, "%s: a list longer than its driver", name.c_str());
  }
  const Lists r = run_phrases(c, phrases, cand_max, ub_sum);  // the bounds the header promises suffice
  bool same = r.ptr[n_phr] == total;
  for (long p = 0; p < n_phr && same; ++p)
    same = r.status[p] == kTsOk && std::vector<int>(r.docs.begin() + r.ptr[p], r.docs.begin() + r.ptr[p + 1]) == want[p];
  CHECK(same, "%s: the lists differ from the naive scan", name.c_str());
  for (size_t i = (size_t)total; i < r.docs.size(); ++i) CHECK(r.docs[i] == -7, "%s: a write past the lists", name.c_str());
  // one below either bound
  long longest = 0;
  for (long p = 0; p < n_phr; ++p)
    if (ph_driver(I, phrases[p].data(), (long long)phrases[p].size()).len == cand_max) longest = p;
  if (cand_max > 0) {
    const Lists s = run_phrases(c, phrases, cand_max - 1, ub_sum);
    CHECK(s.status[longest] == kTsCandOverflow && s.ptr[longest + 1] == s.ptr[longest], "%s: cand_max - 1", name.c_str());
  }
  if (total > 0) {
    const Lists s = run_phrases(c, phrases, cand_max, total - 1);
    long flagged = 0;
    for (long p = 0; p < n_phr; ++p) flagged += s.status[p] == kTsRowsOverflow;
    CHECK(flagged >= 1 && s.ptr[n_phr] == total - 1, "%s: rows_cap - 1", name.c_str());
    CHECK(std::equal(s.docs.begin(), s.docs.end(), r.docs.begin()), "%s: rows_cap - 1 changed the documents that fit", name.c_str());
  }
  // the term step over the first lists as virtual terms
  const long n_x = std::min<long>(n_phr, 6);
  Lists head;
  head.ptr.assign(r.ptr.begin(), r.ptr.begin() + n_x + 1);
  head.docs = r.docs;
  const std::vector<std::vector<int>> naive_head(want.begin(), want.begin() + n_x);
  run_term_step(c, head, naive_head, make_constraints(c, n_x, 40, seed + 2), name.c_str());
  std::printf("%s: %lld documents in the lists, longest driver %lld\n", name.c_str(), total, cand_max);
  if (failures == 0) std::printf("family ok\n");
}

void validation() {
  const int64_t pp[] = {0, 2, 5}, pp_short[] = {0, 1, 5}, pp_long[] = {0, 17, 19}, pp_down[] = {0, 3, 2}, pp_off[] = {1, 3, 5};
  const int32_t pt[19] = {0};
  CHECK(ph_validate(pp, pt, 2) == kPhValid, "valid phrases");
  CHECK(ph_validate(pp, pt, -1) == kPhSizes, "n_phr < 0");
  CHECK(ph_validate(nullptr, pt, 2) == kPhNull && ph_validate(pp, nullptr, 2) == kPhNull, "null arrays");
  CHECK(ph_validate(pp_off, pt, 2) == kPhPtr && ph_validate(pp_down, pt, 2) == kPhPtr, "phr_ptr");
  CHECK(ph_validate(pp_short, pt, 2) == kPhLength && ph_validate(pp_long, pt, 2) == kPhLength, "a length outside 2 .. 16");
  CHECK(ph_validate(pp, nullptr, 0) == kPhValid, "no phrase reads no term");
  const int64_t dp[] = {0, 2, 2, 5}, dp_off[] = {1, 2, 2, 5}, dp_down[] = {0, 3, 2, 5};
  const int32_t tk[] = {0, 1, 2, 0, 1}, tk_neg[] = {0, 1, -1, 0, 1}, tk_big[] = {0, 1, 3, 0, 1};
  const int32_t dl[] = {2, 0, 3}, dl_other[] = {2, 1, 2};
  CHECK(ph_validate_stream(dp, tk, dl, 3, 3) == kPhValid, "a valid stream");
  CHECK(ph_validate_stream(nullptr, tk, dl, 3, 3) == kPhNull && ph_validate_stream(dp, nullptr, dl, 3, 3) == kPhNull, "null stream");
  CHECK(ph_validate_stream(dp_off, tk, dl, 3, 3) == kPhDocPtr && ph_validate_stream(dp_down, tk, dl, 3, 3) == kPhDocPtr, "doc_ptr");
  CHECK(ph_validate_stream(dp, tk_neg, dl, 3, 3) == kPhToken && ph_validate_stream(dp, tk_big, dl, 3, 3) == kPhToken, "token range");
  CHECK(ph_validate_stream(dp, tk, dl_other, 3, 3) == kPhDocLen, "doc_len");
  const int64_t xp[] = {0, 2, 3}, xp_off[] = {1, 2, 3}, xp_down[] = {0, 3, 2};
  const int32_t xd[] = {1, 4, 0}, xd_order[] = {4, 4, 0}, xd_range[] = {1, 5, 0}, xd_neg[] = {-1, 4, 0};
  CHECK(ts_validate_lists(xp, xd, 2, 5) == kTsValid && ts_validate_lists(nullptr, nullptr, 0, 5) == kTsValid, "valid lists");
  CHECK(ts_validate_lists(xp, xd, -1, 5) == kTsSizes && ts_validate_lists(nullptr, xd, 2, 5) == kTsNull, "n_x < 0, null x_ptr");
  CHECK(ts_validate_lists(xp, nullptr, 2, 5) == kTsNull, "null x_doc");
  CHECK(ts_validate_lists(xp_off, xd, 2, 5) == kTsListPtr && ts_validate_lists(xp_down, xd, 2, 5) == kTsListPtr, "x_ptr");
  CHECK(ts_validate_lists(xp, xd_order, 2, 5) == kTsListOrder, "list order");
  CHECK(ts_validate_lists(xp, xd_range, 2, 5) == kTsListRange && ts_validate_lists(xp, xd_neg, 2, 5) == kTsListRange, "list range");
  // an unknown id, or a length outside the rule, makes the driver empty without reading the index: its arrays are null
  const PhIndex none{nullptr, nullptr, 5, 9, nullptr, nullptr};
  const int bad_lo[] = {2, -1, 3}, bad_hi[] = {2, 3, 5}, one[] = {2};
  CHECK(ph_driver(none, bad_lo, 3).at < 0 && ph_driver(none, bad_hi, 3).at < 0, "an unknown id reads nothing");
  CHECK(ph_driver(none, one, 1).at < 0 && ph_driver(none, one, 17).at < 0, "a length outside 2 .. 16 reads nothing");
  // a virtual id past the lists is in no document and is never dereferenced
  const TsIndex I{nullptr, nullptr, 5, 9, nullptr, nullptr, 2};
  CHECK(!posting_has(I, 7, 0) && !posting_has(I, -1, 0), "an id past the virtual lists");
  // ties: the first token of the shortest length drives
  const long long tp[] = {0, 2, 4, 7};
  const int pdoc[] = {0, 1, 0, 1, 0, 1, 2};
  const PhIndex tie{tp, pdoc, 3, 3, nullptr, nullptr};
  const int t201[] = {2, 0, 1}, t210[] = {2, 1, 0};
  CHECK(ph_driver(tie, t201, 3).term == 0 && ph_driver(tie, t201, 3).at == 1, "tie: not the first in phrase order");
  CHECK(ph_driver(tie, t210, 3).term == 1 && ph_driver(tie, t210, 3).at == 1, "tie: not the first in phrase order");
  if (failures == 0) std::printf("validate ok\n");
}

}  // namespace

int main() {
  const long sizes[] = {40, 300, 900};
  const long counts[] = {1, 2, 65};
  for (long n : sizes)
    for (long k : counts) family(n, k, 1000 + (uint64_t)n * 7 + (uint64_t)k);
  validation();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("phrase rule ok\n");
  return 0;
}

// Host check of the rules of amdr_span_lists (near_rule.hpp, over phrase_rule.hpp's driver and conjunction; the host scans
// of compact.hpp), a program of its own:
//   check_near_scope
// It resolves generated items — Nears of both kinds mixed with phrases — tile by tile, round by round and lane by lane as
// the kernels of phrase_scope.hip do: the driver, the conjunction per candidate, per surviving document one round of
// kPhLanes anchors after the other, each from a STAGED run copied into an array of exactly near_run_len ints, the counts,
// the scan, the write — and compares the lists with a naive scan of every window of every document.  Every array has
// exactly the size the header promises (allocated at that size), so with the host sanitizers
// (tests/test_near_rule_host.py) an access outside one is a failure.  Then every refusal of span_validate is provoked once.
// Build: c++ -std=c++17 check_near_scope.cpp (plain host code; no HIP header is needed).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#define AMDR_COMPACT_HOST_ONLY 1  // the host forms alone: this program has no device code
#include "compact.hpp"
#include "near_rule.hpp"

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
  std::vector<int> post_doc, tokens;
  PhIndex index() const {
    return PhIndex{term_ptr.data(), post_doc.data(), n_terms, n_docs, doc_ptr.data(), tokens.data()};
  }
};

// n_docs documents over n_terms terms, term t drawn with weight 1 / (t + 1); the last term is in no document.  Lengths
// 0 .. 90, and the lane stride's edges (63 .. 65, 127 .. 129), one past a whole staged run (320, 400) and one long
// document among them.
Corpus make_corpus(long n_docs, long n_terms, uint64_t seed) {
  Corpus c;
  c.n_docs = n_docs, c.n_terms = n_terms;
  Rng r{seed};
  const long special[] = {63, 64, 65, 127, 128, 129, 4550, 0, 1, 319, 320, 400};
  std::vector<long> cum;
  long total = 0;
  for (long t = 0; t + 1 < n_terms; ++t) cum.push_back(total += 1000 / (t + 1));
  for (long d = 0; d < n_docs; ++d) {
    const long len = d < 12 ? special[d] : r.below(91);
    std::vector<int> seq;
    for (long i = 0; i < len; ++i) {
      const long x = r.below(total);
      seq.push_back((int)(std::upper_bound(cum.begin(), cum.end(), x) - cum.begin()));
    }
    c.docs.push_back(seq);
  }
  std::vector<long long> tp(n_terms + 1, 0), dp(n_docs + 1, 0);
  std::vector<int> pd, tk;
  for (long t = 0; t < n_terms; ++t) {
    for (long d = 0; d < n_docs; ++d)
      if (std::find(c.docs[d].begin(), c.docs[d].end(), (int)t) != c.docs[d].end()) pd.push_back((int)d);
    tp[t + 1] = (long long)pd.size();
  }
  for (long d = 0; d < n_docs; ++d) {
    tk.insert(tk.end(), c.docs[d].begin(), c.docs[d].end());
    dp[d + 1] = (long long)tk.size();
  }
  c.term_ptr = exact(tp), c.doc_ptr = exact(dp), c.post_doc = exact(pd), c.tokens = exact(tk);
  return c;
}

struct Item {
  int kind;
  std::vector<int> terms;
  int dist;
};

// every window of n + 1 consecutive tokens, each on its own: the multiset of the window covers the item's / the item is
// a subsequence of the window
bool naive_near(const std::vector<int>& seq, const Item& it) {
  const long n = it.dist;
  for (long s = 0; s < (long)seq.size(); ++s) {
    const long e = std::min<long>((long)seq.size(), s + n + 1);
    if (it.kind == kSpanNearOrdered) {
      size_t j = 0;
      for (long q = s; q < e && j < it.terms.size(); ++q)
        if (seq[q] == it.terms[j]) ++j;
      if (j == it.terms.size()) return true;
    } else {
      std::map<int, int> need;
      for (int t : it.terms) ++need[t];
      for (long q = s; q < e; ++q) {
        auto f = need.find(seq[q]);
        if (f != need.end()) --f->second;
      }
      bool all = true;
      for (const auto& kv : need) all = all && kv.second <= 0;
      if (all) return true;
    }
  }
  return false;
}

bool naive_phrase(const std::vector<int>& seq, const std::vector<int>& ph) {
  for (size_t p = 0; p + ph.size() <= seq.size(); ++p)
    if (std::equal(ph.begin(), ph.end(), seq.begin() + (long)p)) return true;
  return false;
}

std::vector<int> naive_list(const Corpus& c, const Item& it) {
  std::vector<int> out;
  for (int t : it.terms)
    if (t < 0 || t >= c.n_terms) return out;
  for (long d = 0; d < c.n_docs; ++d)
    if (it.kind == kSpanPhrase ? naive_phrase(c.docs[d], it.terms) : naive_near(c.docs[d], it)) out.push_back((int)d);
  return out;
}

struct Lists {
  std::vector<long long> ptr;
  std::vector<int> docs, status;
};

long long rounds_walked = 0, longest_run = 0;

// one surviving document, as one wave walks it
bool walk_document(const PhIndex& I, const int* terms, int L, int kind, int dist, long long doc) {
  bool found = false;
  if (kind == kSpanPhrase) {
    const long long last = ph_last_start(I, doc, L);
    for (long long base = I.doc_ptr[doc]; base <= last && !found; base += kPhLanes)
      for (int lane = 0; lane < kPhLanes; ++lane) found = ph_lane_hit(I, terms, L, base, lane, last) || found;
    return found;
  }
  const long long end = I.doc_ptr[doc + 1];
  for (long long base = I.doc_ptr[doc]; base < end && !found; base += kPhLanes) {
    const int len = near_run_len(base, end, dist);
    CHECK(len >= 1 && len <= kNearStage && len <= kPhLanes + dist && base + len <= end, "a run of %d tokens", len);
    std::vector<int> run((size_t)len);  // the staged run, at exactly its size
    for (int lane = 0; lane < kPhLanes; ++lane)
      for (int j = lane; j < len; j += kPhLanes) run[(size_t)j] = I.tokens[base + j];
    for (int lane = 0; lane < kPhLanes; ++lane)
      found = near_lane_hit(run.data(), len, lane, terms, L, kind == kSpanNearOrdered, dist) || found;
    ++rounds_walked, longest_run = std::max<long long>(longest_run, len);
  }
  return found;
}

// the three launches of phrase_scope.hip on the CPU, on arrays of the sizes amdr_span_lists_plan / the caller promise
Lists run_items(const Corpus& c, const std::vector<Item>& items, long long cand_max, long long rows_cap) {
  const PhIndex I = c.index();
  const long n = (long)items.size();
  std::vector<long long> pp(n + 1, 0);
  std::vector<int> pt, kd, ds;
  for (long p = 0; p < n; ++p) {
    pt.insert(pt.end(), items[p].terms.begin(), items[p].terms.end()), pp[p + 1] = (long long)pt.size();
    kd.push_back(items[p].kind), ds.push_back(items[p].dist);
  }
  const std::vector<int> terms_all = exact(pt), kind = exact(kd), dist = exact(ds);
  const long long tiles = ph_tiles(cand_max);
  const size_t cells = (size_t)n * (size_t)tiles;
  std::vector<long long> counts(cells), offsets(cells + 1);
  std::vector<int> rank(cells * kPhTile, -7);
  Lists r;
  r.ptr.assign(n + 1, -7), r.docs.assign((size_t)rows_cap, -7), r.status.assign(n, -7);
  for (long p = 0; p < n; ++p) {  // count
    const long long L = pp[p + 1] - pp[p];
    int terms[kPhMaxLen];  // the block's copy: kPhMaxLen ints, filled only for an item the rule defines
    const bool sized = span_sized(kind[p], L, dist[p]);
    for (long long j = 0; sized && j < L; ++j) terms[j] = terms_all[(size_t)(pp[p] + j)];
    const PhDriver D = sized ? ph_driver(I, terms, L) : PhDriver{-1, -1, 0, 0};
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
        if (i < D.len && ph_has_all(I, terms, (int)L, D, I.post_doc[D.begin + i]))
          keep = walk_document(I, terms, (int)L, kind[p], dist[p], I.post_doc[D.begin + i]);
        rank[cell * kPhTile + t] = keep ? run : -1;
        run += keep ? 1 : 0;
      }
      counts[cell] = run;
    }
  }
  compact_scan_host(counts.data(), (long)cells, offsets.data());
  for (long p = 0; p < n; ++p) {  // write
    const PhDriver D = span_driver(I, terms_all.data() + pp[p], pp[p + 1] - pp[p], kind[p], dist[p]);
    const long long b = offsets[(size_t)p * tiles], e = offsets[(size_t)(p + 1) * tiles];
    r.ptr[p] = std::min(b, rows_cap);
    if (p == n - 1) r.ptr[n] = std::min(e, rows_cap);
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
  if (n == 0) r.ptr[0] = 0;
  return r;
}

// Nears of both kinds drawn from a document's window (a hit there) or at random, with repeats, 2 .. 8 tokens, distances
// 1 .. 12 and the edges 64, 254, 255; every fifth item a phrase; every eleventh with an id outside the vocabulary.
std::vector<Item> make_items(const Corpus& c, long count, uint64_t seed) {
  Rng r{seed};
  std::vector<Item> out;
  const int edges[] = {64, 254, kNearMaxDist, 63, 65};
  while ((long)out.size() < count) {
    const long k = (long)out.size();
    Item it;
    it.kind = k % 5 == 4 ? kSpanPhrase : (k % 2 ? kSpanNearOrdered : kSpanNearUnordered);
    const long M = k % 7 == 6 ? kNearMaxTerms : 2 + r.below(3);
    it.dist = it.kind == kSpanPhrase ? 0 : (k % 6 == 5 ? edges[r.below(5)] : 1 + (int)r.below(12));
    if (k % 3 == 2) {
      for (long j = 0; j < M; ++j) it.terms.push_back((int)r.below(c.n_terms));  // (the last term is in no document)
    } else {
      const std::vector<int>& seq = c.docs[r.below(c.n_docs)];
      if ((long)seq.size() < M) continue;
      const long s = k % 2 ? (long)seq.size() - M : r.below((long)seq.size() - M + 1);  // every other one at the end
      it.terms.assign(seq.begin() + s, seq.begin() + s + M);
      if (it.kind == kSpanNearUnordered) std::reverse(it.terms.begin(), it.terms.end());
    }
    if (k % 11 == 10) it.terms[r.below(M)] = k % 2 ? -1 : (int)c.n_terms;  // an id outside the vocabulary, at any position
    out.push_back(it);
  }
  return out;
}

void family(long n_docs, long n_items, uint64_t seed) {
  const std::string name = "nears n=" + std::to_string(n_docs) + " count=" + std::to_string(n_items);
  const Corpus c = make_corpus(n_docs, 9, seed);
  const std::vector<Item> items = make_items(c, n_items, seed + 1);
  std::vector<std::vector<int>> want;
  long long cand_max = 0, total = 0, ub_sum = 0;
  const PhIndex I = c.index();
  rounds_walked = longest_run = 0;
  for (const auto& it : items) {
    want.push_back(naive_list(c, it));
    const long long len = span_driver(I, it.terms.data(), (long long)it.terms.size(), it.kind, it.dist).len;
    cand_max = std::max(cand_max, len), ub_sum += len, total += (long long)want.back().size();
    CHECK((long long)want.back().size() <= len, "%s: a list longer than its driver", name.c_str());
  }
  const Lists r = run_items(c, items, cand_max, ub_sum);  // the bounds the header promises suffice
  bool same = r.ptr[n_items] == total;
  for (long p = 0; p < n_items && same; ++p) {
    same = r.status[p] == kTsOk && std::vector<int>(r.docs.begin() + r.ptr[p], r.docs.begin() + r.ptr[p + 1]) == want[p];
    if (!same) CHECK(false, "%s: item %ld (kind %d, %zu tokens, distance %d) differs from the naive scan", name.c_str(), p,
                     items[p].kind, items[p].terms.size(), items[p].dist);
  }
  CHECK(same, "%s: the lists differ from the naive scan", name.c_str());
  for (size_t i = (size_t)total; i < r.docs.size(); ++i) CHECK(r.docs[i] == -7, "%s: a write past the lists", name.c_str());
  long longest = 0;  // one below either bound
  for (long p = 0; p < n_items; ++p)
    if (span_driver(I, items[p].terms.data(), (long long)items[p].terms.size(), items[p].kind, items[p].dist).len == cand_max) longest = p;
  if (cand_max > 0) {
    const Lists s = run_items(c, items, cand_max - 1, ub_sum);
    CHECK(s.status[longest] == kTsCandOverflow && s.ptr[longest + 1] == s.ptr[longest], "%s: cand_max - 1", name.c_str());
  }
  if (total > 0) {
    const Lists s = run_items(c, items, cand_max, total - 1);
    long flagged = 0;
    for (long p = 0; p < n_items; ++p) flagged += s.status[p] == kTsRowsOverflow;
    CHECK(flagged >= 1 && s.ptr[n_items] == total - 1, "%s: rows_cap - 1", name.c_str());
    CHECK(std::equal(s.docs.begin(), s.docs.end(), r.docs.begin()), "%s: rows_cap - 1 changed the documents that fit", name.c_str());
  }
  std::printf("%s: %lld documents in the lists, longest driver %lld, longest staged run %lld\n", name.c_str(), total, cand_max,
              longest_run);
  if (failures == 0) std::printf("family ok\n");
}

// hand-made sequences: the identities and the anchor argument, one document each, through the same walk
void written_out() {
  struct Case {
    std::vector<int> seq;
    Item it;
    bool want;
  };
  const int a = 0, b = 1, x = 2;
  std::vector<Case> cases = {
      {{a, a, b}, {kSpanNearOrdered, {a, b}, 1}, true},          // only from the second anchor
      {{a, x, x, b, a}, {kSpanNearUnordered, {a, b}, 1}, true},  // the window starts at b
      {{a, x, x, b, a}, {kSpanNearOrdered, {a, b}, 1}, false},
      {{b, x, a}, {kSpanNearUnordered, {a, b}, 2}, true},
      {{b, x, a}, {kSpanNearOrdered, {a, b}, 2}, false},
      {{a, x}, {kSpanNearUnordered, {a, a}, 3}, false},
      {{a, x, a}, {kSpanNearUnordered, {a, a}, 2}, true},
      {{a, x, x, a}, {kSpanNearUnordered, {a, a}, 2}, false},
      {{a, b, a}, {kSpanNearUnordered, {a, a, b}, 2}, true},
      {{a, b}, {kSpanNearUnordered, {a, a, b}, 9}, false},
      {{a, b, a}, {kSpanNearOrdered, {a, b, a}, 2}, true},
      {{a, a, b}, {kSpanNearOrdered, {a, b, a}, 3}, false},
      {{a, a, a, a, a, a, a, a}, {kSpanNearUnordered, {a, a, a, a, a, a, a, a}, 7}, true},
      {{a, a, a, a, x, a, a, a, a}, {kSpanNearOrdered, {a, a, a, a, a, a, a, a}, 7}, false},
  };
  for (int gap : {1, 2, 64, 255})  // exactly n apart, n + 1 apart, across the rounds
    for (int lead : {0, 62, 63, 64, 127}) {
      std::vector<int> seq((size_t)lead, x);
      seq.push_back(a);
      seq.insert(seq.end(), (size_t)gap - 1, x);
      seq.push_back(b);
      cases.push_back({seq, {kSpanNearOrdered, {a, b}, gap}, true});
      cases.push_back({seq, {kSpanNearUnordered, {b, a}, gap}, true});
      if (gap > 1) cases.push_back({seq, {kSpanNearUnordered, {a, b}, gap - 1}, false});
    }
  long n = 0;
  for (const Case& k : cases) {
    Corpus c;
    c.n_docs = 2, c.n_terms = 3, c.docs = {k.seq, {b, a, b, a}};  // the neighbour holds what the case lacks: never reached
    std::vector<long long> tp{0}, dp{0};
    std::vector<int> pd, tk;
    for (int t = 0; t < 3; ++t) {
      for (long d = 0; d < 2; ++d)
        if (std::find(c.docs[d].begin(), c.docs[d].end(), t) != c.docs[d].end()) pd.push_back((int)d);
      tp.push_back((long long)pd.size());
    }
    for (long d = 0; d < 2; ++d) tk.insert(tk.end(), c.docs[d].begin(), c.docs[d].end()), dp.push_back((long long)tk.size());
    c.term_ptr = exact(tp), c.doc_ptr = exact(dp), c.post_doc = exact(pd), c.tokens = exact(tk);
    const bool got = walk_document(c.index(), k.it.terms.data(), (int)k.it.terms.size(), k.it.kind, k.it.dist, 0);
    CHECK(got == k.want && naive_near(k.seq, k.it) == k.want, "written-out case %ld", n);
    ++n;
  }
  if (failures == 0) std::printf("written-out ok\n");
}

void validation() {
  const int64_t pp[] = {0, 2, 5, 7}, pp_off[] = {1, 2, 5, 7}, pp_down[] = {0, 3, 2, 7}, pp_one[] = {0, 1, 5, 7};
  const int64_t pp_nine[] = {0, 9, 12, 14}, pp_17[] = {0, 2, 5, 22};
  const int32_t pt[22] = {0};
  const int32_t kd[] = {1, 2, 0}, kd_bad[] = {1, 3, 0}, kd_neg[] = {-1, 2, 0}, kd_phr[] = {0, 2, 0};
  const int32_t ds[] = {1, 255, -9}, ds_zero[] = {0, 255, 0}, ds_big[] = {1, 256, 0};
  CHECK(span_validate(pp, pt, kd, ds, 3) == kPhValid, "valid items (a phrase's distance is not read)");
  CHECK(span_validate(pp, pt, kd, ds, -1) == kPhSizes, "n_items < 0");
  CHECK(span_validate(nullptr, pt, kd, ds, 3) == kPhNull && span_validate(pp, nullptr, kd, ds, 3) == kPhNull, "null arrays");
  CHECK(span_validate(pp, pt, nullptr, ds, 3) == kPhNull && span_validate(pp, pt, kd, nullptr, 3) == kPhNull, "null kind / dist");
  CHECK(span_validate(pp_off, pt, kd, ds, 3) == kPhPtr && span_validate(pp_down, pt, kd, ds, 3) == kPhPtr, "item_ptr");
  CHECK(span_validate(pp, pt, kd_bad, ds, 3) == kNearKind && span_validate(pp, pt, kd_neg, ds, 3) == kNearKind, "a kind outside 0 .. 2");
  CHECK(span_validate(pp_one, pt, kd, ds, 3) == kNearLength && span_validate(pp_nine, pt, kd, ds, 3) == kNearLength, "a Near length outside 2 .. 8");
  CHECK(span_validate(pp_nine, pt, kd_phr, ds, 3) == kPhValid, "nine tokens are a phrase's to have");
  CHECK(span_validate(pp_17, pt, kd, ds, 3) == kPhLength && span_validate(pp_one, pt, kd_phr, ds, 3) == kPhLength, "a phrase length outside 2 .. 16");
  CHECK(span_validate(pp, pt, kd, ds_zero, 3) == kNearDist && span_validate(pp, pt, kd, ds_big, 3) == kNearDist, "a distance outside 1 .. 255");
  CHECK(span_validate(pp, nullptr, nullptr, nullptr, 0) == kPhValid, "no item reads nothing");
  for (int e : {(int)kNearKind, (int)kNearLength, (int)kNearDist, (int)kPhPtr, (int)kPhLength})
    CHECK(std::string(span_error_text(e)) != "ok", "an error without words");
  // an unknown id, or a size outside the rule, makes the driver empty without reading the index: its arrays are null
  const PhIndex none{nullptr, nullptr, 5, 9, nullptr, nullptr};
  const int bad_lo[] = {2, -1, 3}, bad_hi[] = {2, 3, 5}, nine[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
  CHECK(span_driver(none, bad_lo, 3, kSpanNearUnordered, 5).at < 0 && span_driver(none, bad_hi, 3, kSpanNearOrdered, 5).at < 0, "an unknown id reads nothing");
  CHECK(span_driver(none, nine, 1, kSpanNearUnordered, 5).at < 0 && span_driver(none, nine, 9, kSpanNearOrdered, 5).at < 0, "a length outside 2 .. 8 reads nothing");
  CHECK(span_driver(none, nine, 2, kSpanNearUnordered, 0).at < 0 && span_driver(none, nine, 2, kSpanNearOrdered, 256).at < 0, "a distance outside 1 .. 255 reads nothing");
  CHECK(span_driver(none, nine, 2, 3, 5).at < 0 && span_driver(none, nine, 2, -1, 5).at < 0, "a kind outside 0 .. 2 reads nothing");
  CHECK(near_run_len(0, 1000, 255) == kNearStage && near_run_len(10, 12, 255) == 2 && near_run_len(0, 65, 1) == 65, "run lengths");
  if (failures == 0) std::printf("validate ok\n");
}

}  // namespace

int main() {
  const long sizes[] = {40, 300, 900};
  const long counts[] = {1, 2, 65};
  for (long n : sizes)
    for (long k : counts) family(n, k, 2000 + (uint64_t)n * 7 + (uint64_t)k);
  written_out();
  validation();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("near rule ok\n");
  return 0;
}

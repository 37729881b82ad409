// Host check of the rules of amdr_class_spans (class_span_rule.hpp, over near_rule.hpp's sizes and run length; the host
// scans of compact.hpp), a program of its own:
//   check_class_span
// It resolves generated items — phrases and Nears of both kinds whose slots are plain tokens and token classes — tile by
// tile, round by round and lane by lane as the kernels of class_span.hip do: the slots resolved and linked, the driver
// among posting lists and class lists, the conjunction per candidate, per surviving document one round of kPhLanes anchors
// after the other, each from MASKS staged in an array of exactly cs_run_len unsigned shorts, the counts, the scan, the
// write behind the lists that stand before — and compares the lists with a naive scan of every window of every document
// that decides the unordered form by a bipartite matching.  Every array has exactly the size the header promises, so with
// the host sanitizers (tests/test_class_span_rule_host.py) an access outside one is a failure.  Then the written-out cases,
// the counter-example of the overlap rule among them, and every refusal of cs_validate.
// Build: c++ -std=c++17 check_class_span.cpp (plain host code; no HIP header is needed).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#define AMDR_COMPACT_HOST_ONLY 1  // the host forms alone: this program has no device code
#include "class_span_rule.hpp"
#include "compact.hpp"
#include "union_rule.hpp"

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

constexpr long kTerms = 14;    // terms 0 .. 12 occur, weight 1 / (t + 1); term 13 is in no document
constexpr long kClsFirst = 2;  // two lists of a span step stand before the classes'

// The classes of every corpus.  0, 1, 2, 3, 5, 7 and the plain tokens 5, 11, 12, 13 are pairwise equal or disjoint (3
// equals 0 under another id; the plain token 5 equals class 2): the slots of the unordered items.  4, 6 and 8 overlap
// others: for phrases and ordered Nears only.  8 holds an id outside the vocabulary.
const std::vector<std::vector<int>> kClasses = {{0, 1}, {2, 3, 4}, {5}, {0, 1}, {1, 2}, {}, {6, 7, 8, 9, 10}, {13}, {6, 1000}};

struct Corpus {
  long n_docs;
  std::vector<std::vector<int>> docs;  // the naive scan's own form
  std::vector<long long> term_ptr, doc_ptr, cls_ptr, x_ptr;
  std::vector<int> post_doc, tokens, cls_terms, x_doc;  // x_doc: the lists before the items', at exactly their size
  long n_before() const { return kClsFirst + (long)kClasses.size(); }
};

bool class_has(int c, int x) { return std::find(kClasses[(size_t)c].begin(), kClasses[(size_t)c].end(), x) != kClasses[(size_t)c].end(); }

// the naive predicate: slot id s against token x
bool slot_fills(int s, int x) {
  if (s >= 0 && s < kTerms) return s == x;
  const long c = (long)s - kTerms - kClsFirst;
  return c >= 0 && c < (long)kClasses.size() && class_has((int)c, x);
}
bool slot_known(int s) { return s >= 0 && s < kTerms + kClsFirst + (long)kClasses.size() && !(s >= kTerms && s < kTerms + kClsFirst); }

Corpus make_corpus(long n_docs, uint64_t seed) {
  Corpus c;
  c.n_docs = n_docs;
  Rng r{seed};
  const long special[] = {63, 64, 65, 127, 128, 129, 1200, 0, 1, 319, 320, 400};
  std::vector<long> cum;
  long total = 0;
  for (long t = 0; t + 1 < kTerms; ++t) cum.push_back(total += 1000 / (t + 1));
  for (long d = 0; d < n_docs; ++d) {
    const long len = d < 12 ? special[d] : r.below(91);
    std::vector<int> seq;
    for (long i = 0; i < len; ++i) seq.push_back((int)(std::upper_bound(cum.begin(), cum.end(), r.below(total)) - cum.begin()));
    c.docs.push_back(seq);
  }
  std::vector<long long> tp(kTerms + 1, 0), dp(n_docs + 1, 0), cp{0}, xp{0};
  std::vector<int> pd, tk, ct, xd;
  for (long t = 0; t < kTerms; ++t) {
    for (long d = 0; d < n_docs; ++d)
      if (std::find(c.docs[d].begin(), c.docs[d].end(), (int)t) != c.docs[d].end()) pd.push_back((int)d);
    tp[t + 1] = (long long)pd.size();
  }
  for (long d = 0; d < n_docs; ++d) tk.insert(tk.end(), c.docs[d].begin(), c.docs[d].end()), dp[d + 1] = (long long)tk.size();
  for (long k = 0; k < kClsFirst; ++k) {  // what a span step left: every (k + 3)-th document
    for (long d = k; d < n_docs; d += k + 3) xd.push_back((int)d);
    xp.push_back((long long)xd.size());
  }
  for (size_t k = 0; k < kClasses.size(); ++k) {  // what the union step leaves: the documents that hold a member
    ct.insert(ct.end(), kClasses[k].begin(), kClasses[k].end()), cp.push_back((long long)ct.size());
    for (long d = 0; d < n_docs; ++d)
      if (std::any_of(c.docs[d].begin(), c.docs[d].end(), [&](int x) { return class_has((int)k, x); })) xd.push_back((int)d);
    xp.push_back((long long)xd.size());
  }
  c.term_ptr = exact(tp), c.doc_ptr = exact(dp), c.post_doc = exact(pd), c.tokens = exact(tk);
  c.cls_ptr = exact(cp), c.cls_terms = exact(ct), c.x_ptr = exact(xp), c.x_doc = exact(xd);
  return c;
}

struct Item {
  int kind;
  std::vector<int> slots;
  int dist;
};

// the unordered form as the matching it is: augmenting paths over the positions of one window
bool place(int j, const std::vector<std::vector<int>>& may, std::vector<int>& taken, std::vector<char>& seen) {
  for (int q : may[(size_t)j]) {
    if (seen[(size_t)q]) continue;
    seen[(size_t)q] = 1;
    if (taken[(size_t)q] < 0 || place(taken[(size_t)q], may, taken, seen)) {
      taken[(size_t)q] = j;
      return true;
    }
  }
  return false;
}

bool naive_holds(const std::vector<int>& seq, const Item& it) {
  const long M = (long)it.slots.size(), n = it.dist;
  if (it.kind == kSpanPhrase) {
    for (long p = 0; p + M <= (long)seq.size(); ++p) {
      bool all = true;
      for (long j = 0; j < M && all; ++j) all = slot_fills(it.slots[(size_t)j], seq[(size_t)(p + j)]);
      if (all) return true;
    }
    return false;
  }
  for (long s = 0; s < (long)seq.size(); ++s) {
    const long e = std::min<long>((long)seq.size(), s + n + 1);
    if (it.kind == kSpanNearOrdered) {
      if (!slot_fills(it.slots[0], seq[(size_t)s])) continue;  // (the span is measured from the first slot's position)
      long j = 1;
      for (long q = s + 1; q < e && j < M; ++q)
        if (slot_fills(it.slots[(size_t)j], seq[(size_t)q])) ++j;
      if (j == M) return true;
    } else {
      std::vector<std::vector<int>> may((size_t)M);
      for (long j = 0; j < M; ++j)
        for (long q = s; q < e; ++q)
          if (slot_fills(it.slots[(size_t)j], seq[(size_t)q])) may[(size_t)j].push_back((int)(q - s));
      std::vector<int> taken((size_t)(e - s), -1);
      bool all = true;
      for (long j = 0; j < M && all; ++j) {
        std::vector<char> seen((size_t)(e - s), 0);
        all = place((int)j, may, taken, seen);
      }
      if (all) return true;
    }
  }
  return false;
}

std::vector<int> naive_list(const Corpus& c, const Item& it) {
  std::vector<int> out;
  for (int s : it.slots)
    if (!slot_known(s)) return out;
  for (long d = 0; d < c.n_docs; ++d)
    if (naive_holds(c.docs[(size_t)d], it)) out.push_back((int)d);
  return out;
}

struct Lists {
  std::vector<long long> ptr;  // the whole array's: n_before + n + 1 entries
  std::vector<int> docs, status;
};

long long longest_run = 0;

// one surviving document, as one wave walks it
bool walk_document(const CsIndex& I, const CsSlot* slots, int L, int kind, int dist, long long doc) {
  bool found = false;
  const long long end = I.ph.doc_ptr[doc + 1];
  for (long long base = I.ph.doc_ptr[doc]; base < end && !found; base += kPhLanes) {
    const int len = cs_run_len(base, end, kind, L, dist);
    CHECK(len >= 1 && len <= kNearStage && base + len <= end, "a run of %d masks", len);
    std::vector<unsigned short> run((size_t)len);  // the staged masks, at exactly their size
    for (int lane = 0; lane < kPhLanes; ++lane)
      for (int j = lane; j < len; j += kPhLanes) run[(size_t)j] = (unsigned short)cs_token_mask(I.ph.tokens[base + j], slots, L, I.cls_terms);
    for (int lane = 0; lane < kPhLanes; ++lane) found = cs_lane_hit(run.data(), len, lane, L, kind, dist) || found;
    longest_run = std::max<long long>(longest_run, len);
  }
  return found;
}

// the block's item: the slots resolved, linked and given a driver; 0: an item the rule does not define
int block_item(const CsIndex& I, const std::vector<long long>& pp, const std::vector<int>& all, int kind, int dist, long p,
               CsSlot* slots, CsDriver* D) {
  const long long L = pp[(size_t)p + 1] - pp[(size_t)p];
  const bool sized = span_sized(kind, L, dist);
  for (long long j = 0; sized && j < L; ++j) slots[j] = cs_slot(I, all[(size_t)(pp[(size_t)p] + j)]);
  if (sized) cs_link_slots(slots, (int)L);
  *D = sized ? cs_driver(slots, (int)L) : CsDriver{-1, nullptr, 0, 0};
  return sized ? (int)L : 0;
}

// the three launches of class_span.hip on the CPU, on arrays of the sizes amdr_class_spans_plan / the caller promise; the
// docs array holds rows_cap ints and begins with the lists that stand before
Lists run_items(const Corpus& c, const std::vector<Item>& items, long long cand_max, long long rows_cap) {
  const long n = (long)items.size(), n_before = c.n_before();
  std::vector<long long> pp((size_t)n + 1, 0);
  std::vector<int> pt, kd, ds;
  for (long p = 0; p < n; ++p) {
    pt.insert(pt.end(), items[(size_t)p].slots.begin(), items[(size_t)p].slots.end()), pp[(size_t)p + 1] = (long long)pt.size();
    kd.push_back(items[(size_t)p].kind), ds.push_back(items[(size_t)p].dist);
  }
  const std::vector<int> slots_all = exact(pt), kind = exact(kd), dist = exact(ds);
  Lists r;
  r.ptr.assign((size_t)(n_before + n + 1), -7), r.docs.assign((size_t)rows_cap, -7), r.status.assign((size_t)n, -7);
  std::copy(c.x_ptr.begin(), c.x_ptr.end(), r.ptr.begin());
  for (size_t i = 0; i < c.x_doc.size() && i < r.docs.size(); ++i) r.docs[i] = c.x_doc[i];
  const CsIndex I{PhIndex{c.term_ptr.data(), c.post_doc.data(), kTerms, c.n_docs, c.doc_ptr.data(), c.tokens.data()},
                  r.ptr.data(), r.docs.data(), c.cls_ptr.data(), c.cls_terms.data(), (long)kClasses.size(), kClsFirst};
  long long cells = 0;
  CHECK(cs_cells(n, cand_max, &cells), "the cells of the launch");
  const long long tiles = ph_tiles(cand_max);
  std::vector<long long> counts((size_t)cells), offsets((size_t)cells + 1);
  std::vector<int> rank((size_t)cells * kPhTile, -7);
  for (long long cell = 0; cell < cells; ++cell) {  // count
    const long long p = cell / tiles, tile = cell - p * tiles;
    CsSlot slots[kPhMaxLen];
    CsDriver D;
    const int L = block_item(I, pp, slots_all, kind[(size_t)p], dist[(size_t)p], (long)p, slots, &D);
    const bool over = D.len > cand_max;
    if (tile == 0) r.status[(size_t)p] = over ? kTsCandOverflow : kTsOk;
    const long long i0 = tile * kPhTile;
    if (over || D.at < 0 || i0 >= D.len) {
      counts[(size_t)cell] = 0;
      continue;
    }
    int run = 0;
    for (int t = 0; t < kPhTile; ++t) {
      const long long i = i0 + t;
      bool keep = false;
      if (i < D.len && cs_has_all(slots, L, D, D.docs[D.begin + i]))
        keep = walk_document(I, slots, L, kind[(size_t)p], dist[(size_t)p], D.docs[D.begin + i]);
      rank[(size_t)cell * kPhTile + t] = keep ? run : -1;
      run += keep ? 1 : 0;
    }
    counts[(size_t)cell] = run;
  }
  compact_scan_host(counts.data(), (long)cells, offsets.data());
  for (long long cell = 0; cell < cells; ++cell) {  // write
    const long long p = cell / tiles, tile = cell - p * tiles;
    const long long start = r.ptr[(size_t)n_before];
    if (tile == 0) {
      const long long begin = start + offsets[(size_t)(p * tiles)], end = start + offsets[(size_t)((p + 1) * tiles)];
      r.ptr[(size_t)(n_before + p + 1)] = un_clamp(end, rows_cap);
      if (un_status(begin, end, rows_cap) != kTsOk) r.status[(size_t)p] = kTsRowsOverflow;
    }
    CsSlot slots[kPhMaxLen];
    CsDriver D;
    (void)block_item(I, pp, slots_all, kind[(size_t)p], dist[(size_t)p], (long)p, slots, &D);
    const long long i0 = tile * kPhTile;
    if (D.len > cand_max || D.at < 0 || i0 >= D.len) continue;
    for (int t = 0; t < kPhTile; ++t) {
      const int rk = rank[(size_t)cell * kPhTile + t];
      if (rk < 0) continue;
      const long long at = start + offsets[(size_t)cell] + rk;
      if (at < rows_cap) r.docs[(size_t)at] = D.docs[D.begin + i0 + t];
    }
  }
  return r;
}

// Items of the three kinds over plain tokens and classes: a slot drawn from a document's window (a hit there: the token
// itself or a class that holds it) or at random; 2 .. 8 slots (phrases up to 16), distances 1 .. 12 and the edges; every
// eleventh with an unknown slot id.  The slots of an unordered item come from the equal-or-disjoint family alone.
std::vector<Item> make_items(const Corpus& c, long count, uint64_t seed) {
  Rng r{seed};
  std::vector<Item> out;
  const int edges[] = {64, 254, kNearMaxDist, 63, 65};
  const int C = (int)(kTerms + kClsFirst);
  const std::vector<int> family = {C + 0, C + 1, C + 2, C + 3, C + 5, C + 7, 5, 11, 12, 13};
  const std::vector<int> any = {C + 0, C + 1, C + 2, C + 3, C + 4, C + 5, C + 6, C + 7, C + 8, 0, 1, 2, 3, 6, 9};
  while ((long)out.size() < count) {
    const long k = (long)out.size();
    Item it;
    it.kind = k % 5 == 4 ? kSpanPhrase : (k % 2 ? kSpanNearOrdered : kSpanNearUnordered);
    const std::vector<int>& pool = it.kind == kSpanNearUnordered ? family : any;
    const long M = k % 7 == 6 ? (it.kind == kSpanPhrase ? kPhMaxLen : kNearMaxTerms) : 2 + r.below(3);
    it.dist = it.kind == kSpanPhrase ? 0 : (k % 6 == 5 ? edges[r.below(5)] : 1 + (int)r.below(12));
    if (k % 3 == 2) {
      for (long j = 0; j < M; ++j) it.slots.push_back(pool[(size_t)r.below((long)pool.size())]);
    } else {
      const std::vector<int>& seq = c.docs[(size_t)r.below(c.n_docs)];
      if ((long)seq.size() < M) continue;
      const long s = k % 2 ? (long)seq.size() - M : r.below((long)seq.size() - M + 1);  // every other one at the end
      for (long j = 0; j < M; ++j) {
        const int x = seq[(size_t)(s + j)];
        std::vector<int> fit;  // the pool's slots the token fills
        for (int cand : pool)
          if (slot_fills(cand, x)) fit.push_back(cand);
        it.slots.push_back(fit.empty() ? pool[0] : fit[(size_t)r.below((long)fit.size())]);
      }
      if (it.kind == kSpanNearUnordered) std::reverse(it.slots.begin(), it.slots.end());
    }
    if (k % 11 == 10) it.slots[(size_t)r.below(M)] = k % 2 ? -1 : (k % 4 ? (int)kTerms : C + (int)kClasses.size());
    out.push_back(it);
  }
  return out;
}

long long driver_len(const Corpus& c, const Item& it) {
  const CsIndex I{PhIndex{c.term_ptr.data(), c.post_doc.data(), kTerms, c.n_docs, c.doc_ptr.data(), c.tokens.data()},
                  c.x_ptr.data(), c.x_doc.data(), c.cls_ptr.data(), c.cls_terms.data(), (long)kClasses.size(), kClsFirst};
  std::vector<long long> pp = {0, (long long)it.slots.size()};
  CsSlot slots[kPhMaxLen];
  CsDriver D;
  (void)block_item(I, pp, it.slots, it.kind, it.dist, 0, slots, &D);
  return D.len;
}

void family(long n_docs, long n_items, uint64_t seed) {
  const std::string name = "class spans n=" + std::to_string(n_docs) + " count=" + std::to_string(n_items);
  const Corpus c = make_corpus(n_docs, seed);
  const std::vector<Item> items = make_items(c, n_items, seed + 1);
  std::vector<std::vector<int>> want;
  long long cand_max = 0, total = 0, ub_sum = 0, classy = 0;
  longest_run = 0;
  for (const auto& it : items) {
    want.push_back(naive_list(c, it));
    const long long len = driver_len(c, it);
    cand_max = std::max(cand_max, len), ub_sum += len, total += (long long)want.back().size();
    classy += std::any_of(it.slots.begin(), it.slots.end(), [](int s) { return s >= kTerms; });
    CHECK((long long)want.back().size() <= len, "%s: a list longer than its driver", name.c_str());
  }
  const long long before = (long long)c.x_doc.size();
  const long n_before = c.n_before();
  const Lists r = run_items(c, items, cand_max, before + ub_sum);  // the bounds the header promises suffice
  bool same = r.ptr[(size_t)(n_before + n_items)] == before + total;
  for (long p = 0; p < n_items && same; ++p) {
    const long long b = r.ptr[(size_t)(n_before + p)], e = r.ptr[(size_t)(n_before + p + 1)];
    same = r.status[(size_t)p] == kTsOk && std::vector<int>(r.docs.begin() + b, r.docs.begin() + e) == want[(size_t)p];
    if (!same) CHECK(false, "%s: item %ld (kind %d, %zu slots, distance %d) differs from the naive scan", name.c_str(), p,
                     items[(size_t)p].kind, items[(size_t)p].slots.size(), items[(size_t)p].dist);
  }
  CHECK(same, "%s: the lists differ from the naive scan", name.c_str());
  CHECK(std::equal(c.x_ptr.begin(), c.x_ptr.end(), r.ptr.begin()) && std::equal(c.x_doc.begin(), c.x_doc.end(), r.docs.begin()),
        "%s: the lists that stood before changed", name.c_str());
  for (size_t i = (size_t)(before + total); i < r.docs.size(); ++i) CHECK(r.docs[i] == -7, "%s: a write past the lists", name.c_str());
  long longest = 0;  // one below either bound
  for (long p = 0; p < n_items; ++p)
    if (driver_len(c, items[(size_t)p]) == cand_max) longest = p;
  if (cand_max > 0) {
    const Lists s = run_items(c, items, cand_max - 1, before + ub_sum);
    CHECK(s.status[(size_t)longest] == kTsCandOverflow && s.ptr[(size_t)(n_before + longest + 1)] == s.ptr[(size_t)(n_before + longest)],
          "%s: cand_max - 1", name.c_str());
  }
  if (total > 0) {
    const Lists s = run_items(c, items, cand_max, before + total - 1);
    long flagged = 0;
    for (long p = 0; p < n_items; ++p) flagged += s.status[(size_t)p] == kTsRowsOverflow;
    CHECK(flagged >= 1 && s.ptr[(size_t)(n_before + n_items)] == before + total - 1, "%s: rows_cap - 1", name.c_str());
    CHECK(std::equal(s.docs.begin(), s.docs.end(), r.docs.begin()), "%s: rows_cap - 1 changed the documents that fit", name.c_str());
  }
  std::printf("%s: %lld documents in the lists, %lld items with a class, longest driver %lld, longest staged run %lld\n",
              name.c_str(), total, classy, cand_max, longest_run);
  if (failures == 0) std::printf("family ok\n");
}

// hand-made sequences, one document each, through cs_token_mask and cs_lane_hit
bool hit_anywhere(const std::vector<std::vector<int>>& sets, const std::vector<int>& seq, int kind, int dist) {
  // slots given as id sets: class c = sets[c], slot id 1000 + c over a vocabulary of 1000 plain tokens
  std::vector<long long> cp{0};
  std::vector<int> ct;
  for (const auto& s : sets) ct.insert(ct.end(), s.begin(), s.end()), cp.push_back((long long)ct.size());
  const std::vector<long long> cpe = exact(cp), xp((size_t)sets.size() + 1, 0);
  const std::vector<int> cte = exact(ct);
  const CsIndex I{PhIndex{nullptr, nullptr, 1000, 1, nullptr, nullptr}, xp.data(), nullptr, cpe.data(), cte.data(), (long)sets.size(), 0};
  CsSlot slots[kPhMaxLen];
  const int L = (int)sets.size();
  for (int j = 0; j < L; ++j) slots[j] = cs_slot(I, 1000 + j);
  cs_link_slots(slots, L);
  bool found = false;
  const long long end = (long long)seq.size();
  for (long long base = 0; base < end && !found; base += kPhLanes) {
    const int len = cs_run_len(base, end, kind, L, dist);
    std::vector<unsigned short> run((size_t)len);
    for (int j = 0; j < len; ++j) run[(size_t)j] = (unsigned short)cs_token_mask(seq[(size_t)(base + j)], slots, L, cte.data());
    for (int lane = 0; lane < kPhLanes; ++lane) found = cs_lane_hit(run.data(), len, lane, L, kind, dist) || found;
  }
  return found;
}

void written_out() {
  const int a = 0, b = 1, x = 2, y = 3;
  struct Case {
    std::vector<std::vector<int>> sets;
    std::vector<int> seq;
    int kind, dist;
    bool want;
  };
  std::vector<Case> cases = {
      {{{a, b}, {a, b}}, {a, x, b}, kSpanNearUnordered, 2, true},    // equal slots take two positions ...
      {{{a, b}, {a, b}}, {a, x, x}, kSpanNearUnordered, 2, false},   // ... one token does not fill both
      {{{a, b}, {a, b}}, {a, x, x, b}, kSpanNearUnordered, 2, false},
      {{{a, b}, {x}}, {x, b}, kSpanNearUnordered, 1, true},          // any slot's token anchors the window
      {{{a, b}, {x}}, {x, y, b}, kSpanNearUnordered, 1, false},
      {{{a, b}, {x}}, {x, b}, kSpanNearOrdered, 1, false},           // the order given
      {{{a, b}, {x}}, {b, x}, kSpanNearOrdered, 1, true},
      {{{a, b}, {a}}, {a, a}, kSpanNearOrdered, 1, true},            // overlapping slots are the ordered form's to have
      {{{a, b}, {a}}, {b, a}, kSpanNearOrdered, 1, true},
      {{{a, b}, {a}}, {a, b}, kSpanNearOrdered, 1, false},
      {{{a, b}, {a}}, {a, a, b}, kSpanPhrase, 0, true},
      {{{a, b}, {a}}, {a, b, b}, kSpanPhrase, 0, false},
      {{{a}, {b}}, {a, b}, kSpanPhrase, 0, true},
      {{{a}, {b}}, {y, a}, kSpanPhrase, 0, false},                   // a phrase never leaves the document
      {{{a, b}, {a, b}, {x}}, {b, x, a}, kSpanNearUnordered, 2, true},
      {{{a, b}, {a, b}, {x}}, {b, x, y, a}, kSpanNearUnordered, 2, false},
  };
  for (int gap : {1, 2, 64, 255})  // exactly n apart, n + 1 apart, across the rounds; the anchor in lane 63 among them
    for (int lead : {0, 62, 63, 64, 127}) {
      std::vector<int> seq((size_t)lead, y);
      seq.push_back(a);
      seq.insert(seq.end(), (size_t)gap - 1, y);
      seq.push_back(x);
      cases.push_back({{{a, b}, {x}}, seq, kSpanNearOrdered, gap, true});
      cases.push_back({{{x}, {a, b}}, seq, kSpanNearUnordered, gap, true});
      if (gap > 1) cases.push_back({{{a, b}, {x}}, seq, kSpanNearUnordered, gap - 1, false});
    }
  long n = 0;
  for (const Case& k : cases) {
    CHECK(hit_anywhere(k.sets, k.seq, k.kind, k.dist) == k.want, "written-out case %ld", n);
    ++n;
  }
  // The counter-example of the overlap rule: slots {a, b}, {a} on the tokens a b.  The matching exists (b -> slot 0,
  // a -> slot 1); the first-unfilled-slot tally gives a to slot 0 and finds nothing for slot 1.  cs_validate refuses it.
  CHECK(!hit_anywhere({{a, b}, {a}}, {a, b}, kSpanNearUnordered, 1), "the tally on overlapping slots");
  // a class of 4 096 ids: its first and its last member, and what lies just outside
  std::vector<int> big;
  for (int i = 0; i < 4096; ++i) big.push_back(10 + 2 * i);
  for (int t : {10, 10 + 2 * 4095}) CHECK(hit_anywhere({big, {a}}, {t, a}, kSpanPhrase, 0), "a member at the edge of 4 096");
  for (int t : {9, 11, 10 + 2 * 4095 + 1, 10 + 2 * 4096}) CHECK(!hit_anywhere({big, {a}}, {t, a}, kSpanPhrase, 0), "beside the members");
  if (failures == 0) std::printf("written-out ok\n");
}

void validation() {
  const int64_t V = 10;
  const int64_t pp[] = {0, 2, 5, 7}, pp_off[] = {1, 2, 5, 7}, pp_nine[] = {0, 9, 12, 14};
  const int32_t kd[] = {1, 2, 0}, kd_bad[] = {1, 3, 0}, ds[] = {1, 255, -9}, ds_big[] = {1, 256, 0};
  const int64_t cp[] = {0, 2, 3, 5}, cp_off[] = {1, 2, 3, 5}, cp_down[] = {0, 3, 2, 5};
  const int32_t ct[] = {1, 4, 1, 2, 3}, ct_same[] = {1, 1, 1, 2, 3}, ct_down[] = {4, 1, 1, 2, 3};
  // classes: 0 = {1, 4}, 1 = {1}, 2 = {2, 3}.  Item 0 is the unordered one.
  const int32_t ok[] = {10, 12, 0, 1, 2, 3, 4}, equal_ids[] = {10, 10, 0, 1, 2, 3, 4}, equal_sets[] = {11, 1, 0, 1, 2, 3, 4};
  const int32_t overlap[] = {10, 11, 0, 1, 2, 3, 4}, plain_in[] = {10, 4, 0, 1, 2, 3, 4}, unknown[] = {10, 99, 0, 1, 2, 3, 4};
  const int32_t ordered_overlap[] = {2, 3, 10, 11, 1, 10, 11};
  CHECK(cs_validate(pp, ok, kd, ds, 3, cp, ct, 3, V) == kPhValid, "valid items");
  CHECK(cs_validate(pp, equal_ids, kd, ds, 3, cp, ct, 3, V) == kPhValid && cs_validate(pp, equal_sets, kd, ds, 3, cp, ct, 3, V) == kPhValid,
        "equal slots, by id and by set");
  CHECK(cs_validate(pp, overlap, kd, ds, 3, cp, ct, 3, V) == kCsOverlap && cs_validate(pp, plain_in, kd, ds, 3, cp, ct, 3, V) == kCsOverlap,
        "overlapping unequal slots in an unordered item");
  CHECK(cs_validate(pp, unknown, kd, ds, 3, cp, ct, 3, V) == kPhValid, "an unknown slot overlaps nothing");
  CHECK(cs_validate(pp, ordered_overlap, kd, ds, 3, cp, ct, 3, V) == kPhValid, "the ordered form and the phrase take overlapping slots");
  CHECK(cs_validate(pp_off, ok, kd, ds, 3, cp, ct, 3, V) == kPhPtr, "item_ptr");
  CHECK(cs_validate(pp, ok, kd_bad, ds, 3, cp, ct, 3, V) == kNearKind, "a kind outside 0 .. 2");
  CHECK(cs_validate(pp_nine, ok, kd, ds, 3, cp, ct, 3, V) == kNearLength, "a Near of nine slots");
  CHECK(cs_validate(pp, ok, kd, ds_big, 3, cp, ct, 3, V) == kNearDist, "a distance of 256");
  CHECK(cs_validate(pp, ok, kd, ds, 3, cp_off, ct, 3, V) == kCsClsPtr && cs_validate(pp, ok, kd, ds, 3, cp_down, ct, 3, V) == kCsClsPtr, "cls_ptr");
  CHECK(cs_validate(pp, ok, kd, ds, 3, cp, ct_same, 3, V) == kCsClsOrder && cs_validate(pp, ok, kd, ds, 3, cp, ct_down, 3, V) == kCsClsOrder,
        "member ids not strictly ascending");
  CHECK(cs_validate(pp, ok, kd, ds, 3, nullptr, ct, 3, V) == kPhNull && cs_validate(pp, ok, kd, ds, 3, cp, nullptr, 3, V) == kPhNull, "null class arrays");
  CHECK(cs_validate(pp, ok, kd, ds, 3, cp, ct, -1, V) == kPhSizes && cs_validate(pp, ok, kd, ds, -1, cp, ct, 3, V) == kPhSizes, "negative counts");
  CHECK(cs_validate(pp, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, V) == kPhValid, "no item and no class read nothing");
  for (int e : {(int)kCsClsPtr, (int)kCsClsOrder, (int)kCsOverlap, (int)kNearDist, (int)kPhPtr})
    CHECK(std::string(cs_error_text(e)) != "ok", "an error without words");
  // an unknown slot reads nothing: the index's arrays are null
  const CsIndex none{PhIndex{nullptr, nullptr, 5, 9, nullptr, nullptr}, nullptr, nullptr, nullptr, nullptr, 2, 3};
  for (int s : {-1, 5, 7, 10, 1 << 30}) CHECK(!cs_slot(none, s).known, "slot id %d is unknown", s);
  CsSlot two[2] = {cs_slot(none, -1), cs_slot(none, 6)};
  cs_link_slots(two, 2);
  CHECK(cs_driver(two, 2).at < 0 && cs_driver(two, 2).len == 0, "an unknown slot empties the item");
  long long cells = 0;
  CHECK(cs_cells(1, 0, &cells) && cells == 1 && cs_cells(65, 257, &cells) && cells == 130, "cells");
  CHECK(cs_cells(kCsMaxCells, 256, &cells) && !cs_cells(kCsMaxCells + 1, 256, &cells) && !cs_cells(1LL << 23, 257, &cells), "cells x 256 < 2^32");
  CHECK(cs_run_len(0, 1000, kSpanNearOrdered, 2, 255) == kNearStage && cs_run_len(0, 1000, kSpanPhrase, 16, 0) == 79 &&
        cs_run_len(10, 12, kSpanPhrase, 16, 0) == 2, "run lengths");
  if (failures == 0) std::printf("validate ok\n");
}

}  // namespace

int main() {
  const long sizes[] = {40, 300, 900};
  const long counts[] = {1, 2, 65};
  for (long n : sizes)
    for (long k : counts) family(n, k, 3000 + (uint64_t)n * 7 + (uint64_t)k);
  written_out();
  validation();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("class span rule ok\n");
  return 0;
}

// Host check of the rules of amdr_unit_spans (unit_span_rule.hpp, over class_span_rule.hpp's slots, driver and masks; the
// host scans of compact.hpp), a program of its own:
//   check_unit_span
// It resolves generated unit items — sentence and paragraph, ordered and not, whose slots are plain tokens and token
// classes — tile by tile and round by round as the kernels of unit_span.hip do: the slots resolved and linked, the driver,
// the shape, the conjunction per candidate, per surviving document one round of kPhLanes tokens after the other, each from
// exactly len masks and len break bytes turned into the ballots us_round takes, with the carry between the rounds; the
// counts, the scan, the write behind the lists that stand before — and compares the lists with a naive scan of every unit
// of every document that decides the unordered form by a bipartite matching.  Every array has exactly the size the header
// promises, so with the host sanitizers (tests/test_unit_span_rule_host.py) an access outside one is a failure.  Then the
// written-out cases at the lane and round edges, and every refusal of us_validate.
// Build: c++ -std=c++17 check_unit_span.cpp (plain host code; no HIP header is needed).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#define AMDR_COMPACT_HOST_ONLY 1  // the host forms alone: this program has no device code
#include "compact.hpp"
#include "union_rule.hpp"
#include "unit_span_rule.hpp"

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

// The classes of every corpus.  0, 1, 2, 5 and the plain tokens 11, 12, 13 are pairwise DISJOINT: the slots of the
// unordered items (a slot id may repeat).  3, 4, 6, 7 and 8 overlap or equal others: for the ordered items only.  8 holds
// an id outside the vocabulary.
const std::vector<std::vector<int>> kClasses = {{0, 1}, {2, 3, 4}, {5}, {0, 1}, {1, 2}, {}, {6, 7, 8, 9, 10}, {13}, {6, 1000}};

struct Corpus {
  long n_docs;
  std::vector<std::vector<int>> docs;    // the naive scan's own form
  std::vector<std::vector<int>> breaks;  // per document, per token
  std::vector<long long> term_ptr, doc_ptr, cls_ptr, x_ptr;
  std::vector<int> post_doc, tokens, cls_terms, x_doc;  // x_doc: the lists before the items', at exactly their size
  std::vector<unsigned char> brk;                       // the resident flags, at exactly n_tokens
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
    std::vector<int> seq, brk;
    // the break density of the document: none, every token, or one in `every` (the first byte is whatever comes: forced)
    const long every = d % 7 == 3 ? 0 : d % 7 == 5 ? 1 : 2 + r.below(40);
    for (long i = 0; i < len; ++i) {
      seq.push_back((int)(std::upper_bound(cum.begin(), cum.end(), r.below(total)) - cum.begin()));
      const bool s = every && r.below(every) == 0;
      brk.push_back(s ? (r.below(4) == 0 ? 3 : 1) : 0);
    }
    c.docs.push_back(seq), c.breaks.push_back(brk);
  }
  std::vector<long long> tp(kTerms + 1, 0), dp(n_docs + 1, 0), cp{0}, xp{0};
  std::vector<int> pd, tk, ct, xd;
  std::vector<unsigned char> bk;
  for (long t = 0; t < kTerms; ++t) {
    for (long d = 0; d < n_docs; ++d)
      if (std::find(c.docs[d].begin(), c.docs[d].end(), (int)t) != c.docs[d].end()) pd.push_back((int)d);
    tp[t + 1] = (long long)pd.size();
  }
  for (long d = 0; d < n_docs; ++d) {
    tk.insert(tk.end(), c.docs[d].begin(), c.docs[d].end()), dp[d + 1] = (long long)tk.size();
    bk.insert(bk.end(), c.breaks[d].begin(), c.breaks[d].end());
  }
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
  c.term_ptr = exact(tp), c.doc_ptr = exact(dp), c.post_doc = exact(pd), c.tokens = exact(tk), c.brk = exact(bk);
  c.cls_ptr = exact(cp), c.cls_terms = exact(ct), c.x_ptr = exact(xp), c.x_doc = exact(xd);
  return c;
}

struct Item {
  int kind;
  std::vector<int> slots;
};

// the unordered form as the matching it is: augmenting paths over the positions of one unit
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

bool naive_unit(const std::vector<int>& seq, long b, long e, const Item& it) {
  const long M = (long)it.slots.size();
  if (it.kind & kUsOrdered) {
    long j = 0;
    for (long q = b; q < e && j < M; ++q)
      if (slot_fills(it.slots[(size_t)j], seq[(size_t)q])) ++j;
    return j == M;
  }
  std::vector<std::vector<int>> may((size_t)M);
  for (long j = 0; j < M; ++j)
    for (long q = b; q < e; ++q)
      if (slot_fills(it.slots[(size_t)j], seq[(size_t)q])) may[(size_t)j].push_back((int)(q - b));
  std::vector<int> taken((size_t)(e - b), -1);
  for (long j = 0; j < M; ++j) {
    std::vector<char> seen((size_t)(e - b), 0);
    if (!place((int)j, may, taken, seen)) return false;
  }
  return true;
}

bool naive_holds(const std::vector<int>& seq, const std::vector<int>& brk, const Item& it) {
  const int bit = (it.kind & kUsParagraph) ? 2 : 1;
  long b = 0;
  for (long e = 1; e <= (long)seq.size(); ++e) {
    if (e < (long)seq.size() && !(brk[(size_t)e] & bit)) continue;
    if (naive_unit(seq, b, e, it)) return true;
    b = e;
  }
  return false;
}

std::vector<int> naive_list(const Corpus& c, const Item& it) {
  std::vector<int> out;
  if (!us_sized(it.kind, (long long)it.slots.size())) return out;
  for (int s : it.slots)
    if (!slot_known(s)) return out;
  for (long d = 0; d < c.n_docs; ++d)
    if (naive_holds(c.docs[(size_t)d], c.breaks[(size_t)d], it)) out.push_back((int)d);
  return out;
}

struct Lists {
  std::vector<long long> ptr;  // the whole array's: n_before + n + 1 entries
  std::vector<int> docs, status;
};

long long rounds_walked = 0;

// one round as the wave forms it: len tokens and len break bytes -> the ballots -> us_round
bool walk_round(const int* tokens, const unsigned char* brk, int len, bool first, const CsSlot* slots, int L, const int* cls_terms,
                const UsShape& shape, int kind, UsCarry& carry) {
  const std::vector<int> tk(tokens, tokens + len);  // at exactly their size
  const std::vector<unsigned char> bk(brk, brk + len);
  unsigned long long starts = first ? 1ull : 0ull, B[kUsMaxSlots] = {};
  for (int lane = 0; lane < len; ++lane) {
    const unsigned m = cs_token_mask(tk[(size_t)lane], slots, L, cls_terms);
    if (bk[(size_t)lane] & us_break_bit(kind)) starts |= 1ull << lane;
    for (int j = 0; j < L; ++j)
      if ((m >> j) & 1u) B[j] |= 1ull << lane;
  }
  ++rounds_walked;
  return us_round(shape, B, starts, len, carry);
}

// one surviving document, as one wave walks it
bool walk_document(const CsIndex& I, const unsigned char* brk, const CsSlot* slots, int L, const UsShape& shape, int kind, long long doc) {
  const long long beg = I.ph.doc_ptr[doc], end = I.ph.doc_ptr[doc + 1];
  UsCarry carry = us_carry_clear();
  for (long long base = beg; base < end; base += kPhLanes) {
    const int len = end - base < kPhLanes ? (int)(end - base) : kPhLanes;
    if (walk_round(I.ph.tokens + base, brk + base, len, base == beg, slots, L, I.cls_terms, shape, kind, carry)) return true;
  }
  return false;
}

// the block's item: the slots resolved, linked and given a driver; 0: an item the rule does not define
int block_item(const CsIndex& I, const std::vector<long long>& pp, const std::vector<int>& all, int kind, long p, CsSlot* slots,
               CsDriver* D) {
  const long long L = pp[(size_t)p + 1] - pp[(size_t)p];
  const bool sized = us_sized(kind, L);
  for (long long j = 0; sized && j < L; ++j) slots[j] = cs_slot(I, all[(size_t)(pp[(size_t)p] + j)]);
  if (sized) cs_link_slots(slots, (int)L);
  *D = sized ? cs_driver(slots, (int)L) : CsDriver{-1, nullptr, 0, 0};
  return sized ? (int)L : 0;
}

// the three launches of unit_span.hip on the CPU, on arrays of the sizes amdr_unit_spans_plan / the caller promise; the docs
// array holds rows_cap ints and begins with the lists that stand before
Lists run_items(const Corpus& c, const std::vector<Item>& items, long long cand_max, long long rows_cap) {
  const long n = (long)items.size(), n_before = c.n_before();
  std::vector<long long> pp((size_t)n + 1, 0);
  std::vector<int> pt, kd;
  for (long p = 0; p < n; ++p) {
    pt.insert(pt.end(), items[(size_t)p].slots.begin(), items[(size_t)p].slots.end()), pp[(size_t)p + 1] = (long long)pt.size();
    kd.push_back(items[(size_t)p].kind);
  }
  const std::vector<int> slots_all = exact(pt), kind = exact(kd);
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
    CsSlot slots[kUsMaxSlots];
    CsDriver D;
    const int L = block_item(I, pp, slots_all, kind[(size_t)p], (long)p, slots, &D);
    const UsShape shape = us_shape(slots, L, kind[(size_t)p]);
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
        keep = walk_document(I, c.brk.data(), slots, L, shape, kind[(size_t)p], D.docs[D.begin + i]);
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
    CsSlot slots[kUsMaxSlots];
    CsDriver D;
    (void)block_item(I, pp, slots_all, kind[(size_t)p], (long)p, slots, &D);
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

// Items of the four kinds over plain tokens and classes: the slots drawn from the tokens of one unit of a document (a hit
// there), from a run that may cross a break, or at random; 2 .. 8 slots; every eleventh with an unknown slot id.  The slots
// of an unordered item come from the disjoint family alone (an id may repeat).
std::vector<Item> make_items(const Corpus& c, long count, uint64_t seed) {
  Rng r{seed};
  std::vector<Item> out;
  const int C = (int)(kTerms + kClsFirst);
  const std::vector<int> family = {C + 0, C + 1, C + 2, C + 5, 11, 12, 13};
  const std::vector<int> any = {C + 0, C + 1, C + 2, C + 3, C + 4, C + 5, C + 6, C + 7, C + 8, 0, 1, 2, 3, 6, 9};
  while ((long)out.size() < count) {
    const long k = (long)out.size();
    Item it;
    it.kind = (int)(k % 4);
    const std::vector<int>& pool = (it.kind & kUsOrdered) ? any : family;
    const long M = k % 7 == 6 ? kUsMaxSlots : 2 + r.below(3);
    if (k % 3 == 2) {
      for (long j = 0; j < M; ++j) it.slots.push_back(pool[(size_t)r.below((long)pool.size())]);
    } else {
      const std::vector<int>& seq = c.docs[(size_t)r.below(c.n_docs)];
      if ((long)seq.size() < M) continue;
      const long s = k % 2 ? (long)seq.size() - M : r.below((long)seq.size() - M + 1);  // every other one at the end
      const long step = 1 + r.below(3);  // (a sparse run: the members need not be neighbours)
      for (long j = 0; j < M; ++j) {
        const long at = std::min<long>((long)seq.size() - 1, s + j * step);
        const int x = seq[(size_t)at];
        std::vector<int> fit;  // the pool's slots the token fills
        for (int cand : pool)
          if (slot_fills(cand, x)) fit.push_back(cand);
        it.slots.push_back(fit.empty() ? pool[0] : fit[(size_t)r.below((long)fit.size())]);
      }
      if (!(it.kind & kUsOrdered)) std::reverse(it.slots.begin(), it.slots.end());
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
  CsSlot slots[kUsMaxSlots];
  CsDriver D;
  (void)block_item(I, pp, it.slots, it.kind, 0, slots, &D);
  return D.len;
}

void family(long n_docs, long n_items, uint64_t seed) {
  const std::string name = "unit spans n=" + std::to_string(n_docs) + " count=" + std::to_string(n_items);
  const Corpus c = make_corpus(n_docs, seed);
  const std::vector<Item> items = make_items(c, n_items, seed + 1);
  std::vector<std::vector<int>> want;
  long long cand_max = 0, total = 0, ub_sum = 0, classy = 0;
  rounds_walked = 0;
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
    if (!same) CHECK(false, "%s: item %ld (kind %d, %zu slots) differs from the naive scan", name.c_str(), p, items[(size_t)p].kind,
                     items[(size_t)p].slots.size());
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
  std::printf("%s: %lld documents in the lists, %lld items with a class, longest driver %lld, %lld rounds walked\n", name.c_str(),
              total, classy, cand_max, rounds_walked);
  if (failures == 0) std::printf("family ok\n");
}

// hand-made sequences, one document each, through cs_token_mask and us_round; slots given as id sets: class c = sets[c], slot
// id 1000 + ids[c] over a vocabulary of 1000 plain tokens (equal ids: one group)
bool hit_anywhere(const std::vector<std::vector<int>>& sets, const std::vector<int>& ids, const std::vector<int>& seq,
                  const std::vector<int>& brk, int kind) {
  std::vector<long long> cp{0};
  std::vector<int> ct;
  for (const auto& s : sets) ct.insert(ct.end(), s.begin(), s.end()), cp.push_back((long long)ct.size());
  const std::vector<long long> cpe = exact(cp), xp((size_t)sets.size() + 1, 0);
  const std::vector<int> cte = exact(ct), tk = exact(seq);
  std::vector<unsigned char> bk;
  for (int b : brk) bk.push_back((unsigned char)b);
  const CsIndex I{PhIndex{nullptr, nullptr, 1000, 1, nullptr, nullptr}, xp.data(), nullptr, cpe.data(), cte.data(), (long)sets.size(), 0};
  CsSlot slots[kUsMaxSlots];
  const int L = (int)ids.size();
  for (int j = 0; j < L; ++j) slots[j] = cs_slot(I, 1000 + ids[(size_t)j]);
  cs_link_slots(slots, L);
  const UsShape shape = us_shape(slots, L, kind);
  UsCarry carry = us_carry_clear();
  const long long end = (long long)seq.size();
  for (long long base = 0; base < end; base += kPhLanes) {
    const int len = end - base < kPhLanes ? (int)(end - base) : kPhLanes;
    if (walk_round(tk.data() + base, bk.data() + base, len, base == 0, slots, L, cte.data(), shape, kind, carry)) return true;
  }
  return false;
}

void written_out() {
  const int a = 0, b = 1, y = 3;
  const std::vector<std::vector<int>> ab = {{a}, {b}}, aa = {{a, 7}};
  long n = 0;
  auto doc = [&](long len, std::vector<long> at_a, std::vector<long> at_b, std::vector<long> breaks, int flag) {
    std::vector<int> seq((size_t)len, y), brk((size_t)len, 0);
    for (long p : at_a) seq[(size_t)p] = a;
    for (long p : at_b) seq[(size_t)p] = b;
    for (long p : breaks) brk[(size_t)p] = flag;
    return std::make_pair(seq, brk);
  };
  auto expect = [&](const std::vector<std::vector<int>>& sets, const std::vector<int>& ids, const std::pair<std::vector<int>, std::vector<int>>& d,
                    int kind, bool want) {
    CHECK(hit_anywhere(sets, ids, d.first, d.second, kind) == want, "written-out case %ld", n);
    ++n;
  };
  // a unit that begins at lane 0, 63 and 64; members on both sides of a round boundary; a unit over three rounds
  for (long start : {0L, 1L, 63L, 64L, 65L, 127L, 128L}) {
    expect(ab, {0, 1}, doc(200, {start}, {start + 1}, {start}, 1), 0, true);
    expect(ab, {0, 1}, doc(200, {start}, {start + 1}, {start + 1}, 1), 0, false);      // the break lies between them
    expect(ab, {0, 1}, doc(200, {start}, {start + 1}, {start + 1}, 1), 2, true);       // ... a sentence break: one paragraph
    expect(ab, {0, 1}, doc(200, {start}, {start + 1}, {start + 1}, 3), 2, false);      // ... a paragraph break
    expect(ab, {0, 1}, doc(200, {start}, {start + 70}, {}, 0), 0, true);               // across a round boundary
    expect(ab, {0, 1}, doc(200, {start}, {start + 70}, {start + 64}, 1), 0, false);
    expect(ab, {1, 0}, doc(200, {start}, {start + 70}, {}, 0), 1, false);              // the order given: b before a
    expect(ab, {0, 1}, doc(200, {start}, {start + 70}, {}, 0), 1, true);
  }
  expect(ab, {0, 1}, doc(200, {2}, {190}, {1}, 1), 0, true);        // one unit over three rounds and more
  expect(ab, {0, 1}, doc(200, {2}, {190}, {1, 130}, 1), 0, false);
  expect(ab, {0, 1}, doc(1, {0}, {}, {}, 0), 0, false);             // a document of one token
  // 64 units in one round: every token begins one
  {
    auto d = doc(64, {10}, {11}, {}, 0);
    for (auto& f : d.second) f = 1;
    expect(ab, {0, 1}, d, 0, false);
    expect(ab, {0, 1}, d, 2, true);  // (sentence starts are no paragraph starts)
    d.second[11] = 0;
    expect(ab, {0, 1}, d, 0, true);
  }
  // the same slot twice needs two tokens in one unit; one token never fills both
  expect(aa, {0, 0}, doc(130, {5, 100}, {}, {}, 0), 0, true);
  expect(aa, {0, 0}, doc(130, {5, 100}, {}, {64}, 1), 0, false);
  expect(aa, {0, 0}, doc(130, {5}, {}, {}, 0), 0, false);
  expect(aa, {0, 0}, doc(130, {5}, {}, {}, 0), 1, false);
  expect(aa, {0, 0}, doc(130, {63, 64}, {}, {}, 0), 1, true);
  // the first byte of a document is forced: a unit of the previous document never reaches in
  expect(ab, {0, 1}, doc(3, {0}, {1}, {}, 0), 0, true);
  // the carry saturates: nine tokens of a group of eight slots
  {
    std::vector<long> at;
    for (long i = 0; i < 9; ++i) at.push_back(60 + i);
    expect(aa, {0, 0, 0, 0, 0, 0, 0, 0}, doc(100, at, {}, {}, 0), 0, true);
    at.resize(7);
    expect(aa, {0, 0, 0, 0, 0, 0, 0, 0}, doc(100, at, {}, {}, 0), 0, false);
  }
  if (failures == 0) std::printf("written-out ok\n");
}

void validation() {
  const int64_t V = 10;
  const int64_t pp[] = {0, 2, 5, 7}, pp_off[] = {1, 2, 5, 7}, pp_nine[] = {0, 9, 12, 14}, pp_one[] = {0, 1, 5, 7};
  const int32_t kd[] = {0, 1, 2}, kd_bad[] = {0, 4, 2}, kd_neg[] = {-1, 1, 2};
  const int64_t cp[] = {0, 2, 3, 5, 7}, cp_off[] = {1, 2, 3, 5, 7}, cp_down[] = {0, 3, 2, 5, 7};
  const int32_t ct[] = {1, 4, 1, 2, 3, 2, 3}, ct_same[] = {1, 1, 1, 2, 3, 2, 3};
  // classes: 0 = {1, 4}, 1 = {1}, 2 = {2, 3}, 3 = {2, 3}.  Items 0 and 2 are unordered.
  const int32_t ok[] = {10, 12, 0, 1, 2, 3, 4}, equal_ids[] = {10, 10, 0, 1, 2, 3, 4}, two_ids[] = {12, 13, 0, 1, 2, 3, 4};
  const int32_t overlap[] = {10, 11, 0, 1, 2, 3, 4}, plain_in[] = {10, 4, 0, 1, 2, 3, 4}, unknown[] = {10, 99, 0, 1, 2, 3, 4};
  const int32_t ordered_overlap[] = {2, 3, 10, 11, 1, 5, 6};
  CHECK(us_validate(pp, ok, kd, 3, cp, ct, 4, V) == kPhValid, "valid items");
  CHECK(us_validate(pp, equal_ids, kd, 3, cp, ct, 4, V) == kPhValid, "equal slots by id");
  CHECK(us_validate(pp, two_ids, kd, 3, cp, ct, 4, V) == kUsTwoIds, "equal sets under two ids in an unordered item");
  CHECK(us_validate(pp, overlap, kd, 3, cp, ct, 4, V) == kCsOverlap && us_validate(pp, plain_in, kd, 3, cp, ct, 4, V) == kCsOverlap,
        "overlapping unequal slots in an unordered item");
  CHECK(us_validate(pp, unknown, kd, 3, cp, ct, 4, V) == kPhValid, "an unknown slot overlaps nothing");
  CHECK(us_validate(pp, ordered_overlap, kd, 3, cp, ct, 4, V) == kPhValid, "the ordered form takes overlapping slots");
  CHECK(us_validate(pp_off, ok, kd, 3, cp, ct, 4, V) == kPhPtr, "item_ptr");
  CHECK(us_validate(pp, ok, kd_bad, 3, cp, ct, 4, V) == kUsKind && us_validate(pp, ok, kd_neg, 3, cp, ct, 4, V) == kUsKind, "a kind outside 0 .. 3");
  CHECK(us_validate(pp_nine, ok, kd, 3, cp, ct, 4, V) == kUsLength && us_validate(pp_one, ok, kd, 3, cp, ct, 4, V) == kUsLength,
        "an item of nine slots, of one");
  CHECK(us_validate(pp, ok, kd, 3, cp_off, ct, 4, V) == kCsClsPtr && us_validate(pp, ok, kd, 3, cp_down, ct, 4, V) == kCsClsPtr, "cls_ptr");
  CHECK(us_validate(pp, ok, kd, 3, cp, ct_same, 4, V) == kCsClsOrder, "member ids not strictly ascending");
  CHECK(us_validate(pp, ok, kd, 3, nullptr, ct, 4, V) == kPhNull && us_validate(pp, ok, kd, 3, cp, nullptr, 4, V) == kPhNull, "null class arrays");
  CHECK(us_validate(pp, ok, nullptr, 3, cp, ct, 4, V) == kPhNull && us_validate(nullptr, ok, kd, 3, cp, ct, 4, V) == kPhNull, "null item arrays");
  CHECK(us_validate(pp, ok, kd, 3, cp, ct, -1, V) == kPhSizes && us_validate(pp, ok, kd, -1, cp, ct, 4, V) == kPhSizes, "negative counts");
  CHECK(us_validate(pp, nullptr, nullptr, 0, nullptr, nullptr, 0, V) == kPhValid, "no item and no class read nothing");
  for (int e : {(int)kUsLength, (int)kUsKind, (int)kUsTwoIds, (int)kCsOverlap}) CHECK(std::string(us_error_text(e)) != "ok", "an error without words");
  CHECK(us_break_valid(0) && us_break_valid(1) && us_break_valid(3) && !us_break_valid(2) && !us_break_valid(4) && !us_break_valid(255),
        "the break bytes");
  CHECK(us_sized(0, 2) && us_sized(3, 8) && !us_sized(4, 2) && !us_sized(-1, 2) && !us_sized(0, 1) && !us_sized(0, 9), "sizes");
  CHECK(us_low_bits(0) == 0 && us_low_bits(1) == 1 && us_low_bits(63) == ~0ull >> 1 && us_low_bits(64) == ~0ull, "low bits");
  // an undefined item holds nowhere, whatever the ballots say
  const unsigned long long ones[kUsMaxSlots] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
  for (int kind = 0; kind < 4; ++kind) {
    UsCarry c0 = us_carry_clear();
    CHECK(!us_round(us_shape(nullptr, 0, kind), ones, 1ull, 64, c0), "an item without slots");
  }
  if (failures == 0) std::printf("validate ok\n");
}

}  // namespace

int main() {
  const long sizes[] = {40, 300, 900};
  const long counts[] = {1, 2, 65};
  for (long n : sizes)
    for (long k : counts) family(n, k, 5000 + (uint64_t)n * 7 + (uint64_t)k);
  written_out();
  validation();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("unit span rule ok\n");
  return 0;
}

// Host check of the rules of amdr_union_lists (union_rule.hpp; the host scan of compact.hpp), a program of its own:
//   check_union_lists
// It resolves generated union items cell by cell and word by word as the kernels of union_lists.hip do — per (item, tile
// of kUnTile documents) a bitmap of exactly kUnWords words, per term the tile's part of the posting list by
// un_tile_range, per posting the word and the bit, the bit counts, the scan, and per thread of the write pass the
// expansion of its kUnPer words behind the array's start — and compares the lists with a naive set union.  Every array
// has exactly the size the header promises (allocated at that size), so with the host sanitizers
// (tests/test_union_rule_host.py) an access outside one is a failure.  Then the written-out cases (among them the clamp
// at a capacity one below the total, and an array continued behind earlier lists) and every refusal of un_validate.
// Build: c++ -std=c++17 check_union_lists.cpp (plain host code; no HIP header is needed).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#define AMDR_COMPACT_HOST_ONLY 1  // the host forms alone: this program has no device code
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

struct Corpus {
  long n_docs, n_terms;
  std::vector<std::vector<int>> lists;  // the naive union's own form
  std::vector<long long> term_ptr;
  std::vector<int> post_doc;
  UnIndex index() const { return UnIndex{term_ptr.data(), post_doc.data(), n_terms, n_docs}; }
};

Corpus from_lists(long n_docs, const std::vector<std::vector<int>>& lists) {
  Corpus c;
  c.n_docs = n_docs, c.n_terms = (long)lists.size(), c.lists = lists;
  std::vector<long long> tp(1, 0);
  std::vector<int> pd;
  for (const auto& l : lists) {
    pd.insert(pd.end(), l.begin(), l.end());
    tp.push_back((long long)pd.size());
  }
  c.term_ptr = exact(tp), c.post_doc = exact(pd);
  return c;
}

// n_terms posting lists over n_docs documents: term 0 holds every document, term t >= 1 every document with probability
// 1 / (t + 1); term 1 is forced to hold the documents around every tile boundary (a list that straddles it), the last
// document is in term 2, and the last term is in no document.
Corpus make_corpus(long n_docs, long n_terms, uint64_t seed) {
  Rng r{seed};
  std::vector<std::vector<int>> lists(n_terms);
  for (long d = 0; d < n_docs; ++d) {
    lists[0].push_back((int)d);
    for (long t = 1; t + 1 < n_terms; ++t) {
      const bool edge = (t == 1 && (d % kUnTile == 0 || d % kUnTile == kUnTile - 1)) || (t == 2 && d == n_docs - 1);
      if (edge || r.below(t + 1) == 0) lists[t].push_back((int)d);
    }
  }
  return from_lists(n_docs, lists);
}

typedef std::vector<int> Item;

std::vector<int> naive_union(const Corpus& c, const Item& it) {
  std::set<int> s;
  for (int t : it)
    if (t >= 0 && t < c.n_terms) s.insert(c.lists[t].begin(), c.lists[t].end());
  return std::vector<int>(s.begin(), s.end());
}

struct Result {
  std::vector<long long> list_ptr;  // [n_before + n_items + 1]
  std::vector<int> docs;            // [rows_cap]
  std::vector<int> status;          // [n_items]
};

// The three launches of un_launch on the host: count, scan, write.  list_ptr / docs arrive with the first n_before + 1
// entries and the documents before list_ptr[n_before] written; rows_cap == docs.size().
void run(const Corpus& c, const std::vector<Item>& items, long n_before, Result* out) {
  const UnIndex I = c.index();
  const long n_items = (long)items.size();
  const long long rows_cap = (long long)out->docs.size();
  std::vector<long long> ip(1, 0);
  std::vector<int> it_terms;
  for (const Item& it : items) {
    it_terms.insert(it_terms.end(), it.begin(), it.end());
    ip.push_back((long long)it_terms.size());
  }
  const std::vector<long long> item_ptr = exact(ip);
  const std::vector<int> item_terms = exact(it_terms);
  CHECK(un_validate((const int64_t*)item_ptr.data(), item_terms.data(), n_items) == kUnValid, "generated items are valid");
  long long cells = 0;
  CHECK(un_cells(n_items, c.n_docs, &cells), "the cells fit a launch");
  const long long tiles = un_tiles(c.n_docs);
  CHECK(cells == n_items * tiles, "cells");
  std::vector<long long> counts((size_t)cells), offsets((size_t)cells + 1);
  std::vector<std::vector<unsigned>> parked;  // one bitmap of exactly kUnWords words per cell
  // count
  for (long long cell = 0; cell < cells; ++cell) {
    const long long p = cell / tiles, tile = cell - p * tiles;
    std::vector<unsigned> bits((size_t)kUnWords, 0u);
    for (long long j = item_ptr[p]; j < item_ptr[p + 1]; ++j) {
      long long lo, hi;
      if (!un_tile_range(I, item_terms[j], tile, &lo, &hi)) continue;
      CHECK(lo <= hi, "an ordered range");
      for (long long i = lo; i < hi; ++i) {
        const long long doc = I.post_doc[i];
        const int w = un_bit_word(doc, tile);
        CHECK(w >= 0 && w < kUnWords, "document %lld outside tile %lld", doc, tile);
        if (w >= 0 && w < kUnWords) bits[w] |= un_bit_mask(doc);
      }
    }
    long long n = 0;
    for (unsigned w : bits) n += un_popcount(w);
    counts[cell] = n;
    parked.push_back(exact(bits));
  }
  // scan
  compact_scan_host(counts.data(), (long)cells, offsets.data());
  // write
  const long long start = n_before > 0 ? out->list_ptr[n_before] : 0;
  for (long long cell = 0; cell < cells; ++cell) {
    const long long p = cell / tiles, tile = cell - p * tiles;
    if (tile == 0) {
      const long long begin = start + offsets[p * tiles], end = start + offsets[(p + 1) * tiles];
      if (n_before == 0 && p == 0) out->list_ptr[0] = 0;
      out->list_ptr[n_before + p + 1] = un_clamp(end, rows_cap);
      out->status[p] = un_status(begin, end, rows_cap);
    }
    long long rank = 0;  // the block scan: the bits of the threads before
    for (int t = 0; t < kUnThreads; ++t) {
      long long at = start + offsets[cell] + rank;
      for (int j = 0; j < kUnPer; ++j) {
        const int w = t * kUnPer + j;
        const int n = un_expand_word(parked[cell][w], tile, w, at, rows_cap, out->docs.data());
        CHECK(n == un_popcount(parked[cell][w]), "expansion and count agree");
        at += n, rank += n;
      }
    }
    CHECK(rank == counts[cell], "the write pass meets the count of cell %lld", cell);
  }
}

// items against the naive union, at a capacity that holds them exactly
void compare(const Corpus& c, const std::vector<Item>& items, const char* what) {
  std::vector<std::vector<int>> want;
  long long total = 0;
  for (const Item& it : items) {
    want.push_back(naive_union(c, it));
    total += (long long)want.back().size();
  }
  Result r;
  r.list_ptr.assign(items.size() + 1, -7), r.docs.assign((size_t)total, -7), r.status.assign(items.size(), -7);
  r.list_ptr = exact(r.list_ptr), r.docs = exact(r.docs), r.status = exact(r.status);
  run(c, items, 0, &r);
  CHECK(r.list_ptr[0] == 0 && r.list_ptr[items.size()] == total, "%s: list_ptr ends at %lld, want %lld", what,
        r.list_ptr[items.size()], total);
  for (size_t p = 0; p < items.size(); ++p) {
    const std::vector<int> got(r.docs.begin() + r.list_ptr[p], r.docs.begin() + r.list_ptr[p + 1]);
    CHECK(got == want[p], "%s: item %zu differs from the naive union (%zu against %zu documents)", what, p, got.size(),
          want[p].size());
    CHECK(r.status[p] == kTsOk, "%s: item %zu status %d", what, p, r.status[p]);
  }
}

std::vector<Item> make_items(const Corpus& c, long count, uint64_t seed) {
  Rng r{seed};
  std::vector<Item> items;
  const long V = c.n_terms;
  for (long k = 0; k < count; ++k) {
    Item it;
    switch (k % 8) {
      case 0: it = {(int)(1 + r.below(V - 1))}; break;                          // one term: its posting list
      case 1: it = {2, 2}; break;                                               // a repeated id
      case 2: it = {}; break;                                                   // M = 0
      case 3: it = {-1, (int)V, (int)V + 5}; break;                             // unknown ids alone
      case 4: it = {-1, 3, (int)V, 5}; break;                                   // ... and mixed with known ones
      case 5: it = {0, 4}; break;                                               // nested: term 0 holds every document
      case 6: for (int j = 0; j < 300; ++j) it.push_back((int)(1 + r.below(V - 1))); break;  // more terms than threads
      default: for (long j = 0, m = 2 + r.below(5); j < m; ++j) it.push_back((int)(1 + r.below(V - 1)));
    }
    items.push_back(it);
  }
  return items;
}

void written_out() {
  // five documents; term 0 = {0, 2}, term 1 = {2, 4}, term 2 = {}
  const Corpus c = from_lists(5, {{0, 2}, {2, 4}, {}});
  const std::vector<Item> items = {{0, 1}, {}, {-1, 3}, {0, 0}, {1}};
  compare(c, items, "written-out");
  CHECK(naive_union(c, items[0]) == (std::vector<int>{0, 2, 4}), "the shared document stands once");
  // a capacity one below the total (3 + 0 + 0 + 2 + 2 = 7): the last item is cut, its status 2, the pointers clamped
  Result r;
  r.list_ptr = exact(std::vector<long long>(6, -7)), r.docs = exact(std::vector<int>(6, -7)), r.status = exact(std::vector<int>(5, -7));
  run(c, items, 0, &r);
  CHECK((r.list_ptr == std::vector<long long>{0, 3, 3, 3, 5, 6}), "clamped pointers");
  CHECK((r.status == std::vector<int>{0, 0, 0, 0, 2}), "status 2 from the first item that does not fit");
  CHECK((r.docs == std::vector<int>{0, 2, 4, 0, 2, 2}), "the earlier items are exact");
  // ... and far below: an empty item behind the overflow keeps status 0
  Result s;
  s.list_ptr = exact(std::vector<long long>(6, -7)), s.docs = exact(std::vector<int>(2, -7)), s.status = exact(std::vector<int>(5, -7));
  run(c, items, 0, &s);
  CHECK((s.list_ptr == std::vector<long long>{0, 2, 2, 2, 2, 2}), "clamped pointers at capacity 2");
  CHECK((s.status == std::vector<int>{2, 0, 0, 2, 2}), "status at capacity 2");
  CHECK((s.docs == std::vector<int>{0, 2}), "documents at capacity 2");
  // an array continued behind two earlier lists of 1 and 2 documents
  Result k;
  k.list_ptr = exact(std::vector<long long>{0, 1, 3, -7, -7}), k.docs = exact(std::vector<int>{9, 8, 7, -7, -7, -7, -7, -7});
  k.status = exact(std::vector<int>(2, -7));
  run(c, {{0, 1}, {1}}, 2, &k);
  CHECK((k.list_ptr == std::vector<long long>{0, 1, 3, 6, 8}), "continued pointers");
  CHECK((k.docs == std::vector<int>{9, 8, 7, 0, 2, 4, 2, 4}), "the earlier lists are untouched, the unions behind them");
  CHECK((k.status == std::vector<int>{0, 0}), "continued status");
  // a list that straddles a tile boundary, and the last bit of a tile's last word
  const Corpus t = from_lists(kUnTile + 1, {{kUnTile - 1, kUnTile}, {0, kUnTile - 1}});
  compare(t, {{0}, {1}, {0, 1}}, "straddle");
  long long lo, hi;
  CHECK(un_tile_range(t.index(), 0, 0, &lo, &hi) && lo == 0 && hi == 1, "tile 0 holds the first posting");
  CHECK(un_tile_range(t.index(), 0, 1, &lo, &hi) && lo == 1 && hi == 2, "tile 1 holds the second");
  CHECK(!un_tile_range(t.index(), -1, 0, &lo, &hi) && !un_tile_range(t.index(), 2, 0, &lo, &hi), "unknown terms read nothing");
  CHECK(un_bit_word(kUnTile - 1, 0) == kUnWords - 1 && un_bit_mask(kUnTile - 1) == 0x80000000u, "the last bit of a tile");
  CHECK(un_bit_word(kUnTile, 1) == 0 && un_bit_mask(kUnTile) == 1u, "the first bit of the next");
  CHECK(un_tiles(0) == 1 && un_tiles(1) == 1 && un_tiles(kUnTile) == 1 && un_tiles(kUnTile + 1) == 2, "tiles");
  long long cells;
  CHECK(un_cells(kUnMaxCells, 1, &cells) && cells == kUnMaxCells, "the most cells");
  CHECK(!un_cells(kUnMaxCells + 1, 1, &cells) && !un_cells(1LL << 31, 1, &cells) && !un_cells(1LL << 20, 10000000, &cells),
        "too many cells");
  CHECK(!un_cells(-1, 1, &cells) && !un_cells(1, -1, &cells), "negative sizes");
  std::printf("written-out ok\n");
}

void validation() {
  const std::vector<int64_t> good = {0, 2, 2, 3};
  const std::vector<int32_t> terms = {1, -1, 7};
  CHECK(un_validate(good.data(), terms.data(), 3) == kUnValid, "valid");
  CHECK(un_validate(good.data(), terms.data(), 0) == kUnValid, "no item");
  CHECK(un_validate(good.data(), terms.data(), -1) == kUnSizes, "negative count");
  CHECK(un_validate(nullptr, terms.data(), 3) == kUnNull, "null item_ptr");
  CHECK(un_validate(good.data(), nullptr, 3) == kUnNull, "null item_terms");
  const std::vector<int64_t> empty = {0, 0};
  CHECK(un_validate(empty.data(), nullptr, 1) == kUnValid, "an empty item reads no term");
  const std::vector<int64_t> from1 = {1, 2}, back = {0, 2, 1};
  CHECK(un_validate(from1.data(), terms.data(), 1) == kUnPtr, "item_ptr from 1");
  CHECK(un_validate(back.data(), terms.data(), 2) == kUnPtr, "item_ptr not monotone");
  for (int e : {kUnNull, kUnSizes, kUnPtr}) CHECK(un_error_text(e)[0] != 'o', "error text %d", e);
  std::printf("validate ok\n");
}

}  // namespace

int main() {
  const long sizes[] = {33, kUnTile - 1, kUnTile + 1, 3 * kUnTile + 1};
  const long item_counts[] = {1, 2, 65};
  for (long n : sizes) {
    const Corpus c = make_corpus(n, 12, 0x9e3779b97f4a7c15ull ^ (uint64_t)n);
    for (long k : item_counts) {
      const int before = failures;
      std::printf("unions n=%ld count=%ld:", n, k);
      compare(c, make_items(c, k, 77 + (uint64_t)k), "family");
      if (k == 65) {  // every kind of item stands at least once; and one alone at the head of a call
        for (long kind = 0; kind < 8; ++kind) compare(c, {make_items(c, 8, 5)[kind]}, "family-single");
      }
      std::printf(" %s\n", failures == before ? "family ok" : "family FAILED");
    }
  }
  written_out();
  validation();
  if (failures) {
    std::printf("%d FAILURES\n", failures);
    return 1;
  }
  std::printf("union rule ok\n");
  return 0;
}

// What the host check programs of the BM25 updates share (check_bm25_add.cpp, check_bm25_remove.cpp): the random
// generator, the generated term-major index, CHECK, and the walk over an index tile by tile as the update kernels make it
// (bm25_update.hip, bm_tile_window).  Each program is one translation unit of plain host code.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bm25_tile_rule.hpp"

namespace amdr {

inline uint64_t rng_state = 0x9e3779b97f4a7c15ull;
inline uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

struct Csr {
  std::vector<long long> ptr;
  std::vector<int32_t> doc, tf;
};

// n_terms lists over n_docs documents: term 0 holds every document, list lengths fall off, every `hole`-th term is
// empty; `empty_run` terms without postings follow term 1; further full lists pad the index to exactly pad_to postings
inline Csr make_csr(long n_terms, long n_docs, long hole, long empty_run, long long pad_to) {
  Csr c;
  c.ptr.assign(1, 0);
  for (long t = 0; t < n_terms; ++t) {
    long df = t == 0 ? n_docs : (long)(n_docs / (t + 1)) + (long)(rnd() % 2);
    if (df > n_docs) df = n_docs;
    if (hole && t % hole == hole - 1) df = 0;
    // df documents in ascending order: a random start and stride 1
    const long first = df < n_docs ? (long)(rnd() % (uint32_t)(n_docs - df + 1)) : 0;
    for (long j = 0; j < df; ++j) {
      c.doc.push_back((int32_t)(first + j));
      c.tf.push_back((int32_t)(1 + rnd() % 9));
    }
    c.ptr.push_back((long long)c.doc.size());
    if (t == 1)
      for (long e = 0; e < empty_run; ++e) c.ptr.push_back((long long)c.doc.size());
  }
  while ((long long)c.doc.size() < pad_to) {
    const long long rest = pad_to - (long long)c.doc.size();
    const long df = rest < n_docs ? (long)rest : n_docs;
    for (long j = 0; j < df; ++j) {
      c.doc.push_back((int32_t)j);
      c.tf.push_back(1);
    }
    c.ptr.push_back((long long)c.doc.size());
  }
  return c;
}

inline int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      ++failures;                        \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");                 \
    }                                    \
  } while (0)

// A tile's view of the term table, as bm_tile_window leaves it to the kernel's threads.
struct HostTileWindow {
  const long long* tab;
  long base, t0, t1;
  long term_of(long long p) const { return bm_tile_term_of(tab, base, t0, t1, p); }
  long long start_of(long t) const { return tab[t - base]; }
};

// The postings 0 .. ptr[n_terms] - 1 tile by tile: the tile's terms by bm_tile_terms, a window of the term table copied
// out EXACTLY as the kernel's LDS copy (entries t0 .. t1 + 1 in a vector of that size, so a sanitizer sees a read beyond
// it) or, when it does not fit, the table itself; then on_posting(p, window) for every posting of the tile.  Checks that
// every posting is put in the term whose list holds it is the caller's, through window.term_of.  Returns the number of
// windows searched in the table itself.
template <class F>
long host_tile_walk(const std::vector<long long>& ptr, long n_terms, F on_posting) {
  const long long nnz = ptr[(size_t)n_terms];
  long windows_global = 0;
  for (long long p0 = 0; p0 < nnz; p0 += kBmTile) {
    const long long p1 = std::min<long long>(p0 + kBmTile, nnz);
    long t0, t1;
    bm_tile_terms(ptr.data(), n_terms, p0, p1, &t0, &t1);
    const bool fits = bm_tile_window_fits(t0, t1);
    std::vector<long long> win;  // exactly the entries the kernel copies to LDS
    if (fits) win.assign(ptr.begin() + t0, ptr.begin() + t1 + 2);
    CHECK(!fits || win.size() <= (size_t)kBmTile + 2, "window of %zu entries", win.size());
    windows_global += fits ? 0 : 1;
    const HostTileWindow w{fits ? win.data() : ptr.data(), fits ? t0 : 0, t0, t1};
    for (long long p = p0; p < p1; ++p) on_posting(p, w);
  }
  return windows_global;
}

}  // namespace amdr

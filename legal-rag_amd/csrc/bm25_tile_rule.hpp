// What the rules of amdr_bm25_add and amdr_bm25_remove share (bm25_add_rule.hpp, bm25_remove_rule.hpp; the kernels are in
// bm25_update.hip): the tile of postings a block owns, the search for a posting's term in a term table or a window of
// one, and the checks of the corpus statistics both calls take.  Plain C++ in the style of tokenize_rule.hpp: no HIP
// header is needed, AMDR_HD is empty for a plain host compiler.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define AMDR_HD __host__ __device__
#else
#define AMDR_HD
#endif

namespace amdr {

constexpr int kBmTileThreads = 256;
constexpr int kBmTilePerThread = 8;
constexpr int kBmTile = kBmTileThreads * kBmTilePerThread;  // consecutive postings per block of the update kernels

// The term of posting p: the largest t in [lo, hi] with ptr[t] <= p, where ptr[lo] <= p < ptr[hi + 1] (terms without
// postings are stepped over: the largest such t is the one whose list holds p).  `ptr` may be a window of the table:
// ptr[i] is the entry of term base + i.
AMDR_HD inline long bm_tile_term_of(const long long* ptr, long base, long lo, long hi, long long p) {
  while (lo < hi) {
    const long mid = lo + ((hi - lo + 1) >> 1);
    if (ptr[mid - base] <= p)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// The terms of a tile's first and last posting, [p0, p1) not empty and inside [0, ptr[n_terms]); and whether the table
// entries t0 .. t1 + 1 fit the kernels' LDS window (always, unless terms without postings widen the range).
AMDR_HD inline void bm_tile_terms(const long long* ptr, long n_terms, long long p0, long long p1, long* t0, long* t1) {
  *t0 = bm_tile_term_of(ptr, 0, 0, n_terms - 1, p0);
  *t1 = bm_tile_term_of(ptr, 0, *t0, n_terms - 1, p1 - 1);
}
AMDR_HD inline bool bm_tile_window_fits(long t0, long t1) { return t1 - t0 + 2 <= (long)(kBmTile + 2); }

// The statistics of the corpus after the update: the factors divide by avgdl, and rank_bm25 never produces a non-finite
// idf (the rankings use -inf as "no document" and order NaN by convention).
inline bool bm_avgdl_ok(double avgdl) { return std::isfinite(avgdl) && avgdl > 0.0; }
inline bool bm_idf_all_finite(const double* idf, int64_t n_terms) {
  for (int64_t t = 0; t < n_terms; ++t)
    if (!std::isfinite(idf[t])) return false;
  return true;
}

}  // namespace amdr

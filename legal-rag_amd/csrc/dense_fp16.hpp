// What the exactness of the dense channel's two fp16 first passes rests on — the large scan (dense_hi.hip) and the long
// batch on a short corpus (dense_small_hi.hip + dense_tail.hip dense_hi_select_fuse_kernel) — stated once: the power-of-two
// scale of a vector (pow2_exp / pow2_scale of tile_swizzle.hpp, which MaxSim shares), the rounding bound, the scale range
// it holds in, the statistics of the chunk matrix that feed it.
#pragma once
#include "tile_swizzle.hpp"

#include <cfloat>
#include <cmath>
#include <cstring>

namespace amdr {

// The bound.  Both passes compute x^ . q^: fp16 roundings of x' = x 2^-ex and q' = q 2^-eq, exact products, fp32 sums.
// Per component the fp16 rounding is |dx'| <= 2^-11 |x'| + 2^-25 (the second term covers fp16's subnormal range), the
// same for q'.  Hence
//   |x^ . q^ - x' . q'| <= (2^-10 + 2^-22) |x'| |q'| + 2^-25 (|q'|_1 + |x'|_1) (1 + 2^-11) <= ... + d 2^-24 (1 + 2^-11)
// (the products of two fp16 values are exact in the MFMA's fp32, the accumulation of d of them adds d 2^-24 |x'| |q'|;
// so does the accumulation inside the exact kernel the pass is compared with).  |x'| <= R' = R 2^-ex with R the largest
// row norm.  The result is in the scaled units of x' . q': times 2^(ex + eq) in the units of the exact score.
__host__ __device__ inline float dense_fp16_eps_scaled(int d, float q_norm_scaled, float r_scaled) {
  const float rel = 1.125f * (9.765625e-4f + 2.4e-7f + 2.f * (float)(d + 8) * 5.9604645e-8f);
  return rel * q_norm_scaled * r_scaled + 1.125f * (float)d * 5.9604645e-8f;
}

// The scale range.  The comparison only holds while the exact fp32 scores neither overflow nor sink into fp32's subnormal
// range; a query outside its form's range has no bound.  Both conditions sit on top of |ex| < 100 (DenseFp16Stats::finite).
// The large scan bounds the exponent of the product, the short corpus the query's alone, so there |ex + eq| can reach 199:
// which condition it should have is open.
__host__ __device__ inline bool dense_fp16_range_large_scan(int ex, int eq) { return ex + eq <= 100 && ex + eq >= -100; }
__host__ __device__ inline bool dense_fp16_range_short_corpus(int eq) { return eq <= 100 && eq >= -100; }

// The statistics of a chunk matrix: computed by dense_stats_kernel (dense_hi.hip) into the dense handle's 8-word buffer —
// word 0 the largest |component|, word 1 the largest row L2 norm (bit patterns of non-negative floats; NaN components and
// the norms of rows that hold one are dropped), words 2..4 the large scan's counters, kDenseStatNan != 0 if a NaN was seen —
// owned by amdr_dense, kept current by create / add, copied into amdr_dense_small.
constexpr int kDenseStatNan = 5, kDenseStatWords = 8;
struct DenseFp16Stats {
  float x_scale = 1.f;       // power of two: |x| * x_scale < 1 for every component
  float row_norm_max = 0.f;  // largest row L2 norm
  bool finite = false;       // both maxima finite and |ex| < 100
  bool has_nan = false;
  // What each form requires.  The large scan keeps per-tile MAXIMA, and fmaxf drops a NaN row's scores from them as it
  // drops the row from the statistics; the short corpus hands rows of approximate SCORES on, which would carry the NaN.
  bool large_scan_ok() const { return finite; }
  bool short_corpus_ok() const { return finite && !has_nan; }
};
inline DenseFp16Stats dense_fp16_stats(const unsigned int* words) {
  float amax, rmax;
  memcpy(&amax, words, 4);
  memcpy(&rmax, words + 1, 4);
  const int e = pow2_exp(amax);
  return {pow2_scale(e), rmax, amax <= FLT_MAX && rmax <= FLT_MAX && e > -100 && e < 100, words[kDenseStatNan] != 0u};
}

}  // namespace amdr

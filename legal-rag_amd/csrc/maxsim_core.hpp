// Device code of the split-fp16 pair form of the ColBERT channel (see maxsim.hip for the design notes): one wave scores
// one (query, document) pair straight from the [hi | lo] token image.  Shared by maxsim.hip's kernels and the scoped
// search of scope.hip: the same instruction sequence, hence the same bits.
#pragma once
#include "common.hpp"
#include "tile_swizzle.hpp"
#include "topk.hpp"

#include <cfloat>
#include <cmath>

namespace amdr {

constexpr int kMsWaves = 4;
constexpr int kDim = AMDR_MAXSIM_DIM;  // 128

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float ms_dpp_add(float v) {
  int t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false);
  return v + __int_as_float(t);
}
__device__ __forceinline__ float ms_wave_sum(float v) {  // total in lane 63
  v = ms_dpp_add<0x111, 0xf>(v);
  v = ms_dpp_add<0x112, 0xf>(v);
  v = ms_dpp_add<0x114, 0xf>(v);
  v = ms_dpp_add<0x118, 0xf>(v);
  v = ms_dpp_add<0x142, 0xa>(v);
  v = ms_dpp_add<0x143, 0xc>(v);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// ---- split-fp16 form ("f16x3") -------------------------------------------------------------------------------
// The same tile on the fp16 matrix instructions (v_mfma_f32_32x32x16_f16: 16x the rate of the fp32-input form).
// fp16 alone (11 significant bits) would miss the 1e-4 bar, so every operand x (scaled by a power of two into
// [-1, 1], see below) is split EXACTLY into
//     x = hi + lo / 2048,   hi = fp16(x),   lo = fp16((x - hi) * 2048)
// (x - hi is exact in fp32; lo keeps its next 11 bits: 22 significant bits in all), and a product is taken as
//     a*b ~= a_hi*b_hi + (a_hi*b_lo + a_lo*b_hi) / 2048
// — three fp16 MFMAs instead of the fp32-input sequence, every fp16 x fp16 product exact in the fp32 accumulator;
// only the a_lo*b_lo term (2^-22 of the product) is dropped.  The cross terms run in their own accumulator and are
// folded in with one fma per score.  Measured on the UCC-en / Civil-Code-zh token stores against the fp64 oracle:
// max |score error| 2.0e-6 / 2.5e-6 on scores of ~20 (the fp32-input form: 3.7e-6 / 2.8e-6 — its 128-term fp32
// chains round more often), ranks identical (tests/test_kernels_gpu.py).  Document tokens are split ONCE at index
// creation into a [hi 128 x fp16 | lo 128 x fp16] image of the same 512 bytes per token as the fp32 row (same LDS
// tile, same swizzle); a query is split by its wave at kernel start.  Power-of-two scales (the store's: from its
// largest |component| at creation; a query's: from its own) keep hi / lo inside fp16's range for any finite input
// and are undone exactly on the per-token maxima.  AMDR_MAXSIM_F16X3=0 pins the fp32-input form.
//
// Shape: one 32x32x16 accumulator (16 registers) has the query token on the lane (l & 31) and 16 document tokens in
// the lane's registers: rows mfma32_row(reg, l >> 5) (tile_swizzle.hpp).
//   A (32 doc tokens x 16):   lane (r = l & 31, h = l >> 5) holds row r, k = 16 s + 8 h .. + 7 = 16-B chunk 2 s + h
//   B (16 x 32 query tokens): the same of query-token row r.
// An MFMA holds its SIMD's vector issue for 8 cycles whatever its shape (MI355X_MICROARCH.md): 8 of 16 for a
// 16x16x32, 8 of 32 for a 32x32x16 — the first version of this form ran 48 16x16x32 MFMAs per tile and was bound by
// the issue port (PMC: ~100 vector + 50 scalar instructions per wave and tile beside them, matrix pipe 51 % busy;
// staggering the two waves of a SIMD by half a step gained 10 %); 24 of the wide shape leave 3x the issue slots:
// 2.40 -> 2.23 ms per 1 168 UCC-en queries (fp32-input form: 6.78 ms).  What bounds it now is POWER: under this kernel
// the chip holds 1.70 GHz (GRBM_GUI_ACTIVE; 2.11 GHz under the fp32-input dense kernel), the matrix pipe is busy 67 %
// of those cycles (77 % with DMA and barriers taken out in a timing-only build, which runs 2.10 ms); at the held
// clock the MFMAs alone need 1.63 ms.
constexpr float kMsLoScale = 2048.f, kMsLoInv = 1.f / 2048.f;

__device__ __forceinline__ void ms_split(const float (&x)[8], float s, h8& hi, h8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = x[j] * s;
    const _Float16 h = (_Float16)v;
    hi[j] = h;
    lo[j] = (_Float16)((v - (float)h) * kMsLoScale);
  }
}

// A query's fragments, split (lane (r, h): token row r, chunks 2 s + h); rows past q_len are zero; the wave's
// power-of-two scale comes back in `unscale` (1 / scale, exact).
__device__ __forceinline__ void ms_load_query_h(const float* __restrict__ Qq, int q_len, bool live, int r, int h,
                                                h8 (&qh)[8], h8 (&ql)[8], float& unscale) {
  float x[8][8];
  float m = 0.f;
  const bool out = !live || r >= q_len;
  const float* p = Qq + (size_t)(r < q_len ? r : q_len - 1) * kDim + 8 * h;
#pragma unroll
  for (int st = 0; st < 8; ++st) {
    f32x4 v0 = f32x4{0.f, 0.f, 0.f, 0.f}, v1 = v0;
    if (live) {
      v0 = *reinterpret_cast<const f32x4*>(p + 16 * st);
      v1 = *reinterpret_cast<const f32x4*>(p + 16 * st + 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[st][j] = out ? 0.f : v0[j];
      x[st][4 + j] = out ? 0.f : v1[j];
      m = fmaxf(m, fmaxf(fabsf(x[st][j]), fabsf(x[st][4 + j])));
    }
  }
#pragma unroll
  for (int sft = 1; sft < 64; sft <<= 1) m = fmaxf(m, __shfl_xor(m, sft));
  const int e = pow2_exp(m);  // m = f * 2^e, f in [0.5, 1)
  const float sc = pow2_scale(e);
  unscale = pow2_scale(-e);
#pragma unroll
  for (int st = 0; st < 8; ++st) ms_split(x[st], sc, qh[st], ql[st]);
}

// One 32 x 32 tile: 24 MFMAs, then the lane's maximum over its 16 document tokens (rows >= remain are no tokens of
// the document: masked on the last tile of a document only — a real, wave-uniform branch: if-converted, the 32
// compare / select pairs ran on every tile).  Both kernels of this form call it: identical bits.
__device__ __forceinline__ void ms_tile_h(const h8 (&ah)[8], const h8 (&al)[8], const h8 (&qh)[8],
                                          const h8 (&ql)[8], int h, int remain, float& best) {
  f32x16 am, ac;
#pragma unroll
  for (int j = 0; j < 16; ++j) am[j] = ac[j] = 0.f;
#pragma unroll
  for (int st = 0; st < 8; ++st) {
    am = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[st], qh[st], am, 0, 0, 0);
    ac = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[st], ql[st], ac, 0, 0, 0);
    ac = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[st], qh[st], ac, 0, 0, 0);
  }
  float v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = __builtin_fmaf(ac[j], kMsLoInv, am[j]);
  if (remain < 32) {
    asm volatile("" ::: "memory");
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (mfma32_row(j, h) >= remain) v[j] = -FLT_MAX;
  }
#pragma unroll
  for (int j = 0; j < 16; j += 2) best = fmaxf(best, fmaxf(v[j], v[j + 1]));
}

// Document score from the per-lane maxima: max over the two row halves, sum over the q_len query tokens (lanes
// 0..31 of h = 0), scales undone (powers of two: exact).
__device__ __forceinline__ float ms_finish_h(float best, int r, int h, int q_len, float unscale) {
  const float b = fmaxf(best, __uint_as_float(lane_xor<32>(__float_as_uint(best))));
  return ms_wave_sum((h == 0 && r < q_len) ? b * unscale : 0.f);
}

// One (query, document) pair by one wave: the document's tokens [t_lo, t_lo + len) tile by tile, fragments straight from
// the [hi | lo] image (rows past the end of the document read on into the next document's tokens — the image is padded
// by one tile — and are masked by ms_tile_h).  unscale: the query's power of two times the store's.  The score comes
// back in every lane.  The body of maxsim_scores_h_kernel; scope.hip runs it over a query's scope documents.
__device__ __forceinline__ float ms_pair_doc_h(const unsigned char* img, long t_lo, int len,
                                               const h8 (&qh)[8], const h8 (&ql)[8], int r32, int h, int q_len,
                                               float unscale) {
  float best = -FLT_MAX;
  for (int tok0 = 0; tok0 < len; tok0 += 32) {
    const unsigned char* p = img + (size_t)(t_lo + tok0 + r32) * 512 + h * 16;
    h8 ah[8], al[8];
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      ah[st] = *reinterpret_cast<const h8*>(p + 32 * st);
      al[st] = *reinterpret_cast<const h8*>(p + 256 + 32 * st);
    }
    ms_tile_h(ah, al, qh, ql, h, len - tok0, best);
  }
  return ms_finish_h(best, r32, h, q_len, unscale);
}

}  // namespace amdr

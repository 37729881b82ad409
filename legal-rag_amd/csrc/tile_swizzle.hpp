// The address arithmetic that the matrix kernels share, stated once: the register vector types, the two XOR swizzles of
// an LDS tile, the source offsets of an LDS-DMA piece (the ring that uses them: lds_ring.hpp), the row map of a 32x32x16
// accumulator, the power-of-two scale rule.  No builtins: a host program can include it (check_tile_swizzle.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

namespace amdr {

typedef float f32x4 __attribute__((ext_vector_type(4)));  // native vectors: they stay in registers (HIP's float4 did not)
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

// ---- rows of 256 or 512 bytes (fp16 tiles: MaxSim's [hi | lo] and hi-only images, the short-corpus dense image) ----
// Row j at byte j * ROWB, its logical 16-B slot s at physical slot s ^ (j & 15) (its own inverse).  A ds_read_b128 lane
// group holds 16 distinct rows at two logical slots that differ in bit 0: the XOR maps those two sets onto disjoint bank
// quads (conflict-free).  Bit 4 of the slot is left alone: in a 512-byte row the lo part stays 256 B behind the hi part.
__host__ __device__ __forceinline__ int tile_slot(int row, int slot) { return slot ^ (row & 15); }
template <int ROWB>
__host__ __device__ __forceinline__ int tile_off(int row, int slot) {
  static_assert(ROWB == 256 || ROWB == 512, "rows of 16 or 32 slots");
  return row * ROWB + (tile_slot(row, slot) << 4);
}

// ---- rows of 128 bytes (a 32-float or 64-half K chunk: dense_mfma.hip, dense_panel.hip, dense_hi.hip and its image) ----
// Row r at byte r * 128 — two rows share one 256-B bank row — its logical 16-B slot s (0..7) at physical slot
// s ^ ((r >> 1) & 7) (its own inverse).  A ds_read_b128 lane group covers 16 different rows at the same logical slot: 8
// physical slots x the 2 halves of the bank row = conflict-free; a ds_write_b128 lane group (8 lanes) writes one row.
__host__ __device__ __forceinline__ int stage_slot(int row, int slot) { return slot ^ ((row >> 1) & 7); }
__host__ __device__ __forceinline__ int stage_off(int row, int slot) { return row * 128 + (stage_slot(row, slot) << 4); }

// ---- LDS-DMA pieces of a tile_off<ROWB> tile ----
// A piece = one DMA request of a wave (64 lanes x 16 B = 1 KiB) = 1024 / ROWB whole rows; it lands lane-linear (piece base
// + lane * 16): lane l fills row l / (ROWB / 16), PHYSICAL slot l % (ROWB / 16), which holds the logical slot that the same
// XOR names.  The lane's SOURCE offset inside an unswizzled tile, for one piece and for pieces piece0 .. + PIECES - 1:
template <int ROWB>
__host__ __device__ __forceinline__ long piece_off(int piece, int lane) {
  constexpr int kSlots = ROWB / 16, kRows = 1024 / ROWB;
  const int prow = kRows * piece + lane / kSlots;
  return (long)prow * ROWB + (tile_slot(prow, lane & (kSlots - 1)) << 4);  // tile_off<ROWB> in 64 bits
}
template <int PIECES, int ROWB>
__host__ __device__ __forceinline__ void piece_offs(int piece0, int lane, long (&poff)[PIECES]) {
#pragma unroll
  for (int u = 0; u < PIECES; ++u) poff[u] = piece_off<ROWB>(piece0 + u, lane);
}

// ---- v_mfma_f32_32x32x16_f16: the accumulator has the B row on the lane (l & 31); register j of lane half h = l >> 5 is A row
__host__ __device__ constexpr int mfma32_row(int j, int h) { return (j & 3) + 8 * (j >> 2) + 4 * h; }

// ---- the power-of-two scale of a vector ----
// e with amax = f 2^e, f in [0.5, 1), for a vector's largest |component| amax (0 when amax is 0, infinite or NaN), and
// the scale 2^-e that brings every |component| below 1 (pow2_scale(-e) undoes it exactly)
__host__ __device__ inline int pow2_exp(float amax) {
  int e = 0;
  if (amax > 0.f && amax <= FLT_MAX) (void)frexpf(amax, &e);
  return e;
}
__host__ __device__ inline float pow2_scale(int e) { return ldexpf(1.f, -e); }

}  // namespace amdr

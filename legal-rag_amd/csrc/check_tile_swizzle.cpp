// Host check of tile_swizzle.hpp, a program of its own (never part of the library):
//   check_tile_swizzle        the LDS-DMA ring simulated on the host for every (pieces per wave, row bytes, waves) in use:
//                             the pieces cover the tile exactly once and tile_off<ROWB>(row, slot) of the stage holds source
//                             unit (row, slot); stage_off is a bijection with the same property; mfma32_row is a permutation
//                             of the 32 rows; pow2_exp scales every finite positive maximum into [0.5, 1)
// Build: hipcc -x hip --offload-host-only check_tile_swizzle.cpp (host code only; tests/test_tile_swizzle_host.py adds the
// host sanitizers)
#include "tile_swizzle.hpp"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

using namespace amdr;

// WAVES waves issue PIECES pieces each of a tile of rows of ROWB bytes (wave w: pieces PIECES w ..): a piece lands
// lane-linear at stage + piece * 1024 + lane * 16, from source + poff.  Units are 16 bytes; a source unit's value is its index.
template <int PIECES, int ROWB, int WAVES>
static int check_ring() {
  constexpr int kBytes = PIECES * WAVES * 1024, kUnits = kBytes / 16, kSlots = ROWB / 16, kRows = kBytes / ROWB;
  static_assert(kBytes == 16384 || kBytes == 8192, "the stages in use are 16 KiB and 8 KiB");
  std::vector<int> stage(kUnits, -1), taken(kUnits, 0);
  for (int wave = 0; wave < WAVES; ++wave)
    for (int lane = 0; lane < 64; ++lane) {
      long poff[PIECES];
      piece_offs<PIECES, ROWB>(PIECES * wave, lane, poff);
      for (int u = 0; u < PIECES; ++u) {
        const int piece = PIECES * wave + u;
        if (poff[u] != piece_off<ROWB>(piece, lane)) return 1;
        if (poff[u] < 0 || poff[u] >= kBytes || poff[u] % 16 || taken[poff[u] / 16]++) {
          fprintf(stderr, "pieces=%d rowb=%d waves=%d: offset %ld of piece %d lane %d is outside, unaligned or taken\n", PIECES,
                  ROWB, WAVES, poff[u], piece, lane);
          return 1;
        }
        stage[(piece * 1024 + lane * 16) / 16] = (int)(poff[u] / 16);
      }
    }
  for (int i = 0; i < kUnits; ++i)
    if (taken[i] != 1) return 1;
  for (int row = 0; row < kRows; ++row)
    for (int slot = 0; slot < kSlots; ++slot) {
      const int off = tile_off<ROWB>(row, slot);
      if (off < 0 || off >= kBytes || off % 16 || stage[off / 16] != row * kSlots + slot) {
        fprintf(stderr, "pieces=%d rowb=%d waves=%d: tile_off(%d, %d) = %d does not hold the unit\n", PIECES, ROWB, WAVES, row,
                slot, off);
        return 1;
      }
    }
  return 0;
}

// the 128-byte-row stage: 32 rows x 8 slots onto 4 KiB, every row inside its own 128 bytes, stage_slot its own inverse
static int check_stage() {
  std::vector<int> taken(32 * 8, 0);
  for (int row = 0; row < 32; ++row)
    for (int slot = 0; slot < 8; ++slot) {
      const int off = stage_off(row, slot), phys = stage_slot(row, slot);
      if (off != row * 128 + phys * 16 || phys < 0 || phys > 7 || stage_slot(row, phys) != slot || taken[off / 16]++) {
        fprintf(stderr, "stage_off(%d, %d) = %d\n", row, slot, off);
        return 1;
      }
    }
  for (int t : taken)
    if (t != 1) return 1;
  return 0;
}

static int check_mfma32_row() {
  int seen[32] = {0};
  for (int h = 0; h < 2; ++h)
    for (int j = 0; j < 16; ++j) {
      const int r = mfma32_row(j, h);
      if (r < 0 || r > 31 || seen[r]++) return 1;
    }
  // four consecutive registers are four consecutive rows (the 16-byte stores of dsh_scores_kernel)
  for (int h = 0; h < 2; ++h)
    for (int m = 0; m < 4; ++m)
      for (int e = 0; e < 4; ++e)
        if (mfma32_row(4 * m + e, h) != 8 * m + 4 * h + e) return 1;
  return 0;
}

static int check_pow2() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float none[] = {0.f, -0.f, inf, -inf, nan, -1.f};  // no scale: exponent 0, scale 1
  for (float m : none)
    if (pow2_exp(m) != 0 || pow2_scale(pow2_exp(m)) != 1.f) {
      fprintf(stderr, "pow2_exp(%g) = %d\n", (double)m, pow2_exp(m));
      return 1;
    }
  const float some[] = {std::numeric_limits<float>::denorm_min(), 3 * std::numeric_limits<float>::denorm_min(), FLT_MIN / 2,
                        std::nextafterf(FLT_MIN, 0.f), FLT_MIN, 0.5f, std::nextafterf(1.f, 0.f), 1.f, 3.f, 65504.f, FLT_MAX};
  for (float m : some) {
    const int e = pow2_exp(m);
    // m 2^-e, exact; the factor 2^-e itself is a float for e >= -127 only (below: the smallest subnormals, where it
    // overflows — callers bound the exponent, dense_fp16.hpp), and 2^e for e <= 127
    const float scaled = ldexpf(m, -e);
    if (!(scaled >= 0.5f && scaled < 1.f) || (e >= -127 && pow2_scale(e) * m != scaled) ||
        (e >= -127 && e <= 127 && pow2_scale(e) * pow2_scale(-e) != 1.f)) {
      fprintf(stderr, "pow2_exp(%g) = %d: scaled maximum %g\n", (double)m, e, (double)scaled);
      return 1;
    }
  }
  return 0;
}

int main() {
  // (pieces per wave, row bytes, waves): the one-pass and re-scoring rings of maxsim.hip, its hi-only ring, its
  // wave-private stage, the ring of dense_small_hi.hip
  if (check_ring<2, 512, 8>() || check_ring<4, 256, 4>() || check_ring<16, 512, 1>() || check_ring<2, 256, 4>()) {
    fprintf(stderr, "the ring does not put the tile where tile_off reads it\n");
    return 1;
  }
  if (check_stage()) {
    fprintf(stderr, "stage_off is no bijection\n");
    return 1;
  }
  if (check_mfma32_row()) {
    fprintf(stderr, "mfma32_row is no permutation of the 32 rows\n");
    return 1;
  }
  if (check_pow2()) {
    fprintf(stderr, "pow2_exp does not scale into [0.5, 1)\n");
    return 1;
  }
  printf("tile swizzle ok\n");
  return 0;
}

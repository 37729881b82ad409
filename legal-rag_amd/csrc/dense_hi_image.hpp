// The resident fp16 image of the large scan's first pass: what its builder (dense_hi_image.hip), the scan
// over it (dense_hi.hip dense_hi_image_tilemax_kernel) and a host check must agree on, stated once — the byte order of the
// wave-private stage (stage_off of tile_swizzle.hpp), the image's addressing, and the one conversion.
//
// The image holds, for every 32-row tile and every 64-component chunk of the chunk matrix, the 4 KiB of halves that
// dense_hi_tilemax_kernel puts into its stage: fp16(x * x_scale), in the STAGE's byte order (the XOR swizzle baked in).
// A wave instruction of the scan reads 1 KiB contiguous and stores it lane-linear; the fragment reads behind it are the
// fp32 form's.  The last tile is padded with copies of the last row, as the fp32 form's row clamp does.
#pragma once
#include "tile_swizzle.hpp"

#include <cstddef>

namespace amdr {

constexpr int kHiTileRows = 32;          // rows of a tile
constexpr int kHiKC = 64;                // components of every row per chunk
constexpr int kHiStageBytes = 32 * 128;  // 32 rows x 64 halves: the stage, and one (tile, chunk) piece of the image

// the 16-byte unit of the image that holds components [64 chunk + 8 slot, + 8) of row `row` of tile `tile` (d = 64 nch)
__host__ __device__ __forceinline__ long hi_image_unit(long tile, int chunk, int row, int slot, int nch) {
  return (tile * nch + chunk) * (kHiStageBytes / 16) + (stage_off(row, slot) >> 4);
}
__host__ __device__ inline long hi_image_tiles(long n) { return (n + kHiTileRows - 1) / kHiTileRows; }
__host__ __device__ inline size_t hi_image_bytes(long n, int d) { return (size_t)hi_image_tiles(n) * kHiTileRows * (size_t)d * 2; }

// the conversion: x_scale is a power of two, so the product is exact and the half is the rounding of x * x_scale itself
__host__ __device__ __forceinline__ _Float16 hi_half(float x, float x_scale) { return (_Float16)(x * x_scale); }

}  // namespace amdr

// Dense channel, large scans: the builder of the resident fp16 image that the first pass can read instead of the fp32
// matrix (dense_hi_image.hpp states the layout and the conversion; the scan over it is dense_hi_image_tilemax_kernel in
// dense_hi.hip).  Run by amdr_dense_image_build and by amdr_dense_add on a handle that has an image — never by a search.
#include "common.hpp"
#include "dense_hi_image.hpp"

namespace amdr {

// One thread per 16-byte unit of the image, enumerated in the order of the SOURCE (row by row, 8 components each: a
// wave reads 2 KiB of a row contiguously); the unit's place in the image permutes the 8 units of a row's 128-byte
// segment, so the stores still fill whole segments.  Rows past n repeat row n - 1 (the scan's row clamp).
__global__ __launch_bounds__(256) void dense_hi_image_kernel(const float* __restrict__ X, long tile0, long n, int d,
                                                             float x_scale, h8* __restrict__ image) {
  const int upr = d / 8, nch = d / kHiKC;  // units per row
  const long units = (hi_image_tiles(n) - tile0) * kHiTileRows * upr;
  for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long)gridDim.x * 256) {
    const long rr = u / upr;  // row, counted from the first row of tile0
    const int c8 = (int)(u - rr * upr);
    const long tile = tile0 + rr / kHiTileRows;
    const int row = (int)(rr % kHiTileRows);
    long r = tile * kHiTileRows + row;
    if (r >= n) r = n - 1;
    const float* src = X + (size_t)r * d + c8 * 8;
    const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
    h8 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      y[e] = hi_half(a[e], x_scale);
      y[4 + e] = hi_half(b[e], x_scale);
    }
    image[hi_image_unit(tile, c8 >> 3, row, c8 & 7, nch)] = y;
  }
}

int dense_hi_image_launch(const float* X, long row0, long n, int d, float x_scale, void* image, hipStream_t st) {
  if (row0 >= n) return AMDR_OK;
  if (!dense_hi_supported(d) || row0 < 0 || !X || !image) return fail(AMDR_EINVAL, "dense (fp16 image): d=%d row0=%ld", d, row0);
  const long tile0 = row0 / kHiTileRows;  // the partial last tile of the previous state is written again
  const long units = (hi_image_tiles(n) - tile0) * kHiTileRows * (d / 8);
  long blocks = (units + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(dense_hi_image_kernel, dim3((unsigned)blocks), dim3(256), 0, st, X, tile0, n, d, x_scale,
                     reinterpret_cast<h8*>(image));
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

}  // namespace amdr

// Host check of dense_hi_image.hpp, a program of its own (never part of the library):
//   check_dense_hi_image                      the addressing is a bijection from (tile, chunk, row, 16-byte slot) onto
//                                             [0, bytes / 16) for d in {128, 768, 1024}, full and ragged n
//   check_dense_hi_image IN OUT SCALE         IN: raw fp32 values; OUT: the halves hi_half(x, SCALE) as raw 16-bit words
//                                             (a test compares them with numpy's float16 rounding of x * SCALE)
// Build: hipcc -x hip --offload-host-only check_dense_hi_image.cpp (host code only; tests/test_dense_hi_image_host.py adds
// the host sanitizers)
#include "dense_hi_image.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace amdr;

static int check_bijection(long n, int d) {
  const int nch = d / kHiKC;
  const long tiles = hi_image_tiles(n), units = (long)(hi_image_bytes(n, d) / 16);
  if (units != tiles * nch * (kHiStageBytes / 16)) return 1;
  std::vector<unsigned char> seen((size_t)units, 0);
  for (long t = 0; t < tiles; ++t)
    for (int c = 0; c < nch; ++c)
      for (int r = 0; r < kHiTileRows; ++r)
        for (int s = 0; s < 8; ++s) {
          const long u = hi_image_unit(t, c, r, s, nch);
          if (u < 0 || u >= units || seen[(size_t)u]) {
            fprintf(stderr, "n=%ld d=%d: unit %ld of (%ld, %d, %d, %d) is outside or taken\n", n, d, u, t, c, r, s);
            return 1;
          }
          seen[(size_t)u] = 1;
          // a (tile, chunk) piece is 4 KiB of its own, in the stage's byte order
          if (u / (kHiStageBytes / 16) != t * nch + c || (u % (kHiStageBytes / 16)) * 16 != stage_off(r, s)) return 1;
        }
  for (long u = 0; u < units; ++u)
    if (!seen[(size_t)u]) return 1;
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) {
    const int dims[3] = {128, 768, 1024};
    const long ns[5] = {1, 32, 1000, 9017, 9024};
    for (int d : dims)
      for (long n : ns)
        if (check_bijection(n, d)) {
          fprintf(stderr, "addressing is no bijection at n=%ld d=%d\n", n, d);
          return 1;
        }
    printf("addressing ok\n");
    return 0;
  }
  if (argc != 4) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  std::vector<float> x;
  float buf[1024];
  size_t got;
  while ((got = fread(buf, sizeof(float), 1024, in)) > 0) x.insert(x.end(), buf, buf + got);
  fclose(in);
  const float scale = strtof(argv[3], nullptr);
  std::vector<unsigned short> y(x.size());
  for (size_t i = 0; i < x.size(); ++i) {
    const _Float16 hf = hi_half(x[i], scale);
    memcpy(&y[i], &hf, 2);
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  const size_t put = fwrite(y.data(), 2, y.size(), out);
  fclose(out);
  printf("converted %zu values\n", put);
  return put == y.size() ? 0 : 1;
}

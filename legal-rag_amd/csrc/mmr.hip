// Maximal-marginal-relevance selection over fused hits (amdr_mmr, amdr_mmr_device; the definition is in amdretrieval.h).
//
// One block of 256 threads per query.  The candidates are at most 64 rows of the resident chunk matrix:
//
//   1. Gram matrix.  The candidate rows are gathered through LDS in slices of 128 columns (16-byte loads; a candidate
//      without a vector, a pool position past the query's count and the columns past d are written as zeros, so nothing
//      downstream branches around them).  The next slice is fetched into registers while the current one is multiplied.
//      G = R R^T is cut into 16 x 16 tiles on the exact fp32 matrix instruction (v_mfma_f32_16x16x4_f32); only the tiles
//      on and above the diagonal that the query's count reaches are computed, dealt round-robin to the four waves (pool 30:
//      three tiles, one each; pool 64: ten tiles, at most three each).  Each tile is stored to G[i][j] AND G[j][i], and a
//      diagonal tile stores its upper half only: one value serves both orders of a pair.
//      Both operands of a tile read the slice the same way, lane l holding columns 4*(l>>4) .. +3 of its row as ONE
//      16-byte LDS read that feeds four instructions: the summation order is a permutation of the columns, the same one
//      for both operands.  Rows are 132 floats apart, which spreads the 16 rows of a tile over all 64 banks.
//   2. Greedy selection, in wave 0: lane = candidate.  Each step is two fp64 products and a subtraction per lane, a
//      butterfly arg-max over topk.hpp's ordered key (larger value, then lower position; NaN behind every number), and
//      ONE fp64 square root and division per lane: the cosine to the candidate just selected, from G in LDS.
//
// This file is compiled with -ffp-contract=off: lambda * rel - (1 - lambda) * maxsim stays two products and a subtraction.
// No atomics, no workspace: the "_device" form only enqueues.
#include "common.hpp"
#include "topk.hpp"

#include <vector>

namespace amdr {
namespace {

constexpr int kMmrPool = AMDR_MMR_MAX_POOL;
constexpr int kMmrSlice = 128;             // columns per K slice
constexpr int kMmrLdX = kMmrSlice + 4;     // floats between two rows of the slice (16-byte aligned, 4 banks apart)
constexpr int kMmrLdG = kMmrPool + 1;
static_assert(kMmrPool == 64, "lane = candidate: the pool is one wave");

__global__ __launch_bounds__(256) void mmr_kernel(const float* __restrict__ X, long n, int d,
                                                   const long long* __restrict__ rows, int ld_rows,
                                                   const double* __restrict__ rel, long rel_stride, long rel_ld,
                                                   const int* __restrict__ count, int pool, int k_sel, double lam,
                                                   int* __restrict__ out_pos, double* __restrict__ out_mmr,
                                                   double* __restrict__ out_maxsim, int* __restrict__ out_count) {
  __shared__ __attribute__((aligned(16))) float sX[kMmrPool * kMmrLdX];
  __shared__ float sG[kMmrPool * kMmrLdG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t q = blockIdx.x;
  int m = count[q];
  m = m < 0 ? 0 : (m > pool ? pool : m);
  const int cnt = m < k_sel ? m : k_sel;
  const size_t ob = q * (size_t)k_sel;
  if (wave == 0) {
    for (int j = cnt + lane; j < k_sel; j += 64) {
      out_pos[ob + j] = -1;
      out_mmr[ob + j] = 0.0;
      out_maxsim[ob + j] = 0.0;
    }
    if (lane == 0) out_count[q] = cnt;
  }
  if (m == 0) return;  // (the whole block)

  // ---- Gram matrix -------------------------------------------------------------------------------------------------
  const int nt = (m + 15) >> 4;           // 16-row tiles the candidates reach
  const int n_tiles = nt * (nt + 1) / 2;  // on and above the diagonal, column-major: (0,0) (0,1) (1,1) (0,2) ...
  const int n_ld = nt * 2;                // rows of the slice per thread: row = (tid >> 5) + 8 * i
  const int c4 = (tid & 31) * 4;
  const float* src[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = (tid >> 5) + 8 * i;
    const long long row = r < m ? rows[q * (size_t)ld_rows + r] : -1;
    src[i] = (row >= 0 && row < n) ? X + (size_t)row * d : nullptr;
  }
  int ti[3], tj[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int idx = wave + 4 * t;
    tj[t] = idx >= 6 ? 3 : (idx >= 3 ? 2 : (idx >= 1 ? 1 : 0));
    ti[t] = idx - tj[t] * (tj[t] + 1) / 2;
  }
  f32x4 acc[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 v[8];
  auto fetch = [&](int k0) {
    const int col = k0 + c4;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i < n_ld && src[i] != nullptr && col < d) v[i] = *reinterpret_cast<const f32x4*>(src[i] + col);
    }
  };
  fetch(0);
  const int a_off = (lane & 15) * kMmrLdX + 4 * (lane >> 4);
  for (int k0 = 0; k0 < d; k0 += kMmrSlice) {
    __syncthreads();  // the reads of the slice before this one
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < n_ld) *reinterpret_cast<f32x4*>(&sX[((tid >> 5) + 8 * i) * kMmrLdX + c4]) = v[i];
    __syncthreads();
    if (k0 + kMmrSlice < d) fetch(k0 + kMmrSlice);
    const int kend = d - k0 < kMmrSlice ? d - k0 : kMmrSlice;
    for (int kk = 0; kk < kend; kk += 16) {
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        if (wave + 4 * t < n_tiles) {  // (wave-uniform: the matrix instruction runs with every lane on)
          const f32x4 a = *reinterpret_cast<const f32x4*>(&sX[ti[t] * 16 * kMmrLdX + a_off + kk]);
          const f32x4 b = *reinterpret_cast<const f32x4*>(&sX[tj[t] * 16 * kMmrLdX + a_off + kk]);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[t], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    if (wave + 4 * t < n_tiles) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {  // result r of lane l: row 4 * (l >> 4) + r, column l & 15 of the tile
        const int i = ti[t] * 16 + 4 * (lane >> 4) + r, j = tj[t] * 16 + (lane & 15);
        if (i <= j) {
          sG[i * kMmrLdG + j] = acc[t][r];
          sG[j * kMmrLdG + i] = acc[t][r];
        }
      }
    }
  }
  __syncthreads();
  if (wave != 0) return;

  // ---- greedy selection: lane = candidate --------------------------------------------------------------------------
  const bool valid = lane < m;
  const double r_i = valid ? rel[q * (size_t)rel_ld + (size_t)lane * rel_stride] : 0.0;
  const double g_ii = valid ? (double)sG[lane * kMmrLdG + lane] : 0.0;
  const double one_minus = 1.0 - lam;
  double maxsim = 0.0;
  bool taken = false;
  for (int step = 0; step < cnt; ++step) {
    const double mmr = lam * r_i - one_minus * maxsim;
    C64 c = (valid && !taken) ? C64::make(mmr, lane) : C64::pad();
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const C64 o = wave_xchg_xor(c, s);
      if (better(o, c)) c = o;
    }
    const int j = __builtin_amdgcn_readfirstlane((int)c.idv);
    if (lane == j) {
      out_pos[ob + step] = j;
      out_mmr[ob + step] = mmr;
      out_maxsim[ob + step] = maxsim;
      taken = true;
    }
    const float g_ij = valid ? sG[lane * kMmrLdG + j] : 0.f;
    const double den = sqrt(g_ii * (double)sG[j * kMmrLdG + j]);
    const bool ok = __builtin_isfinite(den) && den > 0.0 && __builtin_isfinite(g_ij);
    const double cosv = ok ? (double)g_ij / den : 0.0;
    maxsim = (step == 0 || cosv > maxsim) ? cosv : maxsim;
  }
}

int mmr_check(const amdr_dense_t* dense, const void* rows, int32_t ld_rows, const void* rel, int64_t rel_stride,
              int64_t rel_ld, const void* count, int32_t nq, int32_t pool, int32_t k_sel, double lambda,
              const void* out_pos, const void* out_mmr, const void* out_maxsim, const void* out_count) {
  AMDR_REQUIRE(dense != nullptr, "mmr: null handle");
  AMDR_REQUIRE(nq >= 0, "mmr: nq must be >= 0");
  AMDR_REQUIRE(pool >= 1 && pool <= AMDR_MMR_MAX_POOL, "mmr: pool must be in [1, %d]", AMDR_MMR_MAX_POOL);
  AMDR_REQUIRE(k_sel >= 1 && k_sel <= pool, "mmr: k_sel must be in [1, pool]");
  AMDR_REQUIRE(lambda >= 0.0 && lambda <= 1.0, "mmr: lambda must be in [0, 1]");  // (a NaN fails both)
  AMDR_REQUIRE(ld_rows >= pool, "mmr: ld_rows must be >= pool");
  AMDR_REQUIRE(rel_stride >= 1 && rel_ld >= 0, "mmr: bad rel strides");
  if (nq == 0) return AMDR_OK;
  AMDR_REQUIRE(rows && rel && count && out_pos && out_mmr && out_maxsim && out_count, "mmr: null buffer");
  return AMDR_OK;
}

int mmr_launch(const amdr_dense_t* dense, const int64_t* rows, int ld_rows, const double* rel, long rel_stride, long rel_ld,
               const int32_t* count, int nq, int pool, int k_sel, double lambda, int32_t* out_pos, double* out_mmr,
               double* out_maxsim, int32_t* out_count, hipStream_t st) {
  const float* X;
  long n;
  int d;
  dense_matrix(dense, &X, &n, &d);
  hipLaunchKernelGGL(mmr_kernel, dim3((unsigned)nq), dim3(256), 0, st, X, n, d, reinterpret_cast<const long long*>(rows),
                     ld_rows, rel, rel_stride, rel_ld, count, pool, k_sel, lambda, out_pos, out_mmr, out_maxsim, out_count);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace
}  // namespace amdr

using namespace amdr;

extern "C" {

int amdr_mmr_device(amdr_dense_t* dense, const int64_t* rows_dev, int32_t ld_rows, const double* rel_dev,
                    int64_t rel_stride, int64_t rel_ld, const int32_t* count_dev, int32_t nq, int32_t pool, int32_t k_sel,
                    double lambda, int32_t* out_pos, double* out_mmr, double* out_maxsim, int32_t* out_count, void* stream) {
  const int rc = mmr_check(dense, rows_dev, ld_rows, rel_dev, rel_stride, rel_ld, count_dev, nq, pool, k_sel, lambda, out_pos,
                           out_mmr, out_maxsim, out_count);
  if (rc || nq == 0) return rc;
  AMDR_HIP(hipSetDevice(dense_device_of(dense)));
  return mmr_launch(dense, rows_dev, ld_rows, rel_dev, (long)rel_stride, (long)rel_ld, count_dev, nq, pool, k_sel, lambda,
                    out_pos, out_mmr, out_maxsim, out_count, reinterpret_cast<hipStream_t>(stream));
}

int amdr_mmr(amdr_dense_t* dense, const int64_t* rows_host, int32_t ld_rows, const double* rel_host, int64_t rel_stride,
             int64_t rel_ld, const int32_t* count_host, int32_t nq, int32_t pool, int32_t k_sel, double lambda,
             int32_t* out_pos, double* out_mmr, double* out_maxsim, int32_t* out_count) {
  int rc = mmr_check(dense, rows_host, ld_rows, rel_host, rel_stride, rel_ld, count_host, nq, pool, k_sel, lambda, out_pos,
                     out_mmr, out_maxsim, out_count);
  if (rc || nq == 0) return rc;
  // the candidates of each query packed [nq][pool]: only positions below min(count, pool) are read from the caller
  const size_t np = (size_t)nq * pool, nk = (size_t)nq * k_sel;
  const size_t o_rows = 0, o_rel = o_rows + np * 8, o_cnt = o_rel + np * 8, o_in_end = up16(o_cnt + (size_t)nq * 4);
  const size_t o_mmr = o_in_end, o_ms = o_mmr + nk * 8, o_pos = o_ms + nk * 8, o_oc = o_pos + nk * 4,
               total = o_oc + (size_t)nq * 4;
  std::vector<char> in(o_in_end, 0);
  int64_t* prow = reinterpret_cast<int64_t*>(in.data() + o_rows);
  double* prel = reinterpret_cast<double*>(in.data() + o_rel);
  int32_t* pcnt = reinterpret_cast<int32_t*>(in.data() + o_cnt);
  for (size_t q = 0; q < (size_t)nq; ++q) {
    const int m = count_host[q] < 0 ? 0 : (count_host[q] > pool ? pool : count_host[q]);
    pcnt[q] = m;
    for (int i = 0; i < m; ++i) {
      prow[q * pool + i] = rows_host[q * (size_t)ld_rows + i];
      prel[q * pool + i] = rel_host[q * (size_t)rel_ld + (size_t)i * rel_stride];
    }
  }
  std::lock_guard<std::mutex> g(dense_mutex(dense));
  AMDR_HIP(hipSetDevice(dense_device_of(dense)));
  void* devp;
  hipStream_t st;
  if ((rc = dense_host_stage(dense, total, &devp, &st))) return rc;
  char* dv = static_cast<char*>(devp);
  AMDR_HIP(hipMemcpyAsync(dv, in.data(), o_in_end, hipMemcpyHostToDevice, st));
  rc = mmr_launch(dense, reinterpret_cast<const int64_t*>(dv + o_rows), pool, reinterpret_cast<const double*>(dv + o_rel), 1,
                  pool, reinterpret_cast<const int32_t*>(dv + o_cnt), nq, pool, k_sel, lambda,
                  reinterpret_cast<int32_t*>(dv + o_pos), reinterpret_cast<double*>(dv + o_mmr),
                  reinterpret_cast<double*>(dv + o_ms), reinterpret_cast<int32_t*>(dv + o_oc), st);
  if (rc) return rc;
  AMDR_HIP(hipMemcpyAsync(out_mmr, dv + o_mmr, nk * 8, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipMemcpyAsync(out_maxsim, dv + o_ms, nk * 8, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipMemcpyAsync(out_pos, dv + o_pos, nk * 4, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipMemcpyAsync(out_count, dv + o_oc, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipStreamSynchronize(st));
  return AMDR_OK;
}

}  // extern "C"

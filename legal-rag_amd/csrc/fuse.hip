// Fusion + min_final filter + rerank blend, on device, fp64, no FMA contraction.
//
// Replaces HybridRetriever._fuse (legalrag/retrieval/hybrid_retriever.py:389-551),
// _minmax (:24-30), _rrf_with_breakdown (:33-56), the min_final_score filter
// (:309-310) and the rerank blend (:338-355, rerankers.py:48-54,349).
// One wave per query; the candidate set is at most kd+kb+kc (<= 768) ids, so
// this is latency work: the point of doing it on the GPU is that a batch of
// queries never leaves HBM between the channel kernels and the final top-k.
// Every expression (here and in fuse_core.hpp, the device code shared with the
// dense tails of dense_tail.hip) is written in the reference's operand order and
// this file is compiled with -ffp-contract=off so results are bit-identical to
// the Python float arithmetic.  Exactly tied scores keep first-appearance order.
#include "fuse_core.hpp"

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace amdr {

constexpr int kFuseMax = 3 * AMDR_MAX_K;  // 768

// block = 64 threads (one wave); grid = nq
__global__ __launch_bounds__(64) void fuse_kernel(amdr_fuse_params_t P, ChanIn c0, ChanIn c1, ChanIn c2, int max_out,
                                                  long long* __restrict__ out_ids, double* __restrict__ out_vals,
                                                  int* __restrict__ out_mask, int* __restrict__ out_count) {
  // dynamic LDS sized by max_out (<= kFuseMax): 36 bytes per candidate
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
  long long* uid = reinterpret_cast<long long*>(fsm);
  double* sc = reinterpret_cast<double*>(uid + max_out);
  double* tot = sc + max_out;
  int* pos0 = reinterpret_cast<int*>(tot + max_out);
  int* pos[3] = {pos0, pos0 + max_out, pos0 + 2 * max_out};
  const int lane = threadIdx.x;
  const int qi = blockIdx.x;
  const ChanIn ch[3] = {c0, c1, c2};
  const double w[3] = {P.w_dense, P.w_bm25, P.w_colbert};

  // ---- valid prefix length, min / max of every channel ------------------
  int n[3];
  double lo[3], hi[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int cnt = 0;
    double mn = INFINITY, mx = -INFINITY;
    for (int j = lane; j < ch[c].k; j += 64) {
      if (ch[c].ids[(size_t)qi * ch[c].k + j] >= 0) {
        cnt++;
        double s = chan_score(ch[c], qi, j);
        mn = fmin(mn, s);
        mx = fmax(mx, s);
      }
    }
    n[c] = wave_allsum_i32(cnt);
    lo[c] = wave_min(mn);
    hi[c] = wave_max(mx);
  }

  // ---- union of ids in first-appearance order ----------------------------
  int U = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int U0 = U;  // entries a new id can collide with (ids are unique inside a channel)
    for (int base = 0; base < n[c]; base += 64) {
      const int j = base + lane;
      const bool v = j < n[c];
      long long my = v ? chan_uid(ch[c], qi, j) : -1;
      int f = -1;
      if (v)
        for (int u = 0; u < U0; ++u)
          if (uid[u] == my) {
            f = u;
            break;
          }
      const bool isnew = v && f < 0;
      const unsigned long long m = __ballot(isnew);
      const unsigned long long lt = (lane == 0) ? 0ull : (m & (~0ull >> (64 - lane)));
      const int idx = isnew ? U + __popcll(lt) : f;
      if (isnew) {
        uid[idx] = my;
        pos[0][idx] = -1;
        pos[1][idx] = -1;
        pos[2][idx] = -1;
      }
      lds_sync();
      if (v) pos[c][idx] = j;
      U += __popcll(m);
      lds_sync();
    }
  }

  // ---- RRF totals, their min / max ---------------------------------------
  const bool wrrf = (P.method == AMDR_FUSE_WRRF);
  double rmn = INFINITY, rmx = -INFINITY;
  for (int u = lane; u < U; u += 64) {
    double t = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int p = pos[c][u];
      if (p >= 0) {
        double wc = wrrf ? w[c] : 1.0;
        double v = wc * (1.0 / (double)(P.rrf_k + p + 1));
        t = t + v;
      }
    }
    tot[u] = t;
    rmn = fmin(rmn, t);
    rmx = fmax(rmx, t);
  }
  rmn = wave_min(rmn);
  rmx = wave_max(rmx);
  const bool rdeg = (rmx - rmn < 1e-12);

  // all values of candidate u (fuse_eval); the long-list path evaluates twice (score pass,
  // output pass) so that nothing but the score has to live across the rank computation
  FuseCtx X;
  X.rmn = rmn;
  X.rmx = rmx;
  X.rdeg = rdeg;
  X.wrrf = wrrf;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    X.w[c] = w[c];
    X.lo[c] = lo[c];
    X.hi[c] = hi[c];
  }
  auto eval = [&](int u, double (&val)[AMDR_FUSE_NVALS], int& mk) {
    const int pp[3] = {pos[0][u], pos[1][u], pos[2][u]};
    fuse_eval(P, X, tot[u], pp, [&](int c, int p) { return chan_score(ch[c], qi, p); }, val, mk);
  };

  // ---- score, stable descending rank, filter, scatter ---------------------
  int kept = 0;
  const size_t obase = (size_t)qi * max_out;
  if (U <= 64) {
    // one candidate per lane (the serving shape: <= 3 x top-k ids): evaluate once, keep the nine
    // values in registers across the rank computation
    double val[AMDR_FUSE_NVALS];
    int mk = 0;
    const int u = lane;
    if (u < U) {
      eval(u, val, mk);
      sc[u] = val[AMDR_FV_SCORE];
    }
    lds_sync();
    if (u < U) {
      const double s = val[AMDR_FV_SCORE];
      int r = 0;
      for (int v2 = 0; v2 < U; ++v2) {
        const double o = sc[v2];
        r += (o > s) || (o == s && v2 < u);
      }
      if (s >= P.min_final_score) kept++;
      out_ids[obase + r] = uid[u];
      out_mask[obase + r] = mk;
#pragma unroll
      for (int x = 0; x < AMDR_FUSE_NVALS; ++x) out_vals[(obase + r) * AMDR_FUSE_NVALS + x] = val[x];
    }
  } else {
    for (int u = lane; u < U; u += 64) {
      double val[AMDR_FUSE_NVALS];
      int mk;
      eval(u, val, mk);
      sc[u] = val[AMDR_FV_SCORE];
    }
    lds_sync();
    for (int u = lane; u < U; u += 64) {
      double val[AMDR_FUSE_NVALS];
      int mk;
      eval(u, val, mk);
      const double s = val[AMDR_FV_SCORE];
      int r = 0;
      for (int v2 = 0; v2 < U; ++v2) {
        const double o = sc[v2];
        r += (o > s) || (o == s && v2 < u);
      }
      if (s >= P.min_final_score) kept++;
      out_ids[obase + r] = uid[u];
      out_mask[obase + r] = mk;
#pragma unroll
      for (int x = 0; x < AMDR_FUSE_NVALS; ++x) out_vals[(obase + r) * AMDR_FUSE_NVALS + x] = val[x];
    }
  }
  kept = wave_allsum_i32(kept);
  for (int r = U + lane; r < max_out; r += 64) {
    out_ids[obase + r] = -1;
    out_mask[obase + r] = 0;
    for (int x = 0; x < AMDR_FUSE_NVALS; ++x) out_vals[(obase + r) * AMDR_FUSE_NVALS + x] = 0.0;
  }
  if (lane == 0) out_count[qi] = kept;
}

template <int W>
__global__ __launch_bounds__(64) void fuse_packed_kernel(amdr_fuse_params_t P, ChanIn c0, ChanIn c1, ChanIn c2, int nq,
                                                         int max_out, long long* __restrict__ out_ids,
                                                         double* __restrict__ out_vals, int* __restrict__ out_mask,
                                                         int* __restrict__ out_count) {
  FusePre none;
  none.have[0] = none.have[1] = none.have[2] = false;
  fuse_packed_body<W, false>(P, c0, c1, c2, nq, max_out, out_ids, out_vals, out_mask, out_count, none, blockIdx.x * (64 / W));
}

// fuse_kernel for long candidate lists, the packed forms when a query fits in 32 or 16 lanes
static void launch_fuse(const amdr_fuse_params_t& P, const ChanIn& c0, const ChanIn& c1, const ChanIn& c2, int nq,
                        int max_out, long long* ids, double* vals, int* mask, int* count, hipStream_t st) {
  if (max_out <= 16)
    hipLaunchKernelGGL(fuse_packed_kernel<16>, dim3((nq + 3) / 4), dim3(64), 0, st, P, c0, c1, c2, nq, max_out, ids, vals,
                       mask, count);
  else if (max_out <= 32)
    hipLaunchKernelGGL(fuse_packed_kernel<32>, dim3((nq + 1) / 2), dim3(64), 0, st, P, c0, c1, c2, nq, max_out, ids, vals,
                       mask, count);
  else
    hipLaunchKernelGGL(fuse_kernel, dim3(nq), dim3(64), (size_t)max_out * 36, st, P, c0, c1, c2, max_out, ids, vals, mask,
                       count);
}

// block = 64 threads; grid = nq.  Dynamic LDS: staging for one query's lists.
__global__ __launch_bounds__(64) void rerank_blend_kernel(int max_out, const int* __restrict__ count,
                                                          long long* __restrict__ ids, double* __restrict__ vals,
                                                          int* __restrict__ mask, const double* __restrict__ ce_raw,
                                                          int top_n, double beta, double* __restrict__ out_rerank) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* svals = reinterpret_cast<double*>(smem);                   // [max_out][NVALS]
  double* snew = svals + (size_t)max_out * AMDR_FUSE_NVALS;            // new score per input position
  double* snorm = snew + max_out;                                    // norm per candidate
  long long* sids = reinterpret_cast<long long*>(snorm + max_out);   // [max_out]
  int* smask = reinterpret_cast<int*>(sids + max_out);               // [max_out]
  int* spre = smask + max_out;                                       // position in the pre-sort sequence
  const int lane = threadIdx.x, qi = blockIdx.x;
  const size_t base = (size_t)qi * max_out;
  const int cnt = count[qi];
  const int n = cnt < top_n ? cnt : top_n;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  for (int r = lane; r < max_out; r += 64) {
    out_rerank[(base + r) * 2 + 0] = nan;
    out_rerank[(base + r) * 2 + 1] = nan;
  }
  if (n <= 0) return;

  double mn = INFINITY, mx = -INFINITY;
  for (int j = lane; j < n; j += 64) {
    double r = ce_raw[(size_t)qi * top_n + j];
    mn = fmin(mn, r);
    mx = fmax(mx, r);
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  const bool deg = (mx - mn < 1e-12);

  for (int j = lane; j < cnt; j += 64) {
    for (int x = 0; x < AMDR_FUSE_NVALS; ++x) svals[(size_t)j * AMDR_FUSE_NVALS + x] = vals[(base + j) * AMDR_FUSE_NVALS + x];
    sids[j] = ids[base + j];
    smask[j] = mask[base + j];
    double s = svals[(size_t)j * AMDR_FUSE_NVALS + AMDR_FV_SCORE];
    if (j < n) {
      double raw = ce_raw[(size_t)qi * top_n + j];
      double nm = deg ? 0.0 : (raw - mn) / (mx - mn);
      snorm[j] = nm;
      s = (1 - beta) * s + beta * nm;
    }
    snew[j] = s;
  }
  lds_sync();
  // pre-sort sequence: candidates by norm desc (stable), then the untouched tail
  for (int j = lane; j < cnt; j += 64) {
    int p = j;
    if (j < n) {
      const double nm = snorm[j];
      p = 0;
      for (int i = 0; i < n; ++i) {
        const double o = snorm[i];
        p += (o > nm) || (o == nm && i < j);
      }
    }
    spre[j] = p;
  }
  lds_sync();
  for (int j = lane; j < cnt; j += 64) {
    const double s = snew[j];
    const int pj = spre[j];
    int r = 0;
    for (int i = 0; i < cnt; ++i) {
      const double o = snew[i];
      r += (o > s) || (o == s && spre[i] < pj);
    }
    ids[base + r] = sids[j];
    mask[base + r] = smask[j];
    for (int x = 0; x < AMDR_FUSE_NVALS; ++x) vals[(base + r) * AMDR_FUSE_NVALS + x] = svals[(size_t)j * AMDR_FUSE_NVALS + x];
    vals[(base + r) * AMDR_FUSE_NVALS + AMDR_FV_SCORE] = s;
    if (j < n) {
      out_rerank[(base + r) * 2 + 0] = ce_raw[(size_t)qi * top_n + j];
      out_rerank[(base + r) * 2 + 1] = snorm[j];
    }
  }
}

static size_t rerank_lds(int max_out) {
  return (size_t)max_out * (AMDR_FUSE_NVALS + 2) * sizeof(double) + (size_t)max_out * sizeof(long long) +
         (size_t)max_out * 2 * sizeof(int);
}

int dense_fuse_plain_launch(const FuseTail& t, int q0, int m, int kd, const float* dense_scores, const int64_t* dense_ids,
                            hipStream_t st) {
  const FuseTailArgs a = fuse_tail_args(t, q0, kd, dense_scores, dense_ids);
  launch_fuse(*t.p, a.c0, a.c1, ChanIn::none(), m, a.mo, a.ids, a.vals, a.mask, a.count, st);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

}  // namespace amdr

using namespace amdr;

namespace {

int fuse_check(const amdr_fuse_params_t* p, int nq, int kd, int kb, int kc) {
  AMDR_REQUIRE(p != nullptr, "fuse: null params");
  AMDR_REQUIRE(p->method >= 0 && p->method <= 3, "fuse: unknown method %d", p->method);
  AMDR_REQUIRE(nq >= 0, "fuse: nq=%d", nq);
  AMDR_REQUIRE(kd >= 0 && kd <= AMDR_MAX_K && kb >= 0 && kb <= AMDR_MAX_K && kc >= 0 && kc <= AMDR_MAX_K,
               "fuse: channel depth outside [0,%d]", AMDR_MAX_K);
  AMDR_REQUIRE(kd + kb + kc >= 1, "fuse: all channels empty (max_out would be 0)");
  return AMDR_OK;
}

}  // namespace

// ---- host-pointer conveniences (single-query API path) ---------------------
namespace {
// The host-pointer entry points stage through ONE grow-only device arena per calling thread
// (ten hipMalloc/hipFree pairs per single-query call used to cost more than the kernel).
struct Arena {
  char* base = nullptr;
  size_t cap = 0, used = 0;
  int device = -1;
  ~Arena() {
    if (base) (void)hipFree(base);
  }
  int begin(int dev, size_t total) {
    if (dev != device || total > cap) {
      if (base) (void)hipFree(base);
      base = nullptr;
      cap = 0;
      size_t want = total < (1u << 20) ? (1u << 20) : total;
      AMDR_HIP(hipMalloc((void**)&base, want));
      cap = want;
      device = dev;
    }
    used = 0;
    return AMDR_OK;
  }
  void* take(size_t bytes) {
    void* p = base + used;
    used += (bytes + 255) & ~(size_t)255;
    return p;
  }
};
inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }
Arena& arena() {
  static thread_local Arena a;
  return a;
}
}  // namespace

// Host-pointer forms: inputs are packed into ONE pinned-size-agnostic host block and moved
// with one H2D copy, outputs come back with one D2H copy (every extra small copy from
// pageable memory costs ~10-15 us).
namespace {
struct Pack {
  std::vector<char>& buf;
  size_t used = 0;
  explicit Pack(std::vector<char>& b) : buf(b) {}
  size_t add(const void* src, size_t bytes) {
    size_t off = used;
    used += pad256(bytes);
    if (buf.size() < used) buf.resize(used);
    if (src && bytes) memcpy(buf.data() + off, src, bytes);
    return off;
  }
};
std::vector<char>& host_block() {
  static thread_local std::vector<char> b;
  return b;
}
}  // namespace

namespace amdr {
// The columns a bulk caller reads, compacted on the device so that ONE small copy serves the host API: the first `w`
// fused hits of every query as rows / scores / channel masks (entries past min(count, w): -1 / 0 / 0) + the clipped
// counts.  The full fused record is 9 doubles per candidate and channel-depth x channels candidates per query — 1.6 KB
// per query at top-10 of two channels; PCIe, not the kernels, then bounds a bulk search (hybrid_retriever
// search_batch_arrays: 15 MB per 9 344 queries).  Here: 20 bytes per kept hit.
__global__ __launch_bounds__(256) void fuse_compact_kernel(const long long* __restrict__ ids, const double* __restrict__ vals,
                                                           const int* __restrict__ mask, const int* __restrict__ count,
                                                           int nq, int max_out, int w, long long* __restrict__ out_rows,
                                                           double* __restrict__ out_scores, int* __restrict__ out_mask,
                                                           int* __restrict__ out_count) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)nq * w) return;
  const int q = (int)(i / w), j = (int)(i - (long)q * w);
  const int c = count[q] < w ? count[q] : w;
  const bool keep = j < c;
  const size_t src = (size_t)q * max_out + j;
  out_rows[i] = keep ? ids[src] : -1ll;
  out_scores[i] = keep ? vals[src * AMDR_FUSE_NVALS + AMDR_FV_SCORE] : 0.0;
  out_mask[i] = keep ? mask[src] : 0;
  if (j == 0) out_count[q] = c;
}
}  // namespace amdr

extern "C" {

int amdr_fuse_device(const amdr_fuse_params_t* p, int32_t nq, const int64_t* dense_ids, const float* dense_scores,
                     int32_t kd, const int64_t* dense_row2uid, const int64_t* bm25_ids, const double* bm25_scores,
                     int32_t kb, const int64_t* bm25_row2uid, const int64_t* colbert_ids, const float* colbert_scores,
                     int32_t kc, const int64_t* colbert_row2uid, int64_t* out_ids, double* out_vals,
                     int32_t* out_mask, int32_t* out_count, int32_t device, void* stream) {
  int rc = fuse_check(p, nq, kd, kb, kc);
  if (rc) return rc;
  AMDR_REQUIRE((kd == 0 || (dense_ids && dense_scores)) && (kb == 0 || (bm25_ids && bm25_scores)) &&
                   (kc == 0 || (colbert_ids && colbert_scores)),
               "fuse: null channel buffer");
  AMDR_REQUIRE(nq == 0 || (out_ids && out_vals && out_mask && out_count), "fuse: null output");
  if (nq == 0) return AMDR_OK;
  AMDR_HIP(hipSetDevice(device));
  ChanIn c0{(const long long*)dense_ids, dense_scores, (const long long*)dense_row2uid, kd, 0};
  ChanIn c1{(const long long*)bm25_ids, bm25_scores, (const long long*)bm25_row2uid, kb, 1};
  ChanIn c2{(const long long*)colbert_ids, colbert_scores, (const long long*)colbert_row2uid, kc, 0};
  launch_fuse(*p, c0, c1, c2, nq, kd + kb + kc, (long long*)out_ids, out_vals, out_mask, out_count, (hipStream_t)stream);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

int amdr_rerank_blend_device(int32_t nq, int32_t max_out, const int32_t* count, int64_t* ids, double* vals,
                             int32_t* mask, const double* ce_raw, int32_t top_n, double beta, double* out_rerank,
                             int32_t device, void* stream) {
  AMDR_REQUIRE(nq >= 0 && max_out >= 1 && max_out <= kFuseMax, "rerank_blend: bad sizes");
  AMDR_REQUIRE(top_n >= 1, "rerank_blend: top_n=%d", top_n);
  AMDR_REQUIRE(nq == 0 || (count && ids && vals && mask && ce_raw && out_rerank), "rerank_blend: null buffer");
  if (nq == 0) return AMDR_OK;
  AMDR_HIP(hipSetDevice(device));
  size_t lds = rerank_lds(max_out);
  if (lds > 48 * 1024)
    AMDR_HIP(hipFuncSetAttribute((const void*)rerank_blend_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(rerank_blend_kernel, dim3(nq), dim3(64), lds, (hipStream_t)stream, max_out, count,
                     (long long*)ids, vals, mask, ce_raw, top_n, beta, out_rerank);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

int amdr_fuse_compact_device(int32_t nq, int32_t max_out, int32_t w, const int64_t* ids, const double* vals,
                             const int32_t* mask, const int32_t* count, int64_t* out_rows, double* out_scores,
                             int32_t* out_mask, int32_t* out_count, int32_t device, void* stream) {
  AMDR_REQUIRE(nq >= 0 && max_out >= 1 && w >= 1 && w <= max_out, "fuse_compact: bad sizes (max_out=%d w=%d)", max_out, w);
  if (nq == 0) return AMDR_OK;
  AMDR_REQUIRE(ids && vals && mask && count && out_rows && out_scores && out_mask && out_count, "fuse_compact: null buffer");
  AMDR_HIP(hipSetDevice(device));
  const long total = (long)nq * w;
  hipLaunchKernelGGL(amdr::fuse_compact_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)ids, vals, mask, count, nq, max_out, w, (long long*)out_rows, out_scores, out_mask,
                     out_count);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

int amdr_fuse(const amdr_fuse_params_t* p, int32_t nq, const int64_t* dense_ids, const double* dense_scores, int32_t kd,
              const int64_t* bm25_ids, const double* bm25_scores, int32_t kb, const int64_t* colbert_ids,
              const double* colbert_scores, int32_t kc, int64_t* out_ids, double* out_vals, int32_t* out_mask,
              int32_t* out_count) {
  int rc = fuse_check(p, nq, kd, kb, kc);
  if (rc) return rc;
  if (nq == 0) return AMDR_OK;
  AMDR_REQUIRE((kd == 0 || (dense_ids && dense_scores)) && (kb == 0 || (bm25_ids && bm25_scores)) &&
                   (kc == 0 || (colbert_ids && colbert_scores)) && out_ids && out_vals && out_mask && out_count,
               "fuse: null buffer");
  int dev = 0;
  AMDR_HIP(hipGetDevice(&dev));
  const size_t q = (size_t)nq, mo = (size_t)(kd + kb + kc);
  Pack in(host_block());
  const size_t o_di = in.add(dense_ids, q * kd * 8), o_ds = in.add(dense_scores, q * kd * 8);
  const size_t o_bi = in.add(bm25_ids, q * kb * 8), o_bs = in.add(bm25_scores, q * kb * 8);
  const size_t o_ci = in.add(colbert_ids, q * kc * 8), o_cs = in.add(colbert_scores, q * kc * 8);
  const size_t in_bytes = in.used;
  // outputs follow the inputs in the same device arena, contiguous so one copy brings them back
  const size_t o_oi = in_bytes, o_ov = o_oi + pad256(q * mo * 8), o_om = o_ov + pad256(q * mo * AMDR_FUSE_NVALS * 8),
               o_oc = o_om + pad256(q * mo * 4), total = o_oc + pad256(q * 4);
  if ((rc = arena().begin(dev, total))) return rc;
  char* d = arena().base;
  hipStream_t st = nullptr;
  // the pageable block is sized for the outputs BEFORE the asynchronous copy reads it: growing
  // it afterwards would free the source of a copy that is nominally still in flight
  std::vector<char>& hb = host_block();
  if (hb.size() < total) hb.resize(total);
  AMDR_HIP(hipMemcpyAsync(d, hb.data(), in_bytes, hipMemcpyHostToDevice, st));
  ChanIn c0{(const long long*)(d + o_di), d + o_ds, nullptr, kd, 1};
  ChanIn c1{(const long long*)(d + o_bi), d + o_bs, nullptr, kb, 1};
  ChanIn c2{(const long long*)(d + o_ci), d + o_cs, nullptr, kc, 1};
  launch_fuse(*p, c0, c1, c2, nq, (int)mo, (long long*)(d + o_oi), (double*)(d + o_ov), (int*)(d + o_om),
              (int*)(d + o_oc), st);
  AMDR_HIP(hipGetLastError());
  AMDR_HIP(hipMemcpyAsync(hb.data() + o_oi, d + o_oi, total - o_oi, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipStreamSynchronize(st));
  memcpy(out_ids, hb.data() + o_oi, q * mo * 8);
  memcpy(out_vals, hb.data() + o_ov, q * mo * AMDR_FUSE_NVALS * 8);
  memcpy(out_mask, hb.data() + o_om, q * mo * 4);
  memcpy(out_count, hb.data() + o_oc, q * 4);
  return AMDR_OK;
}

int amdr_rerank_blend(int32_t nq, int32_t max_out, const int32_t* count, int64_t* ids, double* vals, int32_t* mask,
                      const double* ce_raw, int32_t top_n, double beta, double* out_rerank) {
  AMDR_REQUIRE(nq >= 0 && max_out >= 1 && max_out <= kFuseMax && top_n >= 1, "rerank_blend: bad sizes");
  if (nq == 0) return AMDR_OK;
  AMDR_REQUIRE(count && ids && vals && mask && ce_raw && out_rerank, "rerank_blend: null buffer");
  int dev = 0, rc;
  AMDR_HIP(hipGetDevice(&dev));
  const size_t q = (size_t)nq, mo = (size_t)max_out;
  Pack in(host_block());
  const size_t o_c = in.add(count, q * 4), o_r = in.add(ce_raw, q * top_n * 8);
  // in/out arrays next, contiguous, so one copy each way covers ids, vals, mask (+ rerank out)
  const size_t o_i = in.add(ids, q * mo * 8), o_v = in.add(vals, q * mo * AMDR_FUSE_NVALS * 8),
               o_m = in.add(mask, q * mo * 4);
  const size_t in_bytes = in.used;
  const size_t o_o = in_bytes, total = o_o + pad256(q * mo * 16);
  if ((rc = arena().begin(dev, total))) return rc;
  char* d = arena().base;
  hipStream_t st = nullptr;
  // the pageable block is sized for the outputs BEFORE the asynchronous copy reads it: growing
  // it afterwards would free the source of a copy that is nominally still in flight
  std::vector<char>& hb = host_block();
  if (hb.size() < total) hb.resize(total);
  AMDR_HIP(hipMemcpyAsync(d, hb.data(), in_bytes, hipMemcpyHostToDevice, st));
  rc = amdr_rerank_blend_device(nq, max_out, (const int32_t*)(d + o_c), (int64_t*)(d + o_i), (double*)(d + o_v),
                                (int32_t*)(d + o_m), (const double*)(d + o_r), top_n, beta, (double*)(d + o_o), dev, st);
  if (rc) return rc;
  AMDR_HIP(hipMemcpyAsync(hb.data() + o_i, d + o_i, total - o_i, hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipStreamSynchronize(st));
  memcpy(ids, hb.data() + o_i, q * mo * 8);
  memcpy(vals, hb.data() + o_v, q * mo * AMDR_FUSE_NVALS * 8);
  memcpy(mask, hb.data() + o_m, q * mo * 4);
  memcpy(out_rerank, hb.data() + o_o, q * mo * 16);
  return AMDR_OK;
}


}  // extern "C"

// Dense channel: exact inner-product scan + fused top-k for gfx950.
//
// Replaces faiss `index.search(q_vec, k)` (legalrag/retrieval/dense_retriever.py:42).
// The chunk matrix X[n, d] (fp32, row-major) is streamed from HBM exactly once
// per pass of NQ queries: a wave owns a row at a time, lane l holds the float4
// pieces at columns 4l + 256c, the NQ query vectors live in registers, and the
// per-row partial sums are folded with DPP row operations (no LDS round trip).
// Scores never go to memory: each wave keeps its own top-k staging buffer in
// LDS (topk.hpp), one list per block is written out and a second small kernel
// merges the per-block lists.  HBM-bound by construction: algorithmic bytes
// = n*d*4 per pass, flops = 2*n*d*NQ.
#include "call_scratch.hpp"
#include "common.hpp"
#include "dense_dot.hpp"
#include "dense_fp16.hpp"
#include "dense_hi_image.hpp"
#include "rows_compact.hpp"
#include "topk.hpp"
#include "topk_merge.hpp"

#include <algorithm>
#include <cfloat>
#include <mutex>
#include <new>
#include <vector>

namespace amdr {

constexpr int kWaves = 4;  // 256-thread blocks

// grid: (x = row slabs, y = query groups of NQ).  LDS: TopkLds of kWaves*NQ lists (query b's group: lists b*kWaves ...)
// over one set of kWaves counts.
// NT: the chunk matrix is read with the non-temporal cache policy.  A matrix that does not fit the
// 256 MiB Infinity Cache is read once per scan and gains nothing from being kept: measured on
// 10 M x 768 (30.7 GB), one query per scan 4.85-4.96 -> 4.44-4.58 ms (6.3 -> 6.7-6.9 TB/s), four queries
// 4.98 -> 4.64 ms.  Smaller matrices keep the default policy (a repeated scan is then served on-die).
template <int NQ, int CH, int U, bool NT>
__global__ __launch_bounds__(256) void dense_scan_topk_kernel(const float* __restrict__ X, long n, int d,
                                                               const float* __restrict__ Q, int nq_total, int k,
                                                               int cap, long rows_per_block,
                                                               C32* __restrict__ part /*[gridDim.x][nq_total][k]*/,
                                                               float* __restrict__ fin_scores /* single slab */,
                                                               long long* __restrict__ fin_ids) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const TopkLds<C32> L(smem, kWaves * NQ, cap);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int qbase = blockIdx.y * NQ;

  float4 q[NQ][CH];
#pragma unroll
  for (int b = 0; b < NQ; ++b) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      int col = c * 256 + lane * 4;
      bool ok = (qbase + b < nq_total) && (col < d);
      q[b][c] = ok ? *reinterpret_cast<const float4*>(Q + (size_t)(qbase + b) * d + col) : make_float4(0, 0, 0, 0);
    }
  }

  WaveTopK<C32> tk[NQ];
#pragma unroll
  for (int b = 0; b < NQ; ++b) tk[b].init(L.list(b * kWaves + wave), cap, k);

  const long row_lo = (long)blockIdx.x * rows_per_block;
  long row_hi = row_lo + rows_per_block;
  if (row_hi > n) row_hi = n;

  for (long r0 = row_lo + (long)wave * U; r0 < row_hi; r0 += (long)kWaves * U) {
    float4 x[U][CH];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      long r = r0 + u;
      if (r >= row_hi) r = row_hi - 1;  // clamp: keeps the loads unconditional
      const float* xr = X + (size_t)r * d;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        int col = c * 256 + lane * 4;
        if (NT) {
          const f32x4 t_ = (col < d) ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(xr + col)) : f32x4{0, 0, 0, 0};
          x[u][c] = make_float4(t_.x, t_.y, t_.z, t_.w);
        } else {
          x[u][c] = (col < d) ? *reinterpret_cast<const float4*>(xr + col) : make_float4(0, 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long r = r0 + u;
      const bool rv = r < row_hi;
#pragma unroll
      for (int b = 0; b < NQ; ++b) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) acc = dot4(x[u][c], q[b][c], acc);
        acc = wave_sum_to_lane63(acc);
        float s = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 63));
        if (rv) tk[b].push_uniform(C32::make(s, (u32)r), lane);
      }
    }
  }

#pragma unroll
  for (int b = 0; b < NQ; ++b) tk[b].finalize(lane);
#pragma unroll
  for (int b = 0; b < NQ; ++b) {
    block_combine_topk(tk[b], L.list(b * kWaves), cap, kWaves, wave, lane, L.cnts);
    if (wave == 0 && qbase + b < nq_total)
      topk_emit(tk[b].buf, tk[b].cnt, k, lane, fin_scores, fin_ids, (size_t)(qbase + b), part,
                (size_t)blockIdx.x * nq_total + (qbase + b));
    __syncthreads();
  }
}

// Score an explicit candidate list: out[q][j] = <Q[q], X[rows[q][j]]> (rows < 0 -> -FLT_MAX).
// One wave per (query, candidate): the row is gathered with three coalesced 1-KiB loads.
// Stands where GraphRetriever re-embeds its candidates per query and takes cosines
// (legalrag/retrieval/graph_retriever.py:177-191): the chunk embeddings are already in HBM.
__global__ __launch_bounds__(256) void dense_score_rows_kernel(const float* __restrict__ X, long n, int d,
                                                                const float* __restrict__ Q, int nq,
                                                                const long long* __restrict__ rows, int m,
                                                                float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long idx = (long)blockIdx.x * kWaves + wave;
  if (idx >= (long)nq * m) return;
  const int qi = (int)(idx / m);
  const long long r = rows[idx];
  if (r < 0 || r >= n) {
    if (lane == 0) out[idx] = -FLT_MAX;
    return;
  }
  const float acc = dense_row_dot(X + (size_t)r * d, Q + (size_t)qi * d, d, lane);
  if (lane == 63) out[idx] = acc;
}

// Short corpus, 1-4 queries (the single-query serving call at UCC-en / Civil-Code size): one
// wave per (query, row) writes S[q][row]; the slab top-k of dense_mfma.hip ranks it.  A row-slab
// scan with per-wave top-k state is latency-bound here (591 rows = 40 waves walking 15 rows each,
// then a merge launch: 15.6 + 8.1 us); 591 independent waves finish in one memory round trip.
__global__ __launch_bounds__(256) void dense_all_scores_kernel(const float* __restrict__ X, long n, int d,
                                                                const float* __restrict__ Q, int nq, long ldS,
                                                                float* __restrict__ S) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long idx = (long)blockIdx.x * kWaves + wave;
  if (idx >= (long)nq * n) return;
  const int qi = (int)(idx / n);
  const long r = idx - (long)qi * n;
  const float acc = dense_row_dot(X + (size_t)r * d, Q + (size_t)qi * d, d, lane);
  if (lane == 63) S[(size_t)qi * ldS + r] = acc;
}

}  // namespace amdr

using namespace amdr;

constexpr int kSideEvents = 2;  // fork, join
struct amdr_dense {
  int device = 0;
  int64_t n = 0;
  int64_t cap_rows = 0;
  int d = 0;
  float* X = nullptr;
  bool owns = true;
  hipStream_t stream = nullptr;
  std::mutex mu;
  // Two workspaces: [0] for the "_device" entry points (kernels enqueued on the CALLER's stream,
  // the call returns before they run), [1] for the host-pointer entry points (own stream,
  // synchronised before the mutex is released).  A service thread in amdr_dense_search can
  // therefore never scribble over the score matrix of a search_batch still in flight on another
  // stream.  "_device" calls on ONE handle from SEVERAL streams remain the caller's to order.
  DevBuf part[2], smat[2], aux[2], qbuf, sbuf, ibuf;  // aux: the per-query tile lists of the two-level top-k
  // matrix statistics for both fp16 first passes (dense_fp16.hpp: the device words, among them the large scan's counters,
  // and the record; finite only if d is supported): kept up to date by create / add
  DevBuf stats;
  DenseFp16Stats fp16;
  int64_t hi_queries = 0;    // queries that went through the fp16 first pass (amdr_dense_hi_counters)
  // adaptive width of the candidate cut: level l re-scores k + max(k, kHiExtra[l]) + 1 tiles per query; a handle whose
  // queries the rounding bound keeps failing to resolve moves up a level, and at the top level gives the pass up
  int hi_level = 0;
  bool hi_off = false;
  int64_t hi_passes = 0;        // passes (<= 64 queries each) through the fp16 first pass
  int64_t lvl_p0 = 0;           // device pass / flagged-pass counters when the current level was entered
  unsigned int lvl_f0 = 0;
  unsigned int* hi_host = nullptr;  // pinned: the device's (unresolved queries, flagged passes, passes), copied back after every search
  hipEvent_t hi_ev = nullptr;       // recorded behind that copy: hi_adapt reads hi_host only once it has completed
  bool hi_copy_pending = false;
  unsigned int hi_seen[3] = {0u, 0u, 0u};  // the last completed copy
  // two-pass long-batch form on a short corpus (dense_small_hi.hip + dense_tail.hip dense_hi_select_fuse_kernel): the fp16 image
  // of X, made on first use (not while a stream is capturing) and dropped by add(); the per-query bounds; how many queries
  // re-scored their whole row inside the second pass
  amdr_dense_small_t* small = nullptr;
  bool small_failed = false;
  DevBuf small_eps, small_fb;
  // optional resident fp16 image of X for the large scan's first pass (dense_hi_image.hpp): made by amdr_dense_image_build
  // only, kept current by add (image_sync), never touched by a search; not workspace.  Present = it holds img_rows == n
  // rows converted with img_scale == fp16.x_scale
  void* img = nullptr;
  int64_t img_cap_rows = 0, img_rows = 0;
  float img_scale = 0.f;
  double remove_kernel_ms = -1.0;  // device time of the compaction kernel of the last successful amdr_dense_remove
  double replace_kernel_ms = -1.0;  // device time of the scatter kernel of the last successful amdr_dense_replace
  // optional HIP-event ring bracketing the scan kernel alone (bench.py roofline)
  std::vector<hipEvent_t> prof_ev;
  int prof_used = 0;
  bool prof_on = false;
  // the overlapped long-batch hybrid step (amdr_hybrid_batch_device): one non-blocking side stream and the events of
  // its fork from / join to the caller's stream (timing disabled), made by create / reserve — a call only enqueues
  hipStream_t side = nullptr;
  hipEvent_t side_ev[kSideEvents] = {};
};

namespace {

struct ScanPlan {
  int nq_per_block;  // NQ template
  int ch;
  int cap;
  long rows_per_block;
  int grid_x, grid_y;
  size_t lds;
  size_t part_bytes;
};

int make_plan(int64_t n, int d, int nq, int k, ScanPlan* p) {
  p->ch = ceil_div(d, 256);
  p->cap = topk_cap(k);
  // queries per pass: as many as fit 64 KiB of LDS staging and the register budget
  int nqb = 8;
  while (nqb > 1 && (size_t)kWaves * nqb * p->cap * sizeof(C32) > 60 * 1024) nqb >>= 1;
  if (p->ch >= 4 && nqb > 4) nqb = 4;  // d = 1024: 8 query vectors would spill
  while (nqb > 1 && nqb / 2 >= nq) nqb >>= 1;
  p->nq_per_block = nqb;
  const int U = (nqb <= 2) ? 4 : 2;
  // Row slabs: enough blocks to fill 256 CUs several times over, but never thinner than a
  // few iterations per wave — the per-block top-k finalisation is a fixed cost per slab,
  // so when there are already many query groups (grid_y) the slabs get fatter instead.
  p->grid_y = ceil_div(nq, nqb);
  long min_rows = (long)kWaves * U * 4;
  long want_blocks = 256L * 8;
  long gx = (want_blocks + p->grid_y - 1) / p->grid_y;
  long gx_max = (n + min_rows - 1) / min_rows;
  if (gx > gx_max) gx = gx_max;
  if (gx < 1) gx = 1;
  p->rows_per_block = (n + gx - 1) / gx;
  // round the slab to a multiple of the block's row stride so waves stay aligned
  long stride = (long)kWaves * U;
  p->rows_per_block = ((p->rows_per_block + stride - 1) / stride) * stride;
  if (p->rows_per_block < stride) p->rows_per_block = stride;  // empty index: keep the divisor non-zero
  p->grid_x = (int)((n + p->rows_per_block - 1) / p->rows_per_block);
  if (p->grid_x < 1) p->grid_x = 1;
  p->grid_y = ceil_div(nq, nqb);
  p->lds = TopkLds<C32>::bytes(kWaves * nqb, p->cap, kWaves);
  p->part_bytes = (size_t)p->grid_x * nq * k * sizeof(C32);
  return AMDR_OK;
}

template <int NQ, int CH>
void launch_scan(const ScanPlan& p, const amdr_dense* h, const float* Q, int nq, int k, C32* part, float* fs,
                 int64_t* fi, hipStream_t st) {
  constexpr int U = (NQ <= 2) ? 4 : 2;
  if (dense_stream_nontemporal((long)h->n, h->d))
    hipLaunchKernelGGL((dense_scan_topk_kernel<NQ, CH, U, true>), dim3(p.grid_x, p.grid_y), dim3(256), p.lds, st, h->X,
                       (long)h->n, h->d, Q, nq, k, p.cap, p.rows_per_block, part, fs, (long long*)fi);
  else
    hipLaunchKernelGGL((dense_scan_topk_kernel<NQ, CH, U, false>), dim3(p.grid_x, p.grid_y), dim3(256), p.lds, st, h->X,
                       (long)h->n, h->d, Q, nq, k, p.cap, p.rows_per_block, part, fs, (long long*)fi);
}

template <int NQ>
int launch_scan_ch(const ScanPlan& p, const amdr_dense* h, const float* Q, int nq, int k, C32* part, float* fs,
                   int64_t* fi, hipStream_t st) {
  switch (p.ch) {
    case 1: launch_scan<NQ, 1>(p, h, Q, nq, k, part, fs, fi, st); break;
    case 2: launch_scan<NQ, 2>(p, h, Q, nq, k, part, fs, fi, st); break;
    case 3: launch_scan<NQ, 3>(p, h, Q, nq, k, part, fs, fi, st); break;
    case 4: launch_scan<NQ, 4>(p, h, Q, nq, k, part, fs, fi, st); break;
    default: return fail(AMDR_EINVAL, "dense: unsupported dim %d", h->d);
  }
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

// ---- queries per pass of each form ---------------------------------------------------------------------------------------
// Batched forms (dense_mfma.hip, dense_panel.hip): the score matrix workspace is bounded, so very large batches go in
// chunks of queries.
constexpr size_t kScoreBytesMax = (size_t)4 << 30;
int batched_chunk(const amdr_dense* h, int nq) {
  size_t per_q = (size_t)h->n * sizeof(float);
  long c = (long)(kScoreBytesMax / (per_q ? per_q : 1));
  c = (c / 32) * 32;
  if (c < 32) c = 32;
  return nq < c ? nq : (int)c;
}

// Two-level top-k for batches on a matrix far larger than the caches (the 10 M-row scans): the score matrix of the
// plain two-pass form is 4 B x queries per row — 1.28 GB per 32 queries on 10 M rows, written and read back once, and
// its stores interleave with the read stream at the HBM (timing-only build without them: 5.80 -> 5.10 ms).  Here:
//   1. the tile kernel keeps, per 32-row tile and query, only the MAXIMUM  (n/32 x queries floats: 40 MB);
//   2. top-k of each query's tile maxima (slab lists + merge) -> its k candidate tiles, ascending, in its own list;
//   3. one wave per (query, tile) re-scores them (same loads, same MFMA k order: the same bits as a full pass);
//   4. top-k of each query's re-scored columns, columns -> row ids.
// Exact: at most k - 1 tiles hold a score above a query's k-th best s_k, so the k-th largest tile maximum T <= s_k
// and every tile that holds one of the top k has a maximum >= T; among tiles AT T the lower tile ids are kept, which
// is where the lower row ids of equal scores live.  Steps 2-4 are exact_tail below (kernels: dense_mfma.hip).
// Queries per pass: 8 192 / k in whole 32-query tiles, at most 96.  Nothing in the tail bounds it any more (the value
// once kept the pass's candidate tiles within one wave's sort); it is kept so that the scan launches of every call
// stay what they were.
int two_level_chunk(int nq, int k) {
  int c = (8192 / k) / 32 * 32;  // >= 32 for every k <= AMDR_MAX_K = 256
  if (c < 32) c = 32;
  if (c > 96) c = 96;
  return nq < c ? nq : c;
}

// The fp16 first pass (dense_hi.hip): the tile maxima of step 1 come from v_mfma_f32_32x32x16_f16 on fp16 roundings of
// both operands — 64 queries per scan instead of 32, the scan bound by HBM alone.  Approximate maxima a(t) lie within
// eps_q of the exact ones (dense_hi_select_kernel states the bound), so the candidate set is widened: the kc = k +
// max(k, 22) + 1 tiles with the largest a(t) are re-scored, and the answer is exact if the kc-th largest a(t) lies below
// T_k - 2 eps_q (T_k = the k-th largest): the k tiles on top have exact maxima >= T_k - eps, hence s_k >= T_k - eps,
// and a tile holding a row >= s_k has a(t) >= s_k - eps >= T_k - 2 eps — it is among the first kc - 1.  Steps 3-4 are
// exact: same ids, same score bits.  A query the bound does not separate raises a device flag; exact steps 1-2 are
// enqueued behind, gated on that flag (no host round trip), and give that query its k tiles.
// Extra candidates: the tiles expected within 2 eps below the cut grow with k (about 0.4 k on unit-norm Gaussian rows)
// and with how tightly the matrix clusters around a query's best rows, which only the data knows: three widths.
constexpr int kHiLevels = 3;
constexpr int kHiExtra[kHiLevels] = {22, 54, 96};
int hi_kc(int k, int level) { return k + (k > kHiExtra[level] ? k : kHiExtra[level]) + 1; }
int hi_kc_max(int k) { return hi_kc(k, kHiLevels - 1); }
constexpr int kHi2Tiles = 4;  // query tiles per pass of the round-4 tail: 256 queries (192 at d = 1 024) share one tail
int hi2_chunk(const amdr_dense* h, int nq) {
  const int c = kHi2Tiles * dense_hi_max_queries(h->d);
  return nq < c ? nq : c;
}

// ---- the route: which form a search of nq queries at depth k takes ----------------------------------------------------------
// The environment pins that steer it, read once per call (tests set them between calls of one process: nothing is kept
// from one call to the next).
struct DensePins {
  char two_level = 0, hi = 0;  // AMDR_DENSE_TWO_LEVEL, AMDR_DENSE_HI: '0' off, '1' on wherever there are enough tiles (tests)
  bool hi_level_set = false;   // AMDR_DENSE_HI_LEVEL: pins the width of the fp16 pass's candidate cut (tests, A/B);
  int hi_level = -1;           // set, but not a level: the handle keeps the width it has
  bool small_hi = true;        // AMDR_DENSE_SMALL_HI=0 pins the exact form of long batches on a short corpus
  int small_hi_min = 4096;     // AMDR_DENSE_SMALL_HI_MIN: the batch size its fp16 two-pass form starts at
  bool hi_image = true;        // AMDR_DENSE_HI_IMAGE=0: the fp16 first pass of large scans ignores the handle's image (tests, A/B)
};
DensePins read_pins() {
  auto pin = [](const char* name) { const char* e = getenv(name); return e && (e[0] == '0' || e[0] == '1') ? e[0] : '\0'; };
  DensePins p;
  p.two_level = pin("AMDR_DENSE_TWO_LEVEL");
  p.hi = pin("AMDR_DENSE_HI");
  const char* l = getenv("AMDR_DENSE_HI_LEVEL");
  p.hi_level_set = l != nullptr;
  if (l && l[0] >= '0' && l[0] < '0' + kHiLevels) p.hi_level = l[0] - '0';
  p.small_hi = pin("AMDR_DENSE_SMALL_HI") != '0';
  const char* mn = getenv("AMDR_DENSE_SMALL_HI_MIN");
  if (mn && atoi(mn) > 0) p.small_hi_min = atoi(mn);
  p.hi_image = pin("AMDR_DENSE_HI_IMAGE") != '0';
  return p;
}

enum class Form {
  Scan,      // dense_scan_topk_kernel: the GEMV scan with per-wave top-k (+ merge)
  RowWaves,  // one wave per (query, row) writes the score matrix, slab top-k ranks it
  Batched,   // the score matrix from MFMA tiles, the panel kernel or the fp16 two-pass form; slab top-k or fused select
  TwoLevel,  // exact two-level top-k
  Hi,        // two-level top-k behind the fp16 first pass
};
struct Route {
  Form form;
  int chunk;         // queries per pass (the last pass of a call may be shorter)
  bool hi;           // the fp16 first pass applies to this call: form Hi, or TwoLevel on a handle that gave the pass up
  int hi_level, kc;  // form Hi: the width level of the candidate cut, the tiles re-scored per query
};
constexpr int kBatchedMin = 5;  // measured: from 5 queries up one MFMA tile pass beats the 8-query GEMV pass
constexpr int64_t kRowWavesMax = 16384;  // rows up to which fewer queries take one wave per (query, row)
// In nq the route has two thresholds, both monotone: kBatchedMin, and the batch size from which the exact two-level form
// yields to the panel kernel (the fp16 first pass does not).  Below kBatchedMin, and for a dimension outside the MFMA
// forms, k does not enter.  reserve_need enumerates on these two facts.
Route dense_route(const amdr_dense* h, const DensePins& pins, int nq, int k) {
  Route r{Form::Scan, nq < kGridYMax ? nq : kGridYMax, false, 0, 0};  // (a pass's query groups are the scan's grid y)
  const long n = (long)h->n;
  if (nq >= kBatchedMin && n > 0 && dense_mfma_supported(h->d)) {
    r.form = Form::Batched;
    r.chunk = batched_chunk(h, nq);
    if (pins.two_level == '0') return r;
    const long tiles = (n + 31) / 32;
    const int kc_max = hi_kc_max(k);
    // kc_max <= AMDR_MAX_K: k <= 127; tiles < 2^26: (query, tile) packed in 32 bits of a candidate entry
    r.hi = pins.hi != '0' && h->fp16.large_scan_ok() && kc_max <= AMDR_MAX_K && tiles < (1l << 26) &&
           (pins.hi == '1' ? tiles >= 2L * kc_max : dense_stream_nontemporal(n, h->d) && tiles >= 64L * kc_max);
    if (r.hi && !h->hi_off) {
      r.form = Form::Hi;
      r.chunk = hi2_chunk(h, nq);
      r.hi_level = pins.hi_level >= 0 ? pins.hi_level : h->hi_level;
      r.kc = hi_kc(k, r.hi_level);
    } else if (r.hi ||  // a handle that gave the fp16 pass up runs the exact passes, ungated
               (pins.two_level == '1' ? tiles >= 2L * k                   // pinned on: any matrix with enough tiles
                                      : !dense_panel_supported(n, h->d, r.chunk) &&  // >= 96 queries: the panel kernel
                                            dense_stream_nontemporal(n, h->d) && tiles >= 64L * k)) {
      r.form = Form::TwoLevel;
      r.chunk = two_level_chunk(nq, k);
    }
  } else if (n > 0 && n <= kRowWavesMax) {
    r.form = Form::RowWaves;
    r.chunk = batched_chunk(h, nq);
  }
  return r;
}

// The two-pass form of a LONG batch on a SHORT corpus: approximate scores on the fp16 matrix instructions (16 x the exact
// form's rate), then per query the rows inside a proven margin of its k-th best re-scored exactly.  From
// 4 096 queries per launch (below, the first pass's fixed cost eats the gain: 1 168 queries 28 us against 26 for the whole
// exact search), one slab of <= 1 024 rows, d a multiple of 128, k (+ the BM25 depth when fused) <= 32.
bool small_hi_shape(const amdr_dense* h, const DensePins& pins, int m, int k, int kb) {
  // depth <= 12: the second pass finds its candidates with the pair selector's 32 slots per query; from k ~ 14 up those
  // overflow on most queries and the query re-scores its whole row (37 376 queries on 1 024 x 768: k = 12 230 against 517 us
  // for the exact form, k = 14 465 against 536, k = 20 2 099 against 619)
  return pins.small_hi && m >= pins.small_hi_min && h->n >= 1 && h->n <= 1024 && h->d >= 128 && h->d <= 1024 &&
         h->d % 128 == 0 && k >= 1 && k <= 12 && k + kb <= 32 && h->fp16.short_corpus_ok();
}
// One pass of m queries of the forms that go through a score matrix S[q][row] (Batched, RowWaves; p = its plan): who
// writes S, who ranks it.  What depends on run-time state (small_hi_ready: image present, stream capturing) is decided
// where the pass runs.
struct PassForm {
  enum Scores { RowWaves, Panel, Tiles } scores;  // the exact kernels
  bool small_hi;     // the fp16 two-pass form applies instead of `scores` and the ranking below
  bool select_fuse;  // ranking of the rows and the fusion with the BM25 lists in one kernel (dense_tail.hip dense_select_fuse_kernel);
                     // else slab top-k (+ merge when there are several slabs), then the plain fusion if a tail follows
};
PassForm batched_pass_form(const amdr_dense* h, const DensePins& pins, const Route& r, const DenseMfmaPlan& p, int m, int k,
                           const FuseTail* tail) {
  PassForm f;
  f.scores = r.form == Form::RowWaves ? PassForm::RowWaves : dense_panel_supported((long)h->n, h->d, m) ? PassForm::Panel : PassForm::Tiles;
  f.select_fuse = tail && dense_select_fuse_applies((long)h->n, p.slabs, m, k, tail->kb);
  f.small_hi = r.form == Form::Batched && p.slabs == 1 && (f.select_fuse || !tail) &&
               small_hi_shape(h, pins, m, k, tail ? tail->kb : 0);
  return f;
}

// Between searches (host side, no synchronisation: the counters are whatever the last completed copy-back left).  One
// unresolved query sends its whole pass through the exact first pass as well, so what is counted is PASSES whose flag
// went up: more than 10 % of >= 4 passes at this width -> the next width (+3 % per pass); at the widest, more than half
// -> the exact passes alone are cheaper (1 + 2 f > 2).  True: the handle's route changed.
bool hi_adapt(amdr_dense* h, const DensePins& pins) {
  if (!h->hi_host || h->hi_off || pins.hi_level_set) return false;
  // the counters are whatever the last COMPLETED copy-back left: the pinned words are read only after the event behind
  // their copy has been reached (round 3 read them while a copy could still be in flight)
  if (h->hi_copy_pending) {
    if (hipEventQuery(h->hi_ev) != hipSuccess) return false;  // still on its way: adapt at the next search
    h->hi_copy_pending = false;
    for (int i = 0; i < 3; ++i) h->hi_seen[i] = h->hi_host[i];
  }
  const unsigned int f = h->hi_seen[1];
  // passes: counted on the device next to the flags (a hipGraph replay bumps both; the host's own count would not see
  // replays)
  const int64_t passes = (int64_t)h->hi_seen[2];
  const int64_t p = passes - h->lvl_p0;
  const int64_t bad = (int64_t)(f - h->lvl_f0);
  if (p < 4) return false;
  bool move = false;
  if (h->hi_level + 1 < kHiLevels) {
    move = bad * 10 > p;
    if (move) ++h->hi_level;
  } else {
    move = bad * 2 > p && pins.hi != '1';  // this matrix is not for the fp16 pass
    if (move) h->hi_off = true;
  }
  if (move || p >= (1 << 16)) {  // a new window
    h->lvl_p0 = passes;
    h->lvl_f0 = f;
  }
  return move;
}

// ---- workspaces -----------------------------------------------------------------------------------------------------
// Workspace of one pass of the two-level forms.  Both use
//   smat: tile maxima M [m][ldM] | re-scored columns S2 [m][32 kc];   aux: list [m][kc] | count [m];
// the exact form (kc = k) adds
//   part: the slab lists of the top-k over M   (the k tiles it picks per query, ids [m][k] | maxima [m][k], pass through
//         the head of S2, 12 of its 128 bytes per (query, tile): read by the ordering step before the re-scoring writes S2);
// the fp16 form (kc = its candidate cut; M written only when the flag goes up) adds, behind them,
//   smat: sample maxima MT [qtiles][items][64] | per-query candidate lists [m][qcap];   aux: unres [m] | tau [m] | qcount [m] | the gate flag.
struct TwoLevelLayout {
  int qtiles, kc;
  long tiles, ldM, ldS2;
  size_t qcap;
  DenseMfmaPlan scan, tk1;  // the tile-maxima scan; exact form: the top-k over its output (columns = tiles)
  size_t off_S2, off_MT, off_qlist, smat_bytes;
  size_t off_count, off_unres, off_tau, off_qcount, off_flag, aux_bytes, part_bytes;
};
void two_level_layout(const amdr_dense* h, int m, int k, int kc, bool hi, TwoLevelLayout* p, bool grids = true) {
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  *p = TwoLevelLayout{};
  const int qt = dense_hi_max_queries(h->d);
  p->qtiles = (m + qt - 1) / qt;
  p->kc = kc;
  p->tiles = ((long)h->n + 31) / 32;
  dense_mfma_plan((long)h->n, h->d, m, k, &p->scan, grids);
  p->ldM = (p->tiles + 31) / 32 * 32;
  p->scan.ld = p->ldM;  // (the tile-maxima scan writes one float per tile)
  p->ldS2 = (long)kc * 32;
  p->off_S2 = up((size_t)m * p->ldM * sizeof(float));
  p->off_MT = p->off_S2 + up((size_t)m * p->ldS2 * sizeof(float));
  p->smat_bytes = p->off_MT;
  p->off_count = up((size_t)m * kc * sizeof(int));
  p->off_unres = p->aux_bytes = p->off_count + up((size_t)m * sizeof(int));
  if (!hi) {
    dense_mfma_plan(p->tiles, h->d, m, k, &p->tk1, false);  // only its top-k half is used (tk1.ld == ldM)
    p->part_bytes = p->tk1.part_bytes;
    return;
  }
  p->qcap = dense_hi2_qcap((long)h->n, p->qtiles, kc);
  p->off_qlist = p->off_MT + up((size_t)(2048 + 64 * kHi2Tiles) * 64 * sizeof(float));  // [queries][items rounded up to 64]
  p->smat_bytes = p->off_qlist + up((size_t)m * p->qcap * sizeof(C32));
  p->off_tau = p->off_unres + up((size_t)m * sizeof(int));
  p->off_qcount = p->off_tau + up((size_t)m * sizeof(float));
  p->off_flag = p->off_qcount + up((size_t)m * sizeof(unsigned int));
  p->aux_bytes = p->off_flag + 256;
}

struct Need {  // bytes of smat / part / aux
  size_t smat, part, aux;
  void add(const Need& o) { smat = std::max(smat, o.smat), part = std::max(part, o.part), aux = std::max(aux, o.aux); }
};
// the score scratch of the one-launch serving step (dense_small_raw): nq rows of S
size_t score_rows_bytes(const amdr_dense* h, int nq) { return (size_t)nq * (size_t)(((long)h->n + 31) / 32 * 32) * sizeof(float); }

// One pass of m queries at depth k, from the plans the pass itself runs on (sizes only: without their launch grids).
// Form Hi is sized for its widest candidate cut: the width level a handle has learnt does not enter.
Need pass_need(const amdr_dense* h, Form form, int m, int k) {
  if (form == Form::Scan) {
    ScanPlan p;
    make_plan(h->n, h->d, m, k, &p);
    return {0, p.part_bytes, 0};
  }
  if (form == Form::TwoLevel || form == Form::Hi) {
    TwoLevelLayout p;
    two_level_layout(h, m, k, form == Form::Hi ? hi_kc_max(k) : k, form == Form::Hi, &p, false);
    return {p.smat_bytes, p.part_bytes, p.aux_bytes};
  }
  DenseMfmaPlan p;  // RowWaves, Batched
  dense_mfma_plan((long)h->n, h->d, m, k, &p, false);
  return {p.s_bytes, p.part_bytes, 0};
}
// One call: the maximum over every pass its loop will run — the full chunk AND the remainder, planned for its own size
// (a shorter pass can need MORE slab-list space: slabs(m) * m is not monotone in m).  Where the fp16 first pass applies,
// its passes and the exact ones: a handle gives the pass up (and add() gives it back) between a reserve and a call.
// (The fp16 form of TwoLevelLayout has no slab lists and grows with m in every term — m rows of M, S2 and the lists at
// strides that do not depend on m; the sample stride, hence qcap, with the number of query tiles: no remainder.)
Need call_need(const amdr_dense* h, const Route& r, int nq, int k) {
  const Form form = r.hi ? Form::TwoLevel : r.form;
  const int chunk = r.hi ? two_level_chunk(nq, k) : r.chunk;
  Need need = pass_need(h, form, chunk, k);
  if (nq % chunk) need.add(pass_need(h, form, nq % chunk, k));
  if (r.hi) need.add(pass_need(h, Form::Hi, hi2_chunk(h, nq), k));
  return need;
}
// amdr_dense_reserve: the maximum of call_need over every call with nq <= nq_max and k <= k_max.  Within one form and
// pass size the plans grow with k (the slab counts of DenseMfmaPlan do not depend on it), except the scan's, whose
// grid depends on the staging capacity topk_cap(k): monotone inside a capacity class only.
Need reserve_need(const amdr_dense* h, const DensePins& pins, int nq_max, int k_max) {
  Need need{0, 0, 0};
  // 1. the forms whose route k does not enter (see dense_route): every batch size (the scan's slab lists
  //    grid_x(nq, k) * nq * k * 8 are monotone in neither argument; the passes of the row-waves form are the chunks
  //    of these batch sizes) at the deepest k of every capacity class
  int ks[8], nk = 0;
  for (int k = 1; k < k_max; ++k)
    if (topk_cap(k + 1) != topk_cap(k)) ks[nk++] = k;  // three classes up to AMDR_MAX_K
  ks[nk++] = k_max;
  int nq = 1;
  for (; nq <= nq_max; ++nq) {
    const Route r = dense_route(h, pins, nq, k_max);
    if (r.form != Form::Scan && r.form != Form::RowWaves) break;
    for (int i = 0; i < nk; ++i) need.add(pass_need(h, r.form, r.chunk, ks[i]));
    if (r.form == Form::RowWaves) need.add({score_rows_bytes(h, r.chunk), 0, 0});  // (the same bytes: by construction now)
  }
  if (nq > nq_max) return need;
  // 2. batches: at every depth the forms of [nq, nq_max] are those of its two ends (dense_route: one monotone threshold
  //    above the first).  A call's passes — full chunks and a remainder of ANY size — all run its form: every pass
  //    size up to the form's largest.  A smaller k takes more queries per two-level pass (a larger matrix of tile
  //    maxima) and those forms' own applicability depends on k: they at every k, the batched form at its deepest.
  int k_batched = 0;
  for (int k = 1; k <= k_max; ++k) {
    const Route lo = dense_route(h, pins, nq, k), hi = dense_route(h, pins, nq_max, k);
    if (lo.form == Form::Batched || hi.form == Form::Batched) k_batched = k;
    if (hi.hi) need.add(pass_need(h, Form::Hi, hi2_chunk(h, nq_max), k));  // (the fp16 pass does not look at nq)
    if (hi.hi || lo.form == Form::TwoLevel || hi.form == Form::TwoLevel)
      for (int m = two_level_chunk(nq_max, k); m >= 1; --m) need.add(pass_need(h, Form::TwoLevel, m, k));
  }
  if (k_batched)
    for (int m = batched_chunk(h, nq_max); m >= 1; --m) need.add(pass_need(h, Form::Batched, m, k_batched));
  return need;
}
int ensure_need(amdr_dense* h, int ws, const Need& need) {
  int rc = h->smat[ws].ensure(need.smat);
  if (!rc) rc = h->part[ws].ensure(need.part);
  if (!rc) rc = h->aux[ws].ensure(need.aux);
  return rc;
}

// ---- running a search ----------------------------------------------------------------------------------------------------
// `launch` (the scan of a pass) between a pair of the handle's profiling events (amdr_dense_profile_begin / _end:
// bench.py roofline); a ring that is used up brackets nothing
template <class F>
int profiled(amdr_dense* h, hipStream_t st, F&& launch) {
  const bool on = h->prof_on && (size_t)(h->prof_used + 2) <= h->prof_ev.size();
  if (on) AMDR_HIP(hipEventRecord(h->prof_ev[h->prof_used], st));
  const int rc = launch();
  if (rc) return rc;
  if (on) {
    AMDR_HIP(hipEventRecord(h->prof_ev[h->prof_used + 1], st));
    h->prof_used += 2;
  }
  return AMDR_OK;
}

// one top-k pass over a [m][ld] score matrix with `cols` valid columns (slab lists + merge, or direct)
int topk_pass(const DenseMfmaPlan& p, const float* S, long cols, int m, int k, DevBuf& partb, float* out_scores,
              int64_t* out_ids, hipStream_t st) {
  const bool direct = p.slabs == 1;  // one slab: its list is the answer, no merge launch
  int rc = dense_mfma_launch_topk(p, S, cols, m, k, partb.p, direct ? out_scores : nullptr, direct ? out_ids : nullptr, st);
  if (rc || direct) return rc;
  return launch_merge_packed(partb.as<C32>(), p.slabs, m, k, p.cap, out_scores, out_ids, st);
}

// the image and the workspaces of the fp16 two-pass form; false: not available now (allocating the image failed before, or
// a stream is capturing and nothing was reserved) — the caller takes the exact form
bool small_hi_ready(amdr_dense* h, int m, hipStream_t st) {
  if (h->small_failed) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  const bool capturing = st && hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
  if (!h->small) {
    if (capturing) return false;
    if (dense_small_create_from(h->device, h->X, h->n, h->d, h->fp16, &h->small) != AMDR_OK) {
      h->small_failed = true;
      return false;
    }
  }
  const size_t need = (size_t)m * sizeof(float);
  if (capturing && (h->small_eps.cap < need || !h->small_fb.p)) return false;
  if (h->small_eps.ensure(need) != AMDR_OK) return false;
  if (!h->small_fb.p) {
    if (h->small_fb.ensure(sizeof(unsigned int)) != AMDR_OK) return false;
    (void)hipMemset(h->small_fb.p, 0, sizeof(unsigned int));
  }
  return capturing ? true : dense_small_reserve(h->small, m) == AMDR_OK;
}

// Forms Batched and RowWaves: scores S[q][row] (fp32-MFMA tiles or the panel kernel for batches, one wave per (query,
// row) for few queries on a short corpus), then slab top-k (+ merge when there are several slabs); with a tail, the
// fusion pass by pass.
int run_search_batched(amdr_dense* h, int ws, const DensePins& pins, const Route& r, const float* Q_dev, int nq, int k,
                       float* scores_dev, int64_t* ids_dev, hipStream_t st, const FuseTail* tail) {
  float* S = h->smat[ws].as<float>();
  const long n = (long)h->n;
  DenseMfmaPlan p;
  int rc;
  for (int q0 = 0; q0 < nq; q0 += r.chunk) {
    const int m = nq - q0 < r.chunk ? nq - q0 : r.chunk;
    if (q0 == 0 || m != r.chunk) dense_mfma_plan(n, h->d, m, k, &p);
    const PassForm f = batched_pass_form(h, pins, r, p, m, k, tail);
    const float* Qc = Q_dev + (size_t)q0 * h->d;
    float* os = scores_dev + (size_t)q0 * k;
    int64_t* oi = ids_dev + (size_t)q0 * k;
    if (f.small_hi && small_hi_ready(h, m, st)) {
      rc = profiled(h, st, [&] { return amdr_dense_small_approx_device(h->small, Qc, m, S, p.ld, h->small_eps.as<float>(), st); });
      if (rc) return rc;
      if ((rc = dense_hi_select_launch(tail, q0, S, p.ld, n, m, k, h->X, Qc, h->d, h->small_eps.as<float>(), os, oi,
                                       h->small_fb.as<unsigned int>(), st)))
        return rc;
      continue;
    }
    rc = profiled(h, st, [&]() -> int {
      if (f.scores == PassForm::RowWaves) {
        hipLaunchKernelGGL(dense_all_scores_kernel, dim3(ceil_div((long)m * n, kWaves)), dim3(256), 0, st, h->X, n, h->d, Qc,
                           m, p.ld, S);
        AMDR_HIP(hipGetLastError());
        return AMDR_OK;
      }
      if (f.scores == PassForm::Panel) {
        DensePanelPlan pp;
        dense_panel_plan(n, h->d, m, &pp);
        return dense_panel_launch_scores(pp, h->X, n, h->d, Qc, m, p.ld, S, st);
      }
      return dense_mfma_launch_scores(p, h->X, n, h->d, Qc, m, S, st);
    });
    if (rc) return rc;
    if (f.select_fuse) {
      if ((rc = dense_select_fuse_launch(*tail, q0, S, p.ld, n, m, k, p.cap, os, oi, st))) return rc;
      continue;
    }
    if ((rc = topk_pass(p, S, n, m, k, h->part[ws], os, oi, st))) return rc;
    if (tail && (rc = dense_fuse_plain_launch(*tail, q0, m, k, os, oi, st))) return rc;
  }
  return AMDR_OK;
}

// Steps 1-4 of the exact two-level form for the m queries of a pass laid out by p: tile maxima M -> each query's k best
// tiles, ascending, in list [m][p.kc] -> the exact scores of their rows -> final top-k.  gate, unres (device, nullable):
// behind the fp16 first pass steps 1-2 run only when *gate != 0, step 2 only for queries with unres[q] != 0 (one block
// sweeps a query's row of M), and steps 3-4 take the other queries' lists (<= p.kc tiles) as the fp16 pass left them;
// null = always, every query: the k tiles then come from the slab top-k (+ merge) and step 2 only orders them.
int exact_tail(amdr_dense* h, int ws, const TwoLevelLayout& p, const float* Qc, int m, int k, const int* unres, const int* gate,
               float* out_scores, int64_t* out_ids, hipStream_t st) {
  unsigned char* sm = reinterpret_cast<unsigned char*>(h->smat[ws].p);
  unsigned char* ax = reinterpret_cast<unsigned char*>(h->aux[ws].p);
  float* M = reinterpret_cast<float*>(sm);
  float* S2 = reinterpret_cast<float*>(sm + p.off_S2);
  int* list = reinterpret_cast<int*>(ax);
  int* count = reinterpret_cast<int*>(ax + p.off_count);
  const long n = (long)h->n;
  // ungated, the scan is the launch the profiling events bracket (behind the fp16 pass that pass's own scan is)
  auto scan = [&] { return dense_mfma_launch_scores(p.scan, h->X, n, h->d, Qc, m, M, st, true, gate); };
  int rc = gate ? scan() : profiled(h, st, scan);
  if (rc) return rc;
  int64_t* chosen = nullptr;
  if (!gate) {
    chosen = reinterpret_cast<int64_t*>(S2);  // (see TwoLevelLayout)
    if ((rc = topk_pass(p.tk1, M, p.tiles, m, k, h->part[ws], reinterpret_cast<float*>(chosen + (size_t)m * k), chosen, st))) return rc;
  }
  if ((rc = dense_exact_select_launch(M, p.ldM, p.tiles, m, k, p.kc, list, count, unres, gate, chosen, st))) return rc;
  if ((rc = dense_rescore_tiles_launch(h->X, n, h->d, Qc, m, list, count, p.kc, p.kc, p.ldS2, S2, st))) return rc;
  return dense_final_topk_launch(S2, p.ldS2, list, count, p.kc, p.kc, n, m, k, out_scores, out_ids, st);
}

// One pass of <= two_level_chunk queries of the exact form.
int two_level_pass(amdr_dense* h, int ws, const float* Qc, int m, int k, float* out_scores, int64_t* out_ids,
                   hipStream_t st) {
  TwoLevelLayout p;
  two_level_layout(h, m, k, k, false, &p);
  return exact_tail(h, ws, p, Qc, m, k, nullptr, nullptr, out_scores, out_ids, st);
}

// The image the fp16 first pass reads, or null: the fp32 matrix.
const void* hi_image_of(const amdr_dense* h, const DensePins& pins) {
  return pins.hi_image && h->img && h->img_rows == h->n && h->img_scale == h->fp16.x_scale ? h->img : nullptr;
}

// One pass (<= 4 query tiles) of the round-4 tail: see dense_hi.hip.  Launches: sample, tau, one scan per query tile,
// select, then exact_tail behind the flag: [gated: exact tile maxima, exact select], re-scoring, final top-k.
// `image` (nullable): the handle's fp16 image — sample and scan read it instead of X; everything behind them is the same.
int hi2_pass(amdr_dense* h, int ws, const void* image, const float* Qc, int m, int k, int kc, float* out_scores,
             int64_t* out_ids, hipStream_t st) {
  TwoLevelLayout p;
  two_level_layout(h, m, k, kc, true, &p);
  unsigned char* sm = reinterpret_cast<unsigned char*>(h->smat[ws].p);
  unsigned char* ax = reinterpret_cast<unsigned char*>(h->aux[ws].p);
  float* MT = reinterpret_cast<float*>(sm + p.off_MT);
  C32* qlist = reinterpret_cast<C32*>(sm + p.off_qlist);
  int* list = reinterpret_cast<int*>(ax);
  int* count = reinterpret_cast<int*>(ax + p.off_count);
  int* unres = reinterpret_cast<int*>(ax + p.off_unres);
  float* tau = reinterpret_cast<float*>(ax + p.off_tau);
  unsigned int* qcount = reinterpret_cast<unsigned int*>(ax + p.off_qcount);
  int* flag = reinterpret_cast<int*>(ax + p.off_flag);  // (reset by this pass's own tau kernel)
  unsigned int* stats = h->stats.as<unsigned int>();
  int rc;
  if ((rc = dense_hi2_launch_sample(h->X, image, (long)h->n, h->d, Qc, m, p.qtiles, MT, st, h->fp16.x_scale))) return rc;
  if ((rc = dense_hi2_launch_tau(MT, (long)h->n, h->d, m, p.qtiles, kc, tau, qcount, flag, stats, st))) return rc;
  {  // the scan: ONE launch over all query tiles of the pass (the launch the profiling events bracket);
     // AMDR_DENSE_HI_SCANS=split: one launch per query tile (A/B, tests)
    const char* sp = getenv("AMDR_DENSE_HI_SCANS");
    const bool split = sp && sp[0] == 's';
    const int qt = dense_hi_max_queries(h->d);
    for (int y = 0; y < (split ? p.qtiles : 1); ++y) {
      const int q0 = y * qt, mq = split ? (m - q0 < qt ? m - q0 : qt) : m;
      rc = profiled(h, st, [&] {
        return dense_hi2_launch_emit(h->X, image, (long)h->n, h->d, Qc + (size_t)q0 * h->d, mq, tau + q0, qlist + (size_t)q0 * p.qcap,
                                     qcount + q0, p.qcap, st, h->fp16.x_scale, split ? 1 : p.qtiles);
      });
      if (rc) return rc;
    }
  }
  h->hi_queries += m;
  h->hi_passes += p.qtiles;
  if ((rc = dense_hi2_launch_select(qlist, qcount, p.qcap, m, kc, k, Qc, h->d, h->fp16.row_norm_max, h->fp16.x_scale, p.tiles, list,
                                    count, unres, flag, stats + 2, st)))
    return rc;
  // behind the flag: the exact first pass of the batch and, for the queries the bound did not resolve, their k tiles
  return exact_tail(h, ws, p, Qc, m, k, unres, flag, out_scores, out_ids, st);
}

// Forms TwoLevel and Hi.
int run_search_two_level(amdr_dense* h, int ws, const DensePins& pins, Route r, const float* Q_dev, int nq, int k,
                         float* scores_dev, int64_t* ids_dev, hipStream_t st) {
  hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cap_st);
  const bool capturing = cap_st != hipStreamCaptureStatusNone;
  if (r.hi && !capturing && hi_adapt(h, pins)) r = dense_route(h, pins, nq, k);  // a wider cut, or the pass given up
  const bool hi = r.form == Form::Hi;
  const void* image = hi_image_of(h, pins);
  int rc;
  for (int q0 = 0; q0 < nq; q0 += r.chunk) {
    const int m = nq - q0 < r.chunk ? nq - q0 : r.chunk;
    const float* Qc = Q_dev + (size_t)q0 * h->d;
    float* os = scores_dev + (size_t)q0 * k;
    int64_t* oi = ids_dev + (size_t)q0 * k;
    rc = hi ? hi2_pass(h, ws, image, Qc, m, k, r.kc, os, oi, st) : two_level_pass(h, ws, Qc, m, k, os, oi, st);
    if (rc) return rc;
  }
  if (hi && h->hi_host && !capturing && !h->hi_copy_pending) {  // what hi_adapt reads before a later search
    AMDR_HIP(hipMemcpyAsync(h->hi_host, h->stats.as<unsigned int>() + 2, 3 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    AMDR_HIP(hipEventRecord(h->hi_ev, st));
    h->hi_copy_pending = true;
  }
  return AMDR_OK;
}

// One pass of form Scan: m <= kGridYMax queries, so the ceil(m / queries per block) query groups fit the grid's y.
int scan_pass(amdr_dense* h, int ws, const float* Q_dev, int nq, int k, float* scores_dev, int64_t* ids_dev,
              hipStream_t st) {
  ScanPlan p;
  make_plan(h->n, h->d, nq, k, &p);
  C32* part = h->part[ws].as<C32>();
  const bool direct = h->n > 0 && p.grid_x == 1;  // single slab: its list is the answer
  float* fs = direct ? scores_dev : nullptr;
  int64_t* fi = direct ? ids_dev : nullptr;
  if (h->n > 0) {
    const int rc = profiled(h, st, [&] {
      switch (p.nq_per_block) {
        case 1: return launch_scan_ch<1>(p, h, Q_dev, nq, k, part, fs, fi, st);
        case 2: return launch_scan_ch<2>(p, h, Q_dev, nq, k, part, fs, fi, st);
        case 4: return launch_scan_ch<4>(p, h, Q_dev, nq, k, part, fs, fi, st);
        default: return launch_scan_ch<8>(p, h, Q_dev, nq, k, part, fs, fi, st);
      }
    });
    if (rc) return rc;
  }
  if (direct) return AMDR_OK;
  return launch_merge_packed(part, h->n > 0 ? p.grid_x : 0, nq, k, p.cap, scores_dev, ids_dev, st);  // (an empty index: padding)
}

// Form Scan: passes of r.chunk queries, each with its own plan; they share the slab lists one after the other on the stream.
int run_search_scan(amdr_dense* h, int ws, const Route& r, const float* Q_dev, int nq, int k, float* scores_dev,
                    int64_t* ids_dev, hipStream_t st) {
  for (int q0 = 0; q0 < nq; q0 += r.chunk) {
    const int m = nq - q0 < r.chunk ? nq - q0 : r.chunk;
    const int rc = scan_pass(h, ws, Q_dev + (size_t)q0 * h->d, m, k, scores_dev + (size_t)q0 * k, ids_dev + (size_t)q0 * k, st);
    if (rc) return rc;
  }
  return AMDR_OK;
}

// One search on workspace `ws`; with a tail (amdr_dense_search_fuse_device), the fusion behind it — pass by pass in the
// Batched form, one plain launch over the finished lists behind the others.
int run_search(amdr_dense* h, int ws, const float* Q_dev, int nq, int k, float* scores_dev, int64_t* ids_dev,
               hipStream_t st, const FuseTail* tail = nullptr) {
  const DensePins pins = read_pins();
  const Route r = dense_route(h, pins, nq, k);
  int rc = ensure_need(h, ws, call_need(h, r, nq, k));
  if (rc) return rc;
  switch (r.form) {
    case Form::Batched: return run_search_batched(h, ws, pins, r, Q_dev, nq, k, scores_dev, ids_dev, st, tail);
    case Form::RowWaves: rc = run_search_batched(h, ws, pins, r, Q_dev, nq, k, scores_dev, ids_dev, st, nullptr); break;
    case Form::TwoLevel:
    case Form::Hi: rc = run_search_two_level(h, ws, pins, r, Q_dev, nq, k, scores_dev, ids_dev, st); break;
    case Form::Scan: rc = run_search_scan(h, ws, r, Q_dev, nq, k, scores_dev, ids_dev, st); break;
  }
  if (rc || !tail) return rc;
  return dense_fuse_plain_launch(*tail, 0, nq, k, scores_dev, ids_dev, st);
}

int check_search_args(const amdr_dense* h, const void* Q, int nq, int k, const void* s, const void* i) {
  AMDR_REQUIRE(h != nullptr, "dense: null handle");
  AMDR_REQUIRE(nq >= 0, "dense: nq=%d", nq);
  AMDR_REQUIRE(k >= 1 && k <= AMDR_MAX_K, "dense: k=%d outside [1,%d]", k, AMDR_MAX_K);
  AMDR_REQUIRE(nq == 0 || (Q && s && i), "dense: null buffer");
  return AMDR_OK;
}

// Statistics of rows [row0, row0 + rows) folded into the handle's: what the fp16 first passes scale by and bound their
// error with.  Synchronous (create / add are).
int update_stats(amdr_dense* h, int64_t row0, int64_t rows) {
  h->fp16 = DenseFp16Stats();
  if (!dense_hi_supported(h->d)) return AMDR_OK;
  int rc = h->stats.ensure(kDenseStatWords * sizeof(unsigned int));
  if (rc) return rc;
  if (row0 == 0) AMDR_HIP(hipMemsetAsync(h->stats.p, 0, kDenseStatWords * sizeof(unsigned int), h->stream));
  if (!h->hi_host) {
    AMDR_HIP(hipHostMalloc((void**)&h->hi_host, 4 * sizeof(unsigned int), hipHostMallocDefault));
    h->hi_host[0] = h->hi_host[1] = h->hi_host[2] = 0u;
    AMDR_HIP(hipEventCreateWithFlags(&h->hi_ev, hipEventDisableTiming));
  }
  if ((rc = dense_stats_launch(h->X + (size_t)row0 * h->d, (long)rows, h->d, h->stats.as<unsigned int>(), h->stream)))
    return rc;
  unsigned int words[kDenseStatWords] = {};
  AMDR_HIP(hipMemcpyAsync(words, h->stats.p, sizeof(words), hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipStreamSynchronize(h->stream));
  h->fp16 = dense_fp16_stats(words);
  return AMDR_OK;
}

// The side stream and the events of the overlapped hybrid batch step; whatever exists already is kept.
int side_init(amdr_dense* h) {
  if (!h->side) AMDR_HIP(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
  for (hipEvent_t& e : h->side_ev)
    if (!e) AMDR_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return AMDR_OK;
}

// A matrix in the making beside the live one (a growing amdr_dense_add, amdr_dense_remove).  commit() exchanges the two, so
// the destructor frees the OLD matrix after a commit and the new one after a failure — a failed update leaves the matrix it
// had.  (hipFree waits for the device: host-pointer searches are behind h->mu, "_device" work is the caller's to order.)
struct DenseStagedMatrix {
  float* X = nullptr;
  DenseStagedMatrix() = default;
  DenseStagedMatrix(const DenseStagedMatrix&) = delete;
  ~DenseStagedMatrix() { (void)hipFree(X); }
  void commit(amdr_dense* h, int64_t cap_rows) {
    std::swap(h->X, X);
    h->cap_rows = cap_rows;
  }
};

// The matrix changed (every update): the short-corpus fp16 image is of the old one (and may point at freed memory) and is
// made again on demand; what the fp16 first pass learnt about the matrix (width level, given up) starts over.
void first_pass_forget(amdr_dense* h) {
  if (h->small) {
    (void)hipDeviceSynchronize();
    (void)amdr_dense_small_destroy(h->small);
    h->small = nullptr;
  }
  h->small_failed = false;
  h->hi_level = 0;
  h->hi_off = false;
}

// Rows were removed or replaced, so the statistics are about to be taken again from zero (the largest component and row
// norm can fall): first_pass_forget, as in amdr_dense_add — and since the statistics words are made again from zero, the
// device's counters and the host's view of them start from zero too.
void first_pass_start_over(amdr_dense* h) {
  first_pass_forget(h);
  if (h->hi_copy_pending) {
    (void)hipEventSynchronize(h->hi_ev);
    h->hi_copy_pending = false;
  }
  for (int i = 0; i < 3; ++i) h->hi_seen[i] = 0u;
  h->lvl_f0 = 0u;
  h->lvl_p0 = 0;
  h->hi_queries = h->hi_passes = 0;
}

void image_drop(amdr_dense* h) {
  if (h->img) (void)hipFree(h->img);  // (waits for the device: no scan is reading it any more)
  h->img = nullptr;
  h->img_cap_rows = h->img_rows = 0;
  h->img_scale = 0.f;
}

// Brings the image up to the matrix: rows [row0, n) converted if the image has room and its scale is still the
// matrix's, else all of it again in a new allocation (sized like the matrix's own, so that adds within the matrix's
// capacity find room here too).  The callers have checked that the matrix has rows and finite statistics.  Synchronous
// on the handle's stream.
int image_sync(amdr_dense* h, int64_t row0) {
  if (!h->img || h->img_scale != h->fp16.x_scale || h->n > h->img_cap_rows || row0 > h->img_rows) {
    image_drop(h);
    const int64_t cap = h->cap_rows > h->n ? h->cap_rows : h->n;
    AMDR_HIP(hipMalloc(&h->img, hi_image_bytes((long)cap, h->d)));
    h->img_cap_rows = hi_image_tiles((long)cap) * kHiTileRows;
    row0 = 0;
  }
  int rc = dense_hi_image_launch(h->X, (long)row0, (long)h->n, h->d, h->fp16.x_scale, h->img, h->stream);
  if (rc == AMDR_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(AMDR_EHIP, "dense_image: build failed");
  if (rc) {
    image_drop(h);
    return rc;
  }
  h->img_rows = h->n;
  h->img_scale = h->fp16.x_scale;
  return AMDR_OK;
}

// ---- the long-batch hybrid step with BM25 beside the second dense pass (amdr_hybrid_batch_device) --------
// AMDR_HYBRID_BATCH=0 pins the serial calls (tests, A/B)
bool hybrid_batch_on() {
  const char* e = getenv("AMDR_HYBRID_BATCH");
  return !(e && e[0] == '0');
}

struct HybridBatch {  // the call's operands and channel lists (device pointers)
  amdr_bm25_t* bm25;
  const float* Q;
  const int32_t* q_terms;
  const int64_t* q_ptr;
  int nq, kd, kb;
  float* ds;
  int64_t* di;
  double* bs;
  int64_t* bi;
};

// The overlapped step applies to this call: the two-pass dense form as ONE pass, its buffers ready.  p: the pass's plan.
bool hybrid_batch_applies(amdr_dense* h, const DensePins& pins, const HybridBatch& a, const FuseTail& tail, hipStream_t st,
                          Route* r, DenseMfmaPlan* p) {
  if (!hybrid_batch_on() || !h->side || bm25_device_of(a.bm25) != h->device) return false;
  *r = dense_route(h, pins, a.nq, a.kd);
  if (r->form != Form::Batched || a.nq > r->chunk) return false;
  dense_mfma_plan((long)h->n, h->d, a.nq, a.kd, p);
  return batched_pass_form(h, pins, *r, *p, a.nq, a.kd, &tail).small_hi && small_hi_ready(h, a.nq, st);
}

// Split and scores on the caller's stream; behind the scores kernel the fork: BM25 on the side stream beside the second
// dense pass (dense_hi_select_fuse_kernel<false>: the dense lists alone) on the caller's; behind the join the plain
// fusion.  Released any earlier, BM25 takes the block slots first and the split and the scores kernel wait for them.
int hybrid_batch_overlapped(amdr_dense* h, const HybridBatch& a, const FuseTail& tail, const DenseMfmaPlan& p, hipStream_t st) {
  float* S = h->smat[0].as<float>();
  float* eps = h->small_eps.as<float>();
  int rc = profiled(h, st, [&] { return amdr_dense_small_approx_device(h->small, a.Q, a.nq, S, p.ld, eps, st); });
  if (rc) return rc;
  AMDR_HIP(hipEventRecord(h->side_ev[0], st));
  AMDR_HIP(hipStreamWaitEvent(h->side, h->side_ev[0], 0));
  // from here on the branch is open: it is joined whatever happens (a capture must not end with it dangling)
  rc = amdr_bm25_search_device(a.bm25, a.q_terms, a.q_ptr, a.nq, a.kb, a.bs, a.bi, h->side);
  if (!rc)
    rc = dense_hi_select_launch(nullptr, 0, S, p.ld, (long)h->n, a.nq, a.kd, h->X, a.Q, h->d, eps, a.ds, a.di,
                                h->small_fb.as<unsigned int>(), st);
  hipError_t e = hipEventRecord(h->side_ev[1], h->side);
  if (e == hipSuccess) e = hipStreamWaitEvent(st, h->side_ev[1], 0);
  if (rc) return rc;
  AMDR_HIP(e);
  return dense_fuse_plain_launch(tail, 0, a.nq, a.kd, a.ds, a.di, st);
}

}  // namespace

namespace amdr {
int dense_small_raw(amdr_dense_t* h, int nq, DenseRaw* out) {
  int rc = h->smat[0].ensure(score_rows_bytes(h, nq));
  if (rc) return rc;
  out->X = h->X;
  out->n = (long)h->n;
  out->d = h->d;
  out->S = h->smat[0].as<float>();
  out->ld = ((long)h->n + 31) / 32 * 32;
  return AMDR_OK;
}
std::mutex& dense_mutex(amdr_dense_t* h) { return h->mu; }
int dense_device_of(const amdr_dense_t* h) { return h->device; }
const DenseFp16Stats& dense_fp16_stats_of(const amdr_dense_t* h) { return h->fp16; }
int dense_host_stage(amdr_dense_t* h, size_t bytes, void** dev, hipStream_t* st) {
  const int rc = h->sbuf.ensure(bytes);
  if (rc) return rc;
  *dev = h->sbuf.p;
  *st = h->stream;
  return AMDR_OK;
}
void dense_matrix(const amdr_dense_t* h, const float** X, long* n, int* d) {
  *X = h->X;
  *n = (long)h->n;
  *d = h->d;
}
}  // namespace amdr

extern "C" {

int amdr_dense_create(const float* X_host, int64_t n, int32_t d, int32_t device, amdr_dense_t** out) {
  AMDR_REQUIRE(out != nullptr, "dense_create: out is null");
  *out = nullptr;
  AMDR_REQUIRE(n >= 0 && n < (1ll << 32), "dense_create: n=%lld outside [0, 2^32)", (long long)n);
  AMDR_REQUIRE(d >= 4 && d <= AMDR_MAX_DIM && d % 4 == 0, "dense_create: d=%d must be a multiple of 4 in [4,%d]", d,
               AMDR_MAX_DIM);
  AMDR_REQUIRE(n == 0 || X_host != nullptr, "dense_create: X is null");
  int rc = check_device(device);
  if (rc) return rc;
  amdr_dense* h = new (std::nothrow) amdr_dense();
  if (!h) return fail(AMDR_ENOMEM, "dense_create: host alloc");
  h->device = device;
  h->n = n;
  h->d = d;
  h->cap_rows = n;
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess && n > 0) e = hipMalloc((void**)&h->X, (size_t)n * d * sizeof(float));
  if (e == hipSuccess && n > 0) e = hipMemcpy(h->X, X_host, (size_t)n * d * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    amdr_dense_destroy(h);
    return fail(e == hipErrorOutOfMemory ? AMDR_ENOMEM : AMDR_EHIP, "dense_create: %s", hipGetErrorString(e));
  }
  if ((rc = update_stats(h, 0, n)) || (rc = side_init(h))) {
    amdr_dense_destroy(h);
    return rc;
  }
  *out = h;
  return AMDR_OK;
}

int amdr_dense_create_from_device(const float* X_dev, int64_t n, int32_t d, int32_t device, amdr_dense_t** out) {
  AMDR_REQUIRE(out != nullptr, "dense_create_from_device: out is null");
  *out = nullptr;
  AMDR_REQUIRE(n >= 0 && n < (1ll << 32), "dense_create_from_device: n=%lld outside [0, 2^32)", (long long)n);
  AMDR_REQUIRE(d >= 4 && d <= AMDR_MAX_DIM && d % 4 == 0, "dense_create_from_device: bad d=%d", d);
  AMDR_REQUIRE(n == 0 || X_dev != nullptr, "dense_create_from_device: X is null");
  AMDR_REQUIRE(((uintptr_t)X_dev & 15) == 0, "dense_create_from_device: X must be 16-byte aligned");
  int rc = check_device(device);
  if (rc) return rc;
  amdr_dense* h = new (std::nothrow) amdr_dense();
  if (!h) return fail(AMDR_ENOMEM, "dense_create_from_device: host alloc");
  h->device = device;
  h->n = n;
  h->d = d;
  h->cap_rows = n;
  h->X = const_cast<float*>(X_dev);
  h->owns = false;
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    amdr_dense_destroy(h);
    return fail(AMDR_EHIP, "dense_create_from_device: %s", hipGetErrorString(e));
  }
  // The statistics kernel runs on the handle's own (non-blocking) stream: whatever produced X on ANOTHER stream must
  // have finished first, or the largest component / row norm — the fp16 first pass's error bound — would be taken from
  // a half-written matrix.  Creation is synchronous anyway: wait for the device.
  AMDR_HIP(hipDeviceSynchronize());
  if ((rc = update_stats(h, 0, n)) || (rc = side_init(h))) {  // the wrapped matrix must not change while the handle lives
    amdr_dense_destroy(h);
    return rc;
  }
  *out = h;
  return AMDR_OK;
}

// Append rows.  Where the matrix has room the new rows land behind its end, which no search reads; where it has none, a
// grown matrix (double, or to fit) is staged and takes the old one's place only once both copies have arrived.
int amdr_dense_add(amdr_dense_t* h, const float* X_host, int64_t n_add) {
  static const char* const who = "dense_add";
  AMDR_REQUIRE(h != nullptr, "dense_add: null handle");
  AMDR_REQUIRE(h->owns, "dense_add: handle wraps caller-owned memory");
  AMDR_REQUIRE(n_add >= 0 && (n_add == 0 || X_host), "dense_add: bad arguments");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_REQUIRE(h->n + n_add < (1ll << 32), "dense_add: too many rows");
  AMDR_HIP(hipSetDevice(h->device));
  if (n_add == 0) return AMDR_OK;
  const int64_t row0 = h->n, n_new = row0 + n_add;
  {
    DenseStagedMatrix grown;
    float* X = h->X;
    int64_t cap = h->cap_rows;
    if (n_new > cap) {
      cap = cap * 2 > n_new ? cap * 2 : n_new;
      AMDR_TRY(dev_alloc(&grown.X, (size_t)cap * h->d, who));
      X = grown.X;
      if (row0 > 0) AMDR_HIP(hipMemcpy(X, h->X, (size_t)row0 * h->d * sizeof(float), hipMemcpyDeviceToDevice));
    }
    AMDR_HIP(hipMemcpy(X + (size_t)row0 * h->d, X_host, (size_t)n_add * h->d * sizeof(float), hipMemcpyHostToDevice));
    if (grown.X) grown.commit(h, cap);
  }
  h->n = n_new;
  first_pass_forget(h);
  if (h->hi_copy_pending && hipEventSynchronize(h->hi_ev) == hipSuccess) {
    h->hi_copy_pending = false;
    for (int i = 0; i < 3; ++i) h->hi_seen[i] = h->hi_host[i];
  }
  h->lvl_f0 = h->hi_seen[1];
  h->lvl_p0 = (int64_t)h->hi_seen[2];
  int rc = update_stats(h, row0, n_add);
  // a handle with an fp16 image keeps it current: the new rows, or all of it when the scale changed or it has no room
  if (rc == AMDR_OK && h->img) {
    if (h->fp16.large_scan_ok())
      rc = image_sync(h, row0);
    else
      image_drop(h);  // (no first pass is left to read it)
  }
  return rc;
}

// Remove rows.  Everything that can run out of memory or be refused — the device copy of the list, the new matrix, the
// compaction kernel (rows_compact.hip) — happens beside the old matrix; the staged matrix takes its place only after the
// device has finished.  Then what create() does on the new matrix: the statistics from zero, and a present image made again.
int amdr_dense_remove(amdr_dense_t* h, const int64_t* remove_ids, int64_t n_remove) {
  static const char* const who = "dense_remove";
  AMDR_REQUIRE(h != nullptr, "dense_remove: null handle");
  AMDR_REQUIRE(h->owns, "dense_remove: handle wraps caller-owned memory");
  AMDR_REQUIRE(n_remove >= 0, "dense_remove: n_remove=%lld", (long long)n_remove);
  if (n_remove == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  const int bad = rc_validate(remove_ids, n_remove, h->n);
  AMDR_REQUIRE(bad == kRcOk, "dense_remove: %s", rc_error_text(bad));
  AMDR_HIP(hipSetDevice(h->device));
  const int64_t n_new = h->n - n_remove;
  hipStream_t st = h->stream;
  KernelSpans timer(1);  // the compaction kernel (amdr_dense_remove_kernel_ms)
  {
    CallScratch tmp;
    DenseStagedMatrix nx;  // (stays empty when no row is left)
    if (n_new > 0) {
      long long* rm;
      AMDR_TRY(tmp.alloc(&rm, (size_t)n_remove, who));
      AMDR_TRY(dev_alloc(&nx.X, (size_t)n_new * h->d, who));
      AMDR_HIP(hipMemcpyAsync(rm, remove_ids, (size_t)n_remove * sizeof(long long), hipMemcpyHostToDevice, st));
      AMDR_TRY(timer.begin(0, st));
      AMDR_TRY(rows_compact_launch(h->X, (long long)n_new, (long)h->d * (long)sizeof(float), rm, (long)n_remove, nx.X, st));
      AMDR_TRY(timer.end(0, st));
      AMDR_HIP(hipStreamSynchronize(st));
    }
    first_pass_start_over(h);
    nx.commit(h, n_new);
    h->n = n_new;
  }
  h->remove_kernel_ms = n_new > 0 ? timer.ms() : 0.0;  // (emptying the index runs no kernel)
  int rc = update_stats(h, 0, n_new);
  // a handle with an fp16 image keeps one: of the compacted matrix, whose rows sit in other 32-row tiles now
  if (h->img) {
    image_drop(h);  // (a new allocation, sized like the new matrix's own; none for an empty index or unusable statistics)
    if (rc == AMDR_OK && n_new > 0 && h->fp16.large_scan_ok()) rc = image_sync(h, 0);
  }
  return rc;
}

int amdr_dense_remove_kernel_ms(amdr_dense_t* h, double* ms) {
  AMDR_REQUIRE(h && ms, "dense_remove_kernel_ms: null");
  std::lock_guard<std::mutex> g(h->mu);
  *ms = h->remove_kernel_ms;
  return AMDR_OK;
}

// Replace rows in place, in two phases.  Everything that can run out of memory or be refused — the staged rows and ids,
// their copies, the launcher's checks — has happened and has been waited for before the scatter kernel (rows_compact.hip)
// is enqueued; until then the matrix is untouched.  From then on the handle describes the edited matrix whatever is
// reported: what remove does after its swap, the statistics from zero, and a present image brought up to the matrix from
// the first touched 32-row tile on (image_sync converts all of it when the scale changed).
int amdr_dense_replace(amdr_dense_t* h, const int64_t* replace_ids, const float* X_host, int64_t n_rep) {
  static const char* const who = "dense_replace";
  AMDR_REQUIRE(h != nullptr, "dense_replace: null handle");
  AMDR_REQUIRE(h->owns, "dense_replace: handle wraps caller-owned memory");
  AMDR_REQUIRE(n_rep >= 0, "dense_replace: n_rep=%lld", (long long)n_rep);
  if (n_rep == 0) return AMDR_OK;
  AMDR_REQUIRE(X_host != nullptr, "dense_replace: X is null");
  std::lock_guard<std::mutex> g(h->mu);
  const int bad = rc_validate(replace_ids, n_rep, h->n);
  AMDR_REQUIRE(bad == kRcOk, "dense_replace: %s", rs_error_text(bad));
  AMDR_HIP(hipSetDevice(h->device));
  const size_t row_bytes = (size_t)h->d * sizeof(float);
  hipStream_t st = h->stream;
  CallScratch tmp;
  float* rows;
  long long* ids;
  AMDR_TRY(tmp.alloc(&ids, (size_t)n_rep, who));
  AMDR_TRY(tmp.alloc(&rows, (size_t)n_rep * h->d, who));
  AMDR_HIP(hipMemcpyAsync(ids, replace_ids, (size_t)n_rep * sizeof(long long), hipMemcpyHostToDevice, st));
  AMDR_HIP(hipMemcpyAsync(rows, X_host, (size_t)n_rep * row_bytes, hipMemcpyHostToDevice, st));
  KernelSpans timer(1);  // the scatter kernel (amdr_dense_replace_kernel_ms)
  AMDR_HIP(hipStreamSynchronize(st));  // the staged copies are whole; the matrix is still the old one
  AMDR_TRY(timer.begin(0, st));
  // (a refusal enqueues nothing: the launcher checks its arguments before it launches)
  AMDR_TRY(rows_scatter_launch(rows, (long long)n_rep, (long)row_bytes, ids, h->X, st));
  // from here on the matrix is the edited one; a device error below is reported, and the handle describes that matrix
  int late = timer.end(0, st);
  const hipError_t e = hipStreamSynchronize(st);
  if (!late && e != hipSuccess) late = fail(AMDR_EHIP, "dense_replace: %s", hipGetErrorString(e));
  first_pass_start_over(h);
  h->replace_kernel_ms = late ? -1.0 : timer.ms();
  int rc = update_stats(h, 0, h->n);
  if (h->img) {
    if (rc == AMDR_OK && !late && h->fp16.large_scan_ok())
      rc = image_sync(h, replace_ids[0] / kHiTileRows * kHiTileRows);
    else
      image_drop(h);  // (no first pass is left to read it)
  }
  return rc ? rc : late;
}

int amdr_dense_replace_kernel_ms(amdr_dense_t* h, double* ms) {
  AMDR_REQUIRE(h && ms, "dense_replace_kernel_ms: null");
  std::lock_guard<std::mutex> g(h->mu);
  *ms = h->replace_kernel_ms;
  return AMDR_OK;
}

int amdr_dense_image_build(amdr_dense_t* h) {
  AMDR_REQUIRE(h != nullptr, "dense_image_build: null handle");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  AMDR_REQUIRE(dense_hi_supported(h->d), "dense_image_build: the fp16 first pass does not support d=%d", h->d);
  AMDR_REQUIRE(h->n > 0, "dense_image_build: empty index");
  AMDR_REQUIRE(h->fp16.large_scan_ok(), "dense_image_build: the matrix's statistics are not finite");
  if (h->img && h->img_rows == h->n && h->img_scale == h->fp16.x_scale) return AMDR_OK;
  return image_sync(h, 0);
}

int amdr_dense_image_drop(amdr_dense_t* h) {
  AMDR_REQUIRE(h != nullptr, "dense_image_drop: null handle");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  image_drop(h);
  return AMDR_OK;
}

int amdr_dense_image_info(amdr_dense_t* h, int64_t* out4) {
  AMDR_REQUIRE(h && out4, "dense_image_info: null");
  std::lock_guard<std::mutex> g(h->mu);
  out4[0] = h->img ? 1 : 0;
  out4[1] = h->img ? (int64_t)hi_image_bytes((long)h->img_cap_rows, h->d) : 0;
  out4[2] = h->img ? h->img_rows : 0;
  out4[3] = h->img ? 1 - pow2_exp(h->img_scale) : 0;  // img_scale = 2^-e = 0.5 * 2^(1 - e)
  return AMDR_OK;
}

int amdr_dense_ntotal(const amdr_dense_t* h, int64_t* n) {
  AMDR_REQUIRE(h && n, "dense_ntotal: null");
  *n = h->n;
  return AMDR_OK;
}
int amdr_dense_dim(const amdr_dense_t* h, int32_t* d) {
  AMDR_REQUIRE(h && d, "dense_dim: null");
  *d = h->d;
  return AMDR_OK;
}

int amdr_dense_reserve(amdr_dense_t* h, int32_t nq_max, int32_t k_max) {
  AMDR_REQUIRE(h != nullptr, "dense_reserve: null handle");
  AMDR_REQUIRE(nq_max >= 1 && k_max >= 1 && k_max <= AMDR_MAX_K, "dense_reserve: bad sizes");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  const DensePins pins = read_pins();
  int rc = ensure_need(h, 0, reserve_need(h, pins, nq_max, k_max));
  if (rc) return rc;
  if ((rc = side_init(h))) return rc;
  if ((rc = h->qbuf.ensure((size_t)nq_max * h->d * sizeof(float)))) return rc;
  if ((rc = h->sbuf.ensure((size_t)nq_max * k_max * sizeof(float)))) return rc;
  if (small_hi_shape(h, pins, nq_max, k_max < 12 ? k_max : 12, 0))  // (so that a later capture finds the two-pass form's buffers)
    (void)small_hi_ready(h, batched_chunk(h, nq_max), nullptr);
  return h->ibuf.ensure((size_t)nq_max * k_max * sizeof(int64_t));
}

int amdr_dense_search_device(amdr_dense_t* h, const float* Q_dev, int32_t nq, int32_t k, float* scores_dev,
                             int64_t* ids_dev, void* stream) {
  int rc = check_search_args(h, Q_dev, nq, k, scores_dev, ids_dev);
  if (rc) return rc;
  if (nq == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  return run_search(h, 0, Q_dev, nq, k, scores_dev, ids_dev, (hipStream_t)stream);
}

int amdr_dense_search_fuse_device(amdr_dense_t* h, const float* Q_dev, int32_t nq, int32_t k,
                                  const amdr_fuse_params_t* p, const int64_t* dense_row2uid, const int64_t* bm25_ids,
                                  const double* bm25_scores, int32_t kb, const int64_t* bm25_row2uid,
                                  float* dense_scores_dev, int64_t* dense_ids_dev, int64_t* out_ids, double* out_vals,
                                  int32_t* out_mask, int32_t* out_count, void* stream) {
  int rc = check_search_args(h, Q_dev, nq, k, dense_scores_dev, dense_ids_dev);
  if (rc) return rc;
  AMDR_REQUIRE(p != nullptr, "dense_search_fuse: null params");
  AMDR_REQUIRE(p->method >= 0 && p->method <= AMDR_FUSE_WEIGHTED_SUM, "dense_search_fuse: method=%d", p->method);
  AMDR_REQUIRE(kb >= 0 && kb <= AMDR_MAX_K && (kb == 0 || (bm25_ids && bm25_scores)), "dense_search_fuse: bad BM25 lists");
  AMDR_REQUIRE(nq == 0 || (out_ids && out_vals && out_mask && out_count), "dense_search_fuse: null output");
  if (nq == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  FuseTail tail{p, dense_row2uid, bm25_ids, bm25_scores, kb, bm25_row2uid, out_ids, out_vals, out_mask, out_count};
  return run_search(h, 0, Q_dev, nq, k, dense_scores_dev, dense_ids_dev, (hipStream_t)stream, &tail);
}

int amdr_hybrid_batch_device(amdr_dense_t* h, amdr_bm25_t* bm25, const float* Q_dev, const int32_t* q_terms_dev,
                             const int64_t* q_ptr_dev, int32_t nq, int32_t kd, int32_t kb, const amdr_fuse_params_t* p,
                             const int64_t* dense_row2uid, const int64_t* bm25_row2uid, float* dense_scores_dev,
                             int64_t* dense_ids_dev, double* bm25_scores_dev, int64_t* bm25_ids_dev, int64_t* out_ids,
                             double* out_vals, int32_t* out_mask, int32_t* out_count, void* stream) {
  AMDR_REQUIRE(h && bm25, "hybrid_batch: null index handle");
  AMDR_REQUIRE(p != nullptr, "hybrid_batch: null params");
  AMDR_REQUIRE(p->method >= 0 && p->method <= AMDR_FUSE_WEIGHTED_SUM, "hybrid_batch: method=%d", p->method);
  AMDR_REQUIRE(nq >= 0 && kd >= 1 && kd <= AMDR_MAX_K && kb >= 1 && kb <= AMDR_MAX_K, "hybrid_batch: bad sizes");
  if (nq == 0) return AMDR_OK;
  AMDR_REQUIRE(Q_dev && q_ptr_dev, "hybrid_batch: null query buffers");
  AMDR_REQUIRE(dense_scores_dev && dense_ids_dev && bm25_scores_dev && bm25_ids_dev, "hybrid_batch: null channel lists");
  AMDR_REQUIRE(out_ids && out_vals && out_mask && out_count, "hybrid_batch: null output");
  int rc;
  {
    std::lock_guard<std::mutex> g(h->mu);
    AMDR_HIP(hipSetDevice(h->device));
    const DensePins pins = read_pins();
    const HybridBatch a{bm25, Q_dev, q_terms_dev, q_ptr_dev, nq, kd, kb, dense_scores_dev, dense_ids_dev, bm25_scores_dev, bm25_ids_dev};
    const FuseTail tail{p, dense_row2uid, bm25_ids_dev, bm25_scores_dev, kb, bm25_row2uid, out_ids, out_vals, out_mask, out_count};
    Route r;
    DenseMfmaPlan plan;
    if (hybrid_batch_applies(h, pins, a, tail, (hipStream_t)stream, &r, &plan)) {
      if ((rc = ensure_need(h, 0, call_need(h, r, nq, kd)))) return rc;
      return hybrid_batch_overlapped(h, a, tail, plan, (hipStream_t)stream);
    }
  }
  if ((rc = amdr_bm25_search_device(bm25, q_terms_dev, q_ptr_dev, nq, kb, bm25_scores_dev, bm25_ids_dev, stream))) return rc;
  return amdr_dense_search_fuse_device(h, Q_dev, nq, kd, p, dense_row2uid, bm25_ids_dev, bm25_scores_dev, kb, bm25_row2uid,
                                       dense_scores_dev, dense_ids_dev, out_ids, out_vals, out_mask, out_count, stream);
}

int amdr_dense_search(amdr_dense_t* h, const float* Q_host, int32_t nq, int32_t k, float* scores_host,
                      int64_t* ids_host) {
  int rc = check_search_args(h, Q_host, nq, k, scores_host, ids_host);
  if (rc) return rc;
  if (nq == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  if ((rc = h->qbuf.ensure((size_t)nq * h->d * sizeof(float)))) return rc;
  if ((rc = h->sbuf.ensure((size_t)nq * k * sizeof(float)))) return rc;
  if ((rc = h->ibuf.ensure((size_t)nq * k * sizeof(int64_t)))) return rc;
  AMDR_HIP(hipMemcpyAsync(h->qbuf.p, Q_host, (size_t)nq * h->d * sizeof(float), hipMemcpyHostToDevice, h->stream));
  rc = run_search(h, 1, h->qbuf.as<float>(), nq, k, h->sbuf.as<float>(), h->ibuf.as<int64_t>(), h->stream);
  if (rc) return rc;
  AMDR_HIP(hipMemcpyAsync(scores_host, h->sbuf.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipMemcpyAsync(ids_host, h->ibuf.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipStreamSynchronize(h->stream));
  return AMDR_OK;
}

int amdr_dense_score_rows(amdr_dense_t* h, const float* Q_host, int32_t nq, const int64_t* rows_host, int32_t m,
                          float* scores_host) {
  AMDR_REQUIRE(h != nullptr, "dense_score_rows: null handle");
  AMDR_REQUIRE(nq >= 0 && m >= 0, "dense_score_rows: bad sizes");
  if (nq == 0 || m == 0) return AMDR_OK;
  AMDR_REQUIRE(Q_host && rows_host && scores_host, "dense_score_rows: null buffer");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  int rc;
  const size_t cnt = (size_t)nq * m;
  if ((rc = h->qbuf.ensure((size_t)nq * h->d * sizeof(float)))) return rc;
  if ((rc = h->sbuf.ensure(cnt * sizeof(float)))) return rc;
  if ((rc = h->ibuf.ensure(cnt * sizeof(int64_t)))) return rc;
  AMDR_HIP(hipMemcpyAsync(h->qbuf.p, Q_host, (size_t)nq * h->d * sizeof(float), hipMemcpyHostToDevice, h->stream));
  AMDR_HIP(hipMemcpyAsync(h->ibuf.p, rows_host, cnt * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(dense_score_rows_kernel, dim3(ceil_div((long)cnt, kWaves)), dim3(256), 0, h->stream, h->X,
                     (long)h->n, h->d, h->qbuf.as<float>(), nq, h->ibuf.as<long long>(), m, h->sbuf.as<float>());
  AMDR_HIP(hipGetLastError());
  AMDR_HIP(hipMemcpyAsync(scores_host, h->sbuf.p, cnt * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipStreamSynchronize(h->stream));
  return AMDR_OK;
}

int amdr_dense_read_rows(const amdr_dense_t* h, int64_t row0, int64_t nrows, float* out_host) {
  AMDR_REQUIRE(h && out_host, "dense_read_rows: null");
  AMDR_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= h->n, "dense_read_rows: range outside [0,%lld)",
               (long long)h->n);
  AMDR_HIP(hipSetDevice(h->device));
  if (nrows)
    AMDR_HIP(hipMemcpy(out_host, h->X + (size_t)row0 * h->d, (size_t)nrows * h->d * sizeof(float),
                       hipMemcpyDeviceToHost));
  return AMDR_OK;
}

int amdr_dense_workspace_plan(int64_t n, int32_t d, int32_t nq_max, int32_t k_max, int32_t nq, int32_t k, int64_t* out6) {
  AMDR_REQUIRE(out6 != nullptr, "dense_workspace_plan: null");
  AMDR_REQUIRE(n >= 1 && n < (1ll << 32) && d >= 4 && d <= AMDR_MAX_DIM && d % 4 == 0, "dense_workspace_plan: bad shape");
  AMDR_REQUIRE(nq_max >= 1 && k_max >= 1 && k_max <= AMDR_MAX_K && nq >= 1 && k >= 1 && k <= AMDR_MAX_K,
               "dense_workspace_plan: bad sizes");
  amdr_dense h;  // shape only: no device is touched
  h.n = n;
  h.d = d;
  h.fp16.finite = dense_hi_supported(d);  // shape only: the statistics of a real matrix can only take the fp16 first pass away
  const DensePins pins = read_pins();
  const Need res = reserve_need(&h, pins, nq_max, k_max), used = call_need(&h, dense_route(&h, pins, nq, k), nq, k);
  out6[0] = (int64_t)res.smat, out6[1] = (int64_t)res.part, out6[2] = (int64_t)res.aux;
  out6[3] = (int64_t)used.smat, out6[4] = (int64_t)used.part, out6[5] = (int64_t)used.aux;
  return AMDR_OK;
}

int amdr_dense_plan_info(const amdr_dense_t* h, int32_t nq, int32_t k, char* buf, int32_t buf_len) {
  AMDR_REQUIRE(h && buf && buf_len > 0, "dense_plan_info: null");
  AMDR_REQUIRE(nq >= 1 && k >= 1 && k <= AMDR_MAX_K, "dense_plan_info: bad sizes");
  const DensePins pins = read_pins();
  const Route r = dense_route(h, pins, nq, k);
  const int m = r.chunk;
  if (h->n <= 0) {
    snprintf(buf, buf_len, "empty index");
  } else if (r.form == Form::Hi) {
    TwoLevelLayout p;
    two_level_layout(h, m, k, r.kc, true, &p);
    snprintf(buf, buf_len,
             "%s fp16 first pass queries_per_launch=%d scans_per_launch=%d (%d per scan, one tail): per-query lists of the "
             "approximate tile maxima above a sampled threshold (every %ld-th tile, width level %d) -> top-%d + rounding-bound "
             "check + exact re-scoring of each query's tiles at or above its cut (<= %d each) + top-k: 4 launches behind the "
             "scan(s), the exact first pass behind a device flag in 2",
             hi_image_of(h, pins) ? "dense_hi_image_tilemax_kernel (resident fp16 image)" : "dense_hi_tilemax_kernel", m, p.qtiles,
             m < dense_hi_max_queries(h->d) ? m : dense_hi_max_queries(h->d),
             dense_hi2_sample_stride((long)h->n, p.qtiles), r.hi_level, r.kc, r.kc);
  } else if (r.form == Form::TwoLevel) {
    TwoLevelLayout t;
    two_level_layout(h, m, k, k, false, &t);
    snprintf(buf, buf_len,
             "dense_mfma_scores_kernel tile-maxima grid=%dx%d queries_per_launch=%d two-level: top-%d of %ld tile maxima "
             "+ <= %d tiles per query re-scored + top-k%s",
             t.scan.grid_x, t.scan.grid_y, m, k, t.tiles, k,
             r.hi ? " (fp16 first pass given up: too many unresolved queries)" : "");
  } else if (r.form != Form::Scan) {
    DenseMfmaPlan p;
    dense_mfma_plan((long)h->n, h->d, m, k, &p);
    const PassForm f = batched_pass_form(h, pins, r, p, m, k, nullptr);
    const char* tail = dense_topk_pair_applies(p, (long)h->n, m, k) ? "scores_pair_topk_kernel"
                       : p.slabs == 1                              ? "scores_slab_topk_kernel"
                                                                   : "scores_slab_topk_kernel + merge_parts_kernel";
    if (f.small_hi && !h->small_failed) {
      snprintf(buf, buf_len,
               "dsh_scores_kernel fp16 first pass queries_per_launch=%d (dsh_split_queries_kernel + v_mfma_f32_32x32x16_f16 on "
               "fp16 roundings of both operands, proven per-query bound) + dense_hi_select_fuse_kernel (rows inside 2 eps of the "
               "k-th best re-scored exactly, top-k, fusion); exact form: dense_panel_scores_kernel; amdr_hybrid_batch_device: %s",
               m, hybrid_batch_on() ? "BM25 on a side stream beside the second dense pass, then fuse_packed_kernel"
                                    : "the serial calls (AMDR_HYBRID_BATCH=0)");
    } else if (f.scores == PassForm::RowWaves) {
      snprintf(buf, buf_len, "dense_all_scores_kernel (one wave per query x row) + %s", tail);
    } else if (f.scores == PassForm::Panel) {
      DensePanelPlan pp;
      dense_panel_plan((long)h->n, h->d, m, &pp);
      snprintf(buf, buf_len, "dense_panel_scores_kernel nb=%d parts=%d blocks=%d queries_per_launch=%d + %s", pp.nb,
               pp.parts, pp.m_tiles * pp.parts, m, tail);
    } else {
      snprintf(buf, buf_len, "dense_mfma_scores_kernel query-tiles-in-LDS grid=%dx%d queries_per_launch=%d + %s",
               p.grid_x, p.grid_y, m, tail);
    }
  } else {
    ScanPlan p;
    make_plan(h->n, h->d, m, k, &p);  // (a pass: the whole batch up to kGridYMax queries)
    snprintf(buf, buf_len, "dense_scan_topk_kernel<NQ=%d> grid=%dx%d%s", p.nq_per_block, p.grid_x, p.grid_y,
             p.grid_x == 1 ? "" : " + merge_parts_kernel");
  }
  return AMDR_OK;
}

int amdr_dense_hi_counters(amdr_dense_t* h, int64_t* out6) {
  AMDR_REQUIRE(h && out6, "dense_hi_counters: null");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  out6[0] = h->hi_queries;
  out6[1] = out6[5] = 0;
  if (h->stats.p) {
    unsigned int c[3] = {0, 0, 0};
    AMDR_HIP(hipDeviceSynchronize());  // the counters are bumped by kernels on the callers' streams
    AMDR_HIP(hipMemcpy(c, h->stats.as<unsigned int>() + 2, sizeof(c), hipMemcpyDeviceToHost));
    out6[1] = (int64_t)c[0];
    out6[5] = (int64_t)c[1];
  }
  const DensePins pins = read_pins();
  out6[2] = pins.hi_level >= 0 ? pins.hi_level : h->hi_level;
  out6[3] = h->fp16.large_scan_ok() && !h->hi_off ? 1 : 0;
  out6[4] = h->hi_passes;
  return AMDR_OK;
}

int amdr_dense_profile_begin(amdr_dense_t* h, int32_t max_launches) {
  AMDR_REQUIRE(h != nullptr && max_launches >= 1 && max_launches <= (1 << 16), "dense_profile_begin: bad arguments");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  while (h->prof_ev.size() < (size_t)max_launches * 2) {
    hipEvent_t e;
    AMDR_HIP(hipEventCreate(&e));
    h->prof_ev.push_back(e);
  }
  h->prof_used = 0;
  h->prof_on = true;
  return AMDR_OK;
}

int amdr_dense_profile_end(amdr_dense_t* h, double* total_ms, int32_t* launches) {
  AMDR_REQUIRE(h && total_ms && launches, "dense_profile_end: null");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  h->prof_on = false;
  double tot = 0;
  for (int i = 0; i + 1 < h->prof_used; i += 2) {
    float ms = 0;
    AMDR_HIP(hipEventSynchronize(h->prof_ev[i + 1]));
    AMDR_HIP(hipEventElapsedTime(&ms, h->prof_ev[i], h->prof_ev[i + 1]));
    tot += ms;
  }
  *total_ms = tot;
  *launches = h->prof_used / 2;
  h->prof_used = 0;
  return AMDR_OK;
}

int amdr_dense_two_pass_fallbacks(amdr_dense_t* h, int64_t* out) {
  AMDR_REQUIRE(h && out, "dense_two_pass_fallbacks: null");
  *out = 0;
  std::lock_guard<std::mutex> g(h->mu);
  if (!h->small_fb.p) return AMDR_OK;
  AMDR_HIP(hipSetDevice(h->device));
  unsigned int v = 0;
  AMDR_HIP(hipMemcpy(&v, h->small_fb.p, sizeof(v), hipMemcpyDeviceToHost));  // (synchronises with the device)
  *out = (int64_t)v;
  return AMDR_OK;
}

int amdr_dense_destroy(amdr_dense_t* h) {
  if (!h) return AMDR_OK;
  (void)hipSetDevice(h->device);
  for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
  if (h->stream) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamDestroy(h->stream);
  }
  if (h->side) {
    (void)hipStreamSynchronize(h->side);
    (void)hipStreamDestroy(h->side);
  }
  for (hipEvent_t e : h->side_ev)
    if (e) (void)hipEventDestroy(e);
  if (h->owns && h->X) (void)hipFree(h->X);
  image_drop(h);
  for (int w = 0; w < 2; ++w) {
    h->part[w].release();
    h->smat[w].release();
    h->aux[w].release();
  }
  h->qbuf.release();
  h->sbuf.release();
  h->ibuf.release();
  h->stats.release();
  if (h->small) (void)amdr_dense_small_destroy(h->small);
  h->small_eps.release();
  h->small_fb.release();
  if (h->hi_host) (void)hipHostFree(h->hi_host);
  if (h->hi_ev) (void)hipEventDestroy(h->hi_ev);
  delete h;
  return AMDR_OK;
}

}  // extern "C"

// Device code of the fusion that more than one translation unit runs: the per-candidate arithmetic (fuse_eval) and the
// packed form's body (fuse_packed_body), which fuse.hip's kernels and the dense tails of dense_tail.hip both call.  Every
// expression is written in the reference's operand order; both translation units are compiled with -ffp-contract=off so
// results are bit-identical to the Python float arithmetic.
#pragma once
#include "common.hpp"
#include "topk.hpp"

#include <cmath>

namespace amdr {

// all-lanes reductions on DPP / permlane-swap exchanges (topk.hpp), not ds_bpermute
__device__ __forceinline__ double wave_min(double v) { return wave_allmin_f64(v); }
__device__ __forceinline__ double wave_max(double v) { return wave_allmax_f64(v); }
__device__ __forceinline__ void lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

struct ChanIn {
  const long long* ids;  // [nq, k]
  const void* scores;    // float or double [nq, k]
  const long long* row2uid;
  int k;
  int is_f64;
  __host__ __device__ static ChanIn none() { return ChanIn{nullptr, nullptr, nullptr, 0, 0}; }  // a switched-off channel
};

__device__ __forceinline__ double chan_score(const ChanIn& c, int qi, int j) {
  size_t off = (size_t)qi * c.k + j;
  return c.is_f64 ? ((const double*)c.scores)[off] : (double)((const float*)c.scores)[off];
}
__device__ __forceinline__ long long chan_uid(const ChanIn& c, int qi, int j) {
  long long id = c.ids[(size_t)qi * c.k + j];
  if (id >= 0 && c.row2uid) id = c.row2uid[id];
  return id;
}

// Everything _fuse reports for one candidate (hybrid_retriever.py:389-551), operand for operand
// in the reference's order; shared by the one-query-per-wave kernel and the packed one.
struct FuseCtx {
  double rmn, rmx;  // min / max of the RRF totals over the union
  bool rdeg, wrrf;
  double w[3], lo[3], hi[3];  // channel weight, min and max of the channel's scores
};
template <class ScoreAt>
__device__ __forceinline__ void fuse_eval(const amdr_fuse_params_t& P, const FuseCtx& X, double t, const int (&pos)[3],
                                          ScoreAt&& score_at, double (&val)[AMDR_FUSE_NVALS], int& mk) {
  const double rrf_norm = X.rdeg ? 0.0 : (t - X.rmn) / (X.rmx - X.rmn);
  double nrm[3], raw[3], wt[3];
  mk = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int p = pos[c];
    nrm[c] = 0.0;
    raw[c] = 0.0;
    if (p >= 0) {
      mk |= (1 << c);
      const double s = score_at(c, p);
      nrm[c] = (X.hi[c] - X.lo[c] < 1e-12) ? 0.0 : (s - X.lo[c]) / (X.hi[c] - X.lo[c]);
      const double wc = X.wrrf ? X.w[c] : 1.0;
      raw[c] = wc * (1.0 / (double)(P.rrf_k + p + 1));
    }
    wt[c] = X.w[c] * nrm[c];
  }
  const double wsum = (wt[0] + wt[1]) + wt[2];
  double score, con[3] = {0.0, 0.0, 0.0};
  if (P.method == AMDR_FUSE_WEIGHTED_SUM) {
    score = wsum;
#pragma unroll
    for (int c = 0; c < 3; ++c) con[c] = wt[c];
  } else if (P.method == AMDR_FUSE_RRF || P.method == AMDR_FUSE_WRRF) {
    score = rrf_norm;
    const double mass = score;
    if (!(mass <= 0.0 || t <= 1e-18)) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (pos[c] >= 0) con[c] = mass * raw[c] / t;
    }
  } else {
    score = P.alpha * rrf_norm + (1.0 - P.alpha) * wsum;
#pragma unroll
    for (int c = 0; c < 3; ++c) con[c] = 0.0 + (1.0 - P.alpha) * wt[c];
    const double mass = P.alpha * rrf_norm;
    if (!(mass <= 0.0 || t <= 1e-18)) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (pos[c] >= 0) con[c] = con[c] + mass * raw[c] / t;
    }
  }
  val[AMDR_FV_SCORE] = score;
  val[AMDR_FV_RRF_NORM] = rrf_norm;
  val[AMDR_FV_WSUM] = wsum;
  val[AMDR_FV_NORM_DENSE] = nrm[0];
  val[AMDR_FV_NORM_BM25] = nrm[1];
  val[AMDR_FV_NORM_COLBERT] = nrm[2];
  val[AMDR_FV_CONTRIB_DENSE] = con[0];
  val[AMDR_FV_CONTRIB_BM25] = con[1];
  val[AMDR_FV_CONTRIB_COLBERT] = con[2];
}

// Packed form for the serving shape: when all candidates of a query fit in W lanes (max_out
// <= W; top-10 of two or three channels -> W = 32), a wave fuses 64 / W queries side by side,
// one candidate per lane.  Same arithmetic as fuse_kernel (fuse_eval), same outputs; the
// reductions run inside the W-lane group and the ballots are cut to the group's bits.  The
// kernel is bound by vector instructions issued per wave (fp64 divisions), not by data, so
// halving the waves halves its time.
// Entries a caller already holds in registers (lane sl = list position sl of its query): the fused dense top-k +
// fusion kernel hands over the dense list straight from its selector and the BM25 list it requested up front.
struct FusePre {
  bool have[3];
  long long id[3];  // raw channel id (-1 = padding), before row2uid
  double s[3];
  // What a dense tail hands the packed fusion: the dense entry follows from its selector (dense()), the BM25 entry of
  // list position sl is requested HERE — the caller places this where the load should be issued.
  __device__ __forceinline__ void dense_bm25(const ChanIn& c1, int q, int sl, bool live) {
    have[0] = have[1] = true;
    have[2] = false;
    id[1] = -1;
    s[1] = 0.0;
    if (live && sl < c1.k) {
      id[1] = c1.ids[(size_t)q * c1.k + sl];
      s[1] = chan_score(c1, q, sl);
    }
  }
  __device__ __forceinline__ void dense(const C32& c, bool valid) {  // the dense list straight from a selector's lanes
    id[0] = valid ? c.id() : -1ll;
    s[0] = valid ? (double)c.score() : 0.0;
  }
  __device__ __forceinline__ void bm25(const C64& c, bool valid) {  // the BM25 list (ord64 keys) likewise
    id[1] = valid ? c.idv : -1ll;
    s[1] = valid ? unord64(c.key) : 0.0;
  }
};
template <int W, bool PRE>
__device__ __forceinline__ void fuse_packed_body(const amdr_fuse_params_t& P, const ChanIn& c0, const ChanIn& c1,
                                                 const ChanIn& c2, int nq, int max_out, long long* __restrict__ out_ids,
                                                 double* __restrict__ out_vals, int* __restrict__ out_mask,
                                                 int* __restrict__ out_count, const FusePre& pre, int qbase) {
  constexpr int G = 64 / W;  // queries per wave
  __shared__ long long s_uid[G][W];
  __shared__ double s_sc[G][W];
  __shared__ double s_chs[G][3][W];  // channel scores by list position
  __shared__ int s_pos[G][3][W];
  const int lane = threadIdx.x, seg = lane / W, sl = lane % W;
  const int qi = qbase + seg;  // (the packed kernels: blockIdx.x * G)
  const bool live = qi < nq;
  const ChanIn ch[3] = {c0, c1, c2};
  const double w[3] = {P.w_dense, P.w_bm25, P.w_colbert};
  const unsigned long long seg_bits = (W == 64) ? ~0ull : (((1ull << (W & 63)) - 1ull) << (seg * W));
  long long* uid = s_uid[seg];
  double* sc = s_sc[seg];

  // ---- per channel: valid prefix length, min / max, ids and scores -----------------------
  // A switched-off channel (k = 0, a kernel argument) is skipped as a whole; the counts are ballots, not lane
  // sums; and min / max of a channel whose scores arrive in descending order — the contract of
  // include/amdretrieval.h, and what _fuse's stable sort gives — are its first and last valid entries (one
  // neighbour compare + two lane reads instead of two five-step fp64 reductions; a list that is not descending,
  // NaNs included, still takes the reductions).  SQ counters: 857 -> 640 vector instructions per wave (42 % of
  // them were the cross-lane moves of the 64-bit reductions) — for 31.5 -> 30.7 us only: at 857 the kernel was
  // bound by vector issue, at 640 by the lifetime of its waves (two memory round trips, LDS exchanges, stores).
  // Not kept: two or more passes per wave with the next pass's lists prefetched (33.8 / 35.0 us).
  int n[3] = {0, 0, 0};
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  long long my_uid[3] = {-1, -1, -1};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (ch[c].k == 0) continue;
    const int j = sl;
    const bool inr = live && j < ch[c].k;
    long long id = -1;
    double s = 0.0;
    if (PRE && pre.have[c]) {
      if (inr) {
        id = pre.id[c];
        s = pre.s[c];
      }
    } else if (inr) {  // id and score are requested together: one memory round trip, not two
      id = ch[c].ids[(size_t)qi * ch[c].k + j];
      s = chan_score(ch[c], qi, j);
    }
    const bool has = inr && id >= 0;
    if (!has) s = 0.0;
    if (has && ch[c].row2uid) id = ch[c].row2uid[id];
    my_uid[c] = has ? id : -1;
    s_chs[seg][c][sl] = s;
    const unsigned long long hm = __ballot(has) & seg_bits;
    n[c] = __popcll(hm);
    // descending prefix?  valid entries form a prefix; lane sl compares with its right neighbour
    const double nxt = __shfl_down(s, 1);
    const bool in_order = !(has && sl + 1 < n[c]) || s >= nxt;
    const bool prefix = hm == (seg_bits & ((n[c] >= 64 ? ~0ull : ((1ull << n[c]) - 1ull)) << (seg * W)));
    if (__ballot(!in_order || !prefix) == 0ull) {
      const int first = seg * W, last = seg * W + (n[c] > 0 ? n[c] - 1 : 0);
      const double top = __shfl(s, first), bot = __shfl(s, last);
      hi[c] = n[c] > 0 ? top : -(double)INFINITY;
      lo[c] = n[c] > 0 ? bot : (double)INFINITY;
    } else {
      lo[c] = seg_allmin_f64<W>(has ? s : (double)INFINITY);
      hi[c] = seg_allmax_f64<W>(has ? s : -(double)INFINITY);
    }
  }

  // ---- union of ids in first-appearance order ----------------------------------------------
  int U = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (ch[c].k == 0) continue;
    const int U0 = U;
    const bool v = sl < n[c];  // valid entries form a prefix (-1 padding at the tail)
    const long long my = my_uid[c];
    // the union holds an id once: at most one entry matches, so no early exit is needed and the reads of a
    // group of four are independent (the data-dependent loop paid one LDS round trip per entry)
    int f = -1;
    int u_end = 0;  // wave-uniform loop bound: the longest union among the wave's queries
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int ug = __builtin_amdgcn_readlane(U0, g * W);
      u_end = ug > u_end ? ug : u_end;
    }
    for (int u0 = 0; u0 < u_end; u0 += 4) {
      long long e[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) e[i] = uid[(u0 + i) & (W - 1)];
#pragma unroll
      for (int i = 0; i < 4; ++i) f = (u0 + i < U0 && e[i] == my) ? u0 + i : f;
    }
    f = v ? f : -1;
    const bool isnew = v && f < 0;
    const unsigned long long m = __ballot(isnew) & seg_bits;
    const unsigned long long lt = m & ((1ull << lane) - 1ull);
    const int idx = isnew ? U + __popcll(lt) : f;
    if (isnew) {
      uid[idx] = my;
      s_pos[seg][0][idx] = -1;
      s_pos[seg][1][idx] = -1;
      s_pos[seg][2][idx] = -1;
    }
    lds_sync();
    if (v) s_pos[seg][c][idx] = sl;
    U += __popcll(m);
    lds_sync();
  }

  // ---- RRF totals, their min / max -------------------------------------------------------------
  const bool wrrf = (P.method == AMDR_FUSE_WRRF);
  const int u = sl;
  const bool act = u < U;
  int pp[3] = {-1, -1, -1};
  double t = 0.0;
  if (act) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pp[c] = s_pos[seg][c][u];
      if (pp[c] >= 0) {
        const double wc = wrrf ? w[c] : 1.0;
        const double v = wc * (1.0 / (double)(P.rrf_k + pp[c] + 1));
        t = t + v;
      }
    }
  }
  FuseCtx X;
  X.rmn = seg_allmin_f64<W>(act ? t : (double)INFINITY);
  X.rmx = seg_allmax_f64<W>(act ? t : -(double)INFINITY);
  X.rdeg = (X.rmx - X.rmn < 1e-12);
  X.wrrf = wrrf;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    X.w[c] = w[c];
    X.lo[c] = lo[c];
    X.hi[c] = hi[c];
  }

  // ---- score, stable descending rank, filter, scatter --------------------------------------------
  double val[AMDR_FUSE_NVALS];
  int mk = 0;
  if (act) {
    fuse_eval(P, X, t, pp, [&](int c, int p) { return s_chs[seg][c][p]; }, val, mk);
    sc[u] = val[AMDR_FV_SCORE];
  }
  lds_sync();
  int kept = 0;
  const size_t obase = (size_t)qi * max_out;
  if (act) {
    const double s = val[AMDR_FV_SCORE];
    int r = 0;
    for (int v2 = 0; v2 < U; ++v2) {
      const double o = sc[v2];
      r += (o > s) || (o == s && v2 < u);
    }
    if (s >= P.min_final_score) kept = 1;
    out_ids[obase + r] = uid[u];
    out_mask[obase + r] = mk;
#pragma unroll
    for (int x = 0; x < AMDR_FUSE_NVALS; ++x) out_vals[(obase + r) * AMDR_FUSE_NVALS + x] = val[x];
  } else if (live && u < max_out) {  // rows past the union: padding
    out_ids[obase + u] = -1;
    out_mask[obase + u] = 0;
#pragma unroll
    for (int x = 0; x < AMDR_FUSE_NVALS; ++x) out_vals[(obase + u) * AMDR_FUSE_NVALS + x] = 0.0;
  }
  kept = __popcll(__ballot(kept != 0) & seg_bits);
  if (live && sl == 0) out_count[qi] = kept;
}

// Queries [q0, ..) of a FuseTail as the fusion kernels take them: the two channels and the output rows.  dense lists
// null: the kernel holds the dense list in its lanes.
struct FuseTailArgs {
  ChanIn c0, c1;
  int mo;
  long long* ids;
  double* vals;
  int* mask;
  int* count;
};
inline FuseTailArgs fuse_tail_args(const FuseTail& t, int q0, int kd, const float* dense_scores, const int64_t* dense_ids) {
  const int mo = kd + t.kb;
  return FuseTailArgs{ChanIn{(const long long*)dense_ids, dense_scores, (const long long*)t.dense_row2uid, kd, 0},
                      ChanIn{(const long long*)(t.kb ? t.bm25_ids + (size_t)q0 * t.kb : nullptr),
                             t.kb ? (const void*)(t.bm25_scores + (size_t)q0 * t.kb) : nullptr,
                             (const long long*)t.bm25_row2uid, t.kb, 1},
                      mo, (long long*)(t.out_ids + (size_t)q0 * mo), t.out_vals + (size_t)q0 * mo * AMDR_FUSE_NVALS,
                      t.out_mask + (size_t)q0 * mo, t.out_count + q0};
}

}  // namespace amdr

// Scoped search: the top-k of a query's OWN rows in the dense, BM25 and ColBERT channels.
//
// No reference counterpart: the reference ranks the whole corpus and a caller who asks "within Book III" over-fetches and
// filters on the host (legalrag/retrieval/hybrid_retriever.py:282-384 has no scope argument).  Here a scope is a short,
// ascending list of rows of ONE channel's row space and the work is proportional to it: grid = (slabs of a scope, query),
// a block scores its slab's rows with the channel's own device functions — dense_row_dot (dense_dot.hpp), the BM25
// expression in query order (bm25_core.hpp), the split-fp16 pair form (maxsim_core.hpp) — so every score has the bits
// the unscoped channel gives that row, and ranks them with the selector of topk.hpp (score descending, ties -> lower id,
// NaN last, -0.0 as +0.0).  Corpus statistics stay global (idf, avgdl, the MaxSim store's scale).  One slab: the final
// lists are written directly; several: per-slab lists, merged by launch_merge_parts.  No existing kernel, route or
// workspace is touched: the handle below owns the slab lists, one region per channel, so the three calls of a step need
// no ordering among themselves.
// The scoped STEP (dense + BM25 top-k + fusion) of scopes that fit one slab is one launch, scope_hybrid_kernel: a block
// owns a query from its first row to its fused hits and runs the two channels' own pieces below, so it needs no
// workspace, no counters and no ordering between blocks.
#include "common.hpp"
#include "topk.hpp"
#include "topk_merge.hpp"

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <new>

#include "bm25_core.hpp"
#include "dense_dot.hpp"
#include "fuse_core.hpp"
#include "maxsim_core.hpp"

#include "scope_handle.hpp"

using namespace amdr;

namespace {

constexpr int kScWaves = 4;
constexpr int kScSlabMax = 1024;  // rows per block at most (BM25: 8 KiB of fp64 scores in LDS beside the lists)
constexpr size_t kScAlign = 256;
enum { kDense = 0, kBm25 = 1, kMaxsim = 2 };

size_t align_up(size_t b) { return (b + kScAlign - 1) / kScAlign * kScAlign; }

// Rows per block.  Dense: a row is one wave's GEMV step, 64 rows per wave keep a 28-row section in one block and one
// launch.  BM25: a row is one thread's walk over the query's tokens.  MaxSim: a document is 24 matrix instructions per
// 32 tokens, 16 documents per wave.  AMDR_SCOPE_SLAB (read per call, and by reserve / workspace_plan) pins the length
// for all three so that tests reach the multi-slab path at small sizes.
int scope_slab(int chan) {
  const char* e = getenv("AMDR_SCOPE_SLAB");
  if (e && atoi(e) > 0) return atoi(e) < kScSlabMax ? atoi(e) : kScSlabMax;
  return chan == kDense ? 256 : chan == kBm25 ? 1024 : 64;
}
int scope_slabs(int chan, int64_t rows_max) {
  const int64_t s = scope_slab(chan);
  const int64_t n = (rows_max + s - 1) / s;
  return n < 1 ? 1 : (int)n;
}
// bytes of a channel's slab lists: scores [slabs, nq, k] then ids [slabs, nq, k]; a single slab writes the final lists
size_t scope_score_bytes(int chan, int slabs, int nq, int k) {
  return align_up((size_t)slabs * nq * k * (chan == kBm25 ? sizeof(double) : sizeof(float)));
}
size_t scope_region_bytes(int chan, int nq, int k, int64_t rows_max) {
  const int slabs = scope_slabs(chan, rows_max);
  if (slabs <= 1) return 0;
  return scope_score_bytes(chan, slabs, nq, k) + align_up((size_t)slabs * nq * k * sizeof(int64_t));
}

// a block's piece [lo, hi) of the row list: the slab `at` of the scope of query q; empty for a qscope outside
// [0, n_scopes) and for a slab beyond the scope
__device__ __forceinline__ void scope_piece(const long long* __restrict__ scope_ptr, const int* __restrict__ qscope,
                                            int n_scopes, int slab, unsigned at, int q, long& lo, long& hi) {
  lo = hi = 0;
  const int s = qscope[q];
  if (s < 0 || s >= n_scopes) return;
  const long b = scope_ptr[s], e = scope_ptr[s + 1];
  lo = b + (long)at * slab;
  hi = lo + slab < e ? lo + slab : e;
  if (hi < lo) hi = lo;
}

// ---- dense: one wave per scope row (dense_row_dot), lane 63's score into the wave's list ---------------------------------
// The piece [lo, hi) of the row list against query row qr: every wave's list, combined into wave 0's (tk of wave 0 holds
// the block's top-k afterwards).  Called by all four waves; two block barriers (block_combine_topk).
// LDS: TopkLds<C32>(kScWaves, cap)
// This wave takes rows lo + first, lo + first + step, ... (the channel kernel: first = wave, step = 4).
__device__ __forceinline__ void scope_dense_piece(const float* __restrict__ X, long n, int d, const float* __restrict__ qr,
                                                  const long long* __restrict__ rows, long lo, long hi, int first, int step,
                                                  int k, const TopkLds<C32>& L, int wave, int lane, WaveTopK<C32>& tk) {
  tk.init(L.list(wave), L.cap, k);
  for (long i = lo + first; i < hi; i += step) {
    const long r = uniform_i64(rows[i]);
    if (r < 0 || r >= n) continue;  // never dereferenced
    const float acc = dense_row_dot(X + (size_t)r * d, qr, d, lane);
    const float s = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 63));
    tk.push_uniform(C32::make(s, (u32)r), lane);
  }
  tk.finalize(lane);
  block_combine_topk(tk, L, kScWaves, wave, lane);
}

// The three channel kernels write row blockIdx.x * nq + q of (out_scores, out_ids): the slab lists, or — a single slab,
// blockIdx.x = 0 — the final result itself (sc_run hands in the one or the other).
// grid: (x = slabs, y = queries)
__global__ __launch_bounds__(kScWaves * 64) void scope_dense_kernel(
    const float* __restrict__ X, long n, int d, const float* __restrict__ Q, const long long* __restrict__ scope_ptr,
    const long long* __restrict__ rows, const int* __restrict__ qscope, int n_scopes, int slab, int nq, int k, int cap,
    float* __restrict__ out_scores, long long* __restrict__ out_ids) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const TopkLds<C32> L(smem, kScWaves, cap);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.y;
  long lo, hi;
  scope_piece(scope_ptr, qscope, n_scopes, slab, blockIdx.x, q, lo, hi);
  WaveTopK<C32> tk;
  scope_dense_piece(X, n, d, Q + (size_t)q * d, rows, lo, hi, wave, kScWaves, k, L, wave, lane, tk);
  if (wave != 0) return;
  const size_t row = (size_t)blockIdx.x * nq + q;
  topk_store(tk.buf, tk.cnt, k, lane, out_scores + row * k, out_ids + row * k);
}

// ---- BM25: the slab's fp64 scores in LDS, one thread per scope document, tokens in query order ---------------------------
// A document's posting in a term's list is found by binary search (scopes are short next to posting lists); a hit adds
// idf[term] * post_w[p] — a multiply, then an add (this file is built with -ffp-contract=off) — in the order
// bm25_block_query's scatter gives the same document, duplicates counted, unknown terms skipped: the same bits.
// The piece [lo, hi) of the document list for query q, scored and ranked: wave 0's tk holds the block's top-k afterwards.
// Called by all four waves; every barrier is under a block-uniform condition.  ONE_WAVE: called by wave 0 alone for a
// piece of <= 64 documents — in the four-wave form the other three waves have no document of such a piece and only
// keep the barriers company — with wave-level fences for the block barriers and no combine: the same scores, the same
// list, no block barrier.
// LDS (smem): double sc[slab] + TopkLds<C64>(kScWaves, cap) + token table
struct ScBm25 {  // the index side of the BM25 piece (device pointers)
  const long long* term_ptr;
  const int* post_doc;
  const double* post_w;
  const double* idf;
  long n_terms, n_docs;
};
template <bool ONE_WAVE>
__device__ __forceinline__ void scope_bm25_piece(const ScBm25& B, const int* __restrict__ q_terms,
                                                 const long long* __restrict__ q_ptr, int q,
                                                 const long long* __restrict__ rows, long lo, long hi, int slab, int k,
                                                 int cap, unsigned char* smem, WaveTopK<C64>& tk) {
  const long long* __restrict__ term_ptr = B.term_ptr;
  const int* __restrict__ post_doc = B.post_doc;
  const double* __restrict__ post_w = B.post_w;
  const double* __restrict__ idf = B.idf;
  const long n_terms = B.n_terms, n_docs = B.n_docs;
  double* sc = reinterpret_cast<double*>(smem);
  const TopkLds<C64> L(sc + slab, kScWaves, cap);
  long* tk_ps = reinterpret_cast<long*>(L.cnts + kScWaves);  // posting range + idf of up to kBmTok query tokens at a time
  long* tk_pe = tk_ps + kBmTok;
  double* tk_w = reinterpret_cast<double*>(tk_pe + kBmTok);
  int* tk_n = reinterpret_cast<int*>(tk_w + kBmTok);
  constexpr int NT = ONE_WAVE ? 64 : kScWaves * 64;
  constexpr int SYNC = ONE_WAVE ? 1 : kScWaves;  // block_sync<1>: a wave-level fence
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = (int)(hi - lo);
  for (int i = tid; i < m; i += NT) sc[i] = 0.0;
  block_sync<SYNC>();
  if (m > 0) {  // block-uniform; an empty piece reads nothing
    const long t0 = q_ptr[q], t1 = q_ptr[q + 1];
    for (long tb = t0; tb < t1; tb += kBmTok) {
      const int nt_all = (int)((t1 - tb) < kBmTok ? (t1 - tb) : kBmTok);
      if (tid < 64) {
        long ps = 0, pe = 0;
        double w = 0.0;
        if (tid < nt_all) {
          const int term = q_terms[tb + tid];
          if (term >= 0 && term < n_terms) {  // unknown token: skipped
            ps = term_ptr[term];
            pe = term_ptr[term + 1];
            w = idf[term];
          }
        }
        const bool keep = pe > ps;  // kept in query order
        const unsigned long long km = __ballot(keep);
        const unsigned long long below = (tid == 0) ? 0ull : (km & (~0ull >> (64 - tid)));
        if (keep) {
          const int at = __popcll(below);
          tk_ps[at] = ps;
          tk_pe[at] = pe;
          tk_w[at] = w;
        }
        if (tid == 0) *tk_n = __popcll(km);
      }
      block_sync<SYNC>();
      const int nt = *tk_n;
      for (int i = tid; i < m; i += NT) {
        const long doc = rows[lo + i];
        if (doc < 0 || doc >= n_docs) continue;
        double s = sc[i];
        for (int t = 0; t < nt; ++t) {
          const long pe = tk_pe[t];
          const long p = lower_bound_i32(post_doc, tk_ps[t], pe, (int)doc);
          if (p < pe && post_doc[p] == (int)doc) s += tk_w[t] * post_w[p];
        }
        sc[i] = s;
      }
      block_sync<SYNC>();  // the table is rewritten by the next group
    }
  }
  tk.init(L.list(wave), cap, k);
  for (int base = wave * 64; base < m; base += NT) {
    const int i = base + lane;
    const long doc = i < m ? rows[lo + i] : -1;
    const bool v = doc >= 0 && doc < n_docs;  // zero-score documents ARE ranked
    tk.push_lanes(v ? C64::make(sc[i], doc) : C64::pad(), v, lane);
  }
  tk.finalize(lane);
  if (!ONE_WAVE) block_combine_topk(tk, L, kScWaves, wave, lane);
}
__host__ __device__ inline size_t scope_bm25_lds(int slab, int cap) {
  return (size_t)slab * sizeof(double) + TopkLds<C64>::bytes(kScWaves, cap) + 3 * kBmTok * sizeof(long) + 8;
}

// grid: (x = slabs, y = queries)
__global__ __launch_bounds__(kScWaves * 64) void scope_bm25_kernel(ScBm25 B, const int* __restrict__ q_terms,
    const long long* __restrict__ q_ptr, const long long* __restrict__ scope_ptr, const long long* __restrict__ rows,
    const int* __restrict__ qscope, int n_scopes, int slab, int nq, int k, int cap, double* __restrict__ out_scores,
    long long* __restrict__ out_ids) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.y;
  long lo, hi;
  scope_piece(scope_ptr, qscope, n_scopes, slab, blockIdx.x, q, lo, hi);
  WaveTopK<C64> tk;
  scope_bm25_piece<false>(B, q_terms, q_ptr, q, rows, lo, hi, slab, k, cap, smem, tk);
  if (wave != 0) return;
  const size_t row = (size_t)blockIdx.x * nq + q;
  topk_store(tk.buf, tk.cnt, k, lane, out_scores + row * k, out_ids + row * k);
}

// ---- the scoped step in one launch: dense piece, BM25 piece, fusion -----------------------------------------------------
// grid = one block per query, 256 threads, no workspace: both scopes of the query fit one slab of their channel, so the
// block runs the two pieces above one after the other (all four waves each; the same floating-point sequence per row /
// document as the two kernels above, hence the same bits).  Wave 0 writes each finished list to the caller's [nq, kd] /
// [nq, kb] as its piece ends, keeps the dense list in registers across the BM25 piece, takes the BM25 list from LDS and
// fuses with fuse_packed_body, the packed fusion's own code (W = 16 / 32 lanes per query as launch_fuse picks them; lanes
// past W carry no query).  Both lists reach the fusion through FusePre, not from global memory; the optional ColBERT
// list c2 was written by an earlier launch on the stream and is read from memory.  The dense and the BM25 scope come
// from their own tables (their row spaces differ).  Every barrier (two in each block_combine_topk, one + two per token
// group in the BM25 piece) sits under block-uniform conditions and is reached by all four waves; waves 1-3 leave only
// after the last of them.  An empty scope or a qscope outside the table reads nothing and fuses nothing (count 0).
// A BM25 scope of <= 64 documents takes the overlapped order instead (below; AMDR_SCOPE_OVERLAP=0 pins the sequential
// one): measured 37.7 against 46.1 us for one query with a 28-row section, the same bits.
// LDS: the dense lists (TopkLds<C32>) followed by the BM25 piece's region (scope_bm25_lds) — separate, so no barrier
// is needed between the pieces — + the packed fusion's 3.3 KB of static arrays.
struct ScTab {  // one channel's scope table (device pointers)
  const long long* scope_ptr;
  const long long* rows;
  const int* qscope;
  int n_scopes;
};
struct ScFuse {  // what only the fusion at the end needs
  amdr_fuse_params_t P;
  const long long* d_row2uid;  // (both lists go in through FusePre: the row -> uid maps are all the fusion takes of them)
  const long long* b_row2uid;
  ChanIn c2;
  int max_out;
  long long* out_ids;
  double* out_vals;
  int* out_mask;
  int* out_count;
};
__host__ __device__ inline size_t scope_hybrid_dense_lds(int cap_d) { return (TopkLds<C32>::bytes(kScWaves, cap_d) + 15) / 16 * 16; }
// F_at_0 must stay the FIRST parameter: wave 0 reads it from offset 0 of the kernel-argument segment when it gets to
// the fusion.  As an ordinary argument its 33 scalar registers are loaded at the kernel's start and parked across both
// channel pieces, which need 56 and 66 of their own: the compiler then spills 14 of them (to lanes of a vector register).
template <int W>
__global__ __launch_bounds__(kScWaves * 64) void scope_hybrid_kernel(
    ScFuse F_at_0, const float* __restrict__ X, long n, int d, const float* __restrict__ Q, ScBm25 B,
    const int* __restrict__ q_terms, const long long* __restrict__ q_ptr, ScTab td, ScTab tb, int slab_d, int slab_b, int kd,
    int kb, int cap_d, int cap_b, int overlap_docs, float* __restrict__ d_scores, long long* __restrict__ d_ids,
    double* __restrict__ b_scores, long long* __restrict__ b_ids) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const TopkLds<C32> L(smem, kScWaves, cap_d);
  unsigned char* smem_b = smem + scope_hybrid_dense_lds(cap_d);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x;
  long lo, hi, lo_b, hi_b;
  scope_piece(td.scope_ptr, td.qscope, td.n_scopes, slab_d, 0, q, lo, hi);
  scope_piece(tb.scope_ptr, tb.qscope, tb.n_scopes, slab_b, 0, q, lo_b, hi_b);
  // list position sl of query q in lanes 0 .. W-1 (segment 0 of the packed fusion; the other segments have no query:
  // the limit handed in is q + 1)
  const int sl = lane % W;
  const bool seg0 = lane < W;
  FusePre pre;
  pre.have[0] = pre.have[1] = true;
  pre.have[2] = false;
  WaveTopK<C32> tkd;
  WaveTopK<C64> tkb;
  if (hi_b - lo_b <= overlap_docs) {  // block-uniform
    // A BM25 piece of <= 64 documents is one wave's work and the longest chain of the block (per token a binary search
    // of dependent loads): wave 0 runs it alone, without a block barrier, while waves 1-3 take the dense rows; the two
    // meet at the dense combine.  The same lists as the sequential form: the selectors' order is total.
    if (wave == 0) scope_bm25_piece<true>(B, q_terms, q_ptr, q, tb.rows, lo_b, hi_b, slab_b, kb, cap_b, smem_b, tkb);
    scope_dense_piece(X, n, d, Q + (size_t)q * d, td.rows, wave == 0 ? hi : lo, hi, wave == 0 ? 0 : wave - 1, kScWaves - 1,
                      kd, L, wave, lane, tkd);  // (wave 0: no row, an empty list into the combine)
    if (wave != 0) return;  // (behind the last block-wide exchange)
    topk_store(tkd.buf, tkd.cnt, kd, lane, d_scores + (size_t)q * kd, d_ids + (size_t)q * kd);
    const bool vd = seg0 && sl < tkd.cnt;
    pre.dense(vd ? tkd.buf[sl] : C32::pad(), vd);
  } else {
    scope_dense_piece(X, n, d, Q + (size_t)q * d, td.rows, lo, hi, wave, kScWaves, kd, L, wave, lane, tkd);
    if (wave == 0) {  // the dense list: out, and into wave 0's registers for the fusion (the BM25 piece has its own LDS)
      topk_store(tkd.buf, tkd.cnt, kd, lane, d_scores + (size_t)q * kd, d_ids + (size_t)q * kd);
      const bool vd = seg0 && sl < tkd.cnt;
      pre.dense(vd ? tkd.buf[sl] : C32::pad(), vd);
    }
    scope_bm25_piece<false>(B, q_terms, q_ptr, q, tb.rows, lo_b, hi_b, slab_b, kb, cap_b, smem_b, tkb);
    if (wave != 0) return;  // (behind the last block-wide exchange)
  }
  topk_store(tkb.buf, tkb.cnt, kb, lane, b_scores + (size_t)q * kb, b_ids + (size_t)q * kb);
  const bool vb = seg0 && sl < tkb.cnt;
  pre.bm25(vb ? tkb.buf[sl] : C64::pad(), vb);
  typedef const ScFuse __attribute__((address_space(4))) * KernArg;  // (constant address space: scalar loads)
  KernArg f = (KernArg)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(f));  // read here, not before
  const ScFuse F{{f->P.method, f->P.rrf_k, f->P.alpha, f->P.w_dense, f->P.w_bm25, f->P.w_colbert, f->P.min_final_score},
                 f->d_row2uid, f->b_row2uid, ChanIn{f->c2.ids, f->c2.scores, f->c2.row2uid, f->c2.k, f->c2.is_f64},
                 f->max_out, f->out_ids, f->out_vals, f->out_mask, f->out_count};
  const ChanIn c0{nullptr, nullptr, F.d_row2uid, kd, 0}, c1{nullptr, nullptr, F.b_row2uid, kb, 1};
  fuse_packed_body<W, true>(F.P, c0, c1, F.c2, q + 1, F.max_out, F.out_ids, F.out_vals, F.out_mask, F.out_count, pre, q);
}

// ---- MaxSim: one wave per (query, scope document), the pair form of maxsim_scores_h_kernel -------------------------------
// grid: (x = slabs, y = queries).  LDS: TopkLds<C32>(kScWaves, cap)
__global__ __launch_bounds__(kScWaves * 64) void scope_maxsim_kernel(
    const unsigned char* __restrict__ img, const long long* __restrict__ doc_ptr, long n_docs, const float* __restrict__ Q,
    int q_len, float unscale_d, const long long* __restrict__ scope_ptr, const long long* __restrict__ rows,
    const int* __restrict__ qscope, int n_scopes, int slab, int nq, int k, int cap, float* __restrict__ out_scores,
    long long* __restrict__ out_ids) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const TopkLds<C32> L(smem, kScWaves, cap);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.y;
  const int r32 = lane & 31, h = lane >> 5;
  long lo, hi;
  scope_piece(scope_ptr, qscope, n_scopes, slab, blockIdx.x, q, lo, hi);
  WaveTopK<C32> tk;
  tk.init(L.list(wave), cap, k);
  if (lo + wave < hi) {  // wave-uniform: a wave without a document does not read its query
    h8 qh[8], ql[8];
    float unscale;
    ms_load_query_h(Q + (size_t)q * q_len * kDim, q_len, true, r32, h, qh, ql, unscale);
    unscale *= unscale_d;
    for (long i = lo + wave; i < hi; i += kScWaves) {
      const long doc = uniform_i64(rows[i]);
      if (doc < 0 || doc >= n_docs) continue;
      const long t_lo = doc_ptr[doc];
      const int len = (int)(doc_ptr[doc + 1] - t_lo);
      const float total = ms_pair_doc_h(img, t_lo, len, qh, ql, r32, h, q_len, unscale);
      tk.push_uniform(C32::make(total, (u32)doc), lane);
    }
  }
  tk.finalize(lane);
  block_combine_topk(tk, L, kScWaves, wave, lane);
  if (wave != 0) return;
  const size_t row = (size_t)blockIdx.x * nq + q;
  topk_store(tk.buf, tk.cnt, k, lane, out_scores + row * k, out_ids + row * k);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
struct ScTable {  // device pointers
  const long long* scope_ptr;
  const long long* rows;
  const int* qscope;
  int n_scopes;
  int64_t rows_max;
};

int sc_check_table(const char* who, const void* scope_ptr, const void* rows, const void* qscope, int n_scopes,
                   int64_t rows_max, int nq, int k) {
  AMDR_REQUIRE(nq >= 0, "%s: nq=%d", who, nq);
  AMDR_REQUIRE(k >= 1 && k <= AMDR_MAX_K, "%s: k=%d outside [1,%d]", who, k, AMDR_MAX_K);
  AMDR_REQUIRE(n_scopes >= 0 && rows_max >= 0, "%s: bad table sizes", who);
  AMDR_REQUIRE(nq == 0 || (scope_ptr && qscope), "%s: null table", who);
  AMDR_REQUIRE(rows_max == 0 || rows, "%s: null rows", who);
  return AMDR_OK;
}

// where a "_device" call of this channel keeps its slab lists: inside the reserve, or AMDR_EINVAL
int sc_device_region(amdr_scope* s, int chan, int nq, int k, int64_t rows_max, unsigned char** base) {
  AMDR_REQUIRE(nq <= s->nq_max && k <= s->k_max && rows_max <= s->rows_max,
               "scope: a call of nq=%d k=%d rows_max=%lld beyond the reserve (%d, %d, %lld)", nq, k, (long long)rows_max,
               s->nq_max, s->k_max, (long long)s->rows_max);
  const size_t need = scope_region_bytes(chan, nq, k, rows_max);
  AMDR_REQUIRE(need <= s->len[chan], "scope: slab lists of %zu bytes in a region of %zu (AMDR_SCOPE_SLAB changed since the reserve?)",
               need, s->len[chan]);
  *base = s->ws[0].as<unsigned char>() + s->off[chan];
  return AMDR_OK;
}

// Launches of one channel: the batch is the grid's y, so it goes in pieces (grid_y_pieces).  launch(q0, m, slab,
// slabs, cap, out_scores, out_ids) enqueues the scoring kernel of queries [q0, q0 + m); out: where its lists go — the
// slab lists in `region`, merged behind it, or, with a single slab, the queries' rows of the result.
template <class T, class Launch>
int sc_run(int chan, int nq, int k, int64_t rows_max, unsigned char* region, T* scores_dev, int64_t* ids_dev, hipStream_t st,
           Launch&& launch) {
  const int slab = scope_slab(chan), slabs = scope_slabs(chan, rows_max);
  const int cap = topk_cap(k);
  return grid_y_pieces(nq, [&](int q0, int m) -> int {
    T* fs = scores_dev + (size_t)q0 * k;
    int64_t* fi = ids_dev + (size_t)q0 * k;
    T* ps = slabs > 1 ? reinterpret_cast<T*>(region) : fs;
    int64_t* pi = slabs > 1 ? reinterpret_cast<int64_t*>(region + scope_score_bytes(chan, slabs, nq, k)) : fi;
    launch(q0, m, slab, slabs, cap, ps, (long long*)pi);
    AMDR_HIP(hipGetLastError());
    return slabs > 1 ? launch_merge_parts<T>(ps, pi, slabs, m, k, k, fs, fi, st) : AMDR_OK;
  });
}

int sc_dense_run(amdr_dense_t* dense, const float* Q, const ScTable& t, int nq, int k, unsigned char* region,
                 float* scores_dev, int64_t* ids_dev, hipStream_t st) {
  const float* X;
  long n;
  int d;
  dense_matrix(dense, &X, &n, &d);
  return sc_run<float>(kDense, nq, k, t.rows_max, region, scores_dev, ids_dev, st,
                       [&](int q0, int m, int slab, int slabs, int cap, float* os, long long* oi) {
                         hipLaunchKernelGGL(scope_dense_kernel, dim3(slabs, m), dim3(kScWaves * 64),
                                            TopkLds<C32>::bytes(kScWaves, cap), st, X, n, d, Q + (size_t)q0 * d, t.scope_ptr,
                                            t.rows, t.qscope + q0, t.n_scopes, slab, m, k, cap, os, oi);
                       });
}

int sc_bm25_run(const Bm25Raw& b, const int* q_terms, const long long* q_ptr, const ScTable& t, int nq, int k,
                unsigned char* region, double* scores_dev, int64_t* ids_dev, hipStream_t st) {
  return sc_run<double>(kBm25, nq, k, t.rows_max, region, scores_dev, ids_dev, st,
                        [&](int q0, int m, int slab, int slabs, int cap, double* os, long long* oi) {
                          const ScBm25 B{b.term_ptr, b.post_doc, b.post_w, b.idf, b.n_terms, b.n_docs};
                          hipLaunchKernelGGL(scope_bm25_kernel, dim3(slabs, m), dim3(kScWaves * 64), scope_bm25_lds(slab, cap),
                                             st, B, q_terms, q_ptr + q0, t.scope_ptr, t.rows, t.qscope + q0, t.n_scopes, slab, m,
                                             k, cap, os, oi);
                        });
}

int sc_maxsim_run(const MaxsimRaw& r, const float* Q, int q_len, const ScTable& t, int nq, int k, unsigned char* region,
                  float* scores_dev, int64_t* ids_dev, hipStream_t st) {
  return sc_run<float>(kMaxsim, nq, k, t.rows_max, region, scores_dev, ids_dev, st,
                       [&](int q0, int m, int slab, int slabs, int cap, float* os, long long* oi) {
                         hipLaunchKernelGGL(scope_maxsim_kernel, dim3(slabs, m), dim3(kScWaves * 64),
                                            TopkLds<C32>::bytes(kScWaves, cap), st, r.img, r.doc_ptr, r.n_docs,
                                            Q + (size_t)q0 * q_len * kDim, q_len, r.unscale_d, t.scope_ptr, t.rows,
                                            t.qscope + q0, t.n_scopes, slab, m, k, cap, os, oi);
                       });
}

// ---- the one-launch step -------------------------------------------------------------------------------------------------
// AMDR_SCOPE_FUSED=0 pins the separate launches (A/B and tests).  Otherwise: both scopes inside one slab of their channel
// and all candidates of a query inside the packed fusion's 32 lanes.
bool scope_hybrid_applies(int nq, int kd, int kb, int kc, int64_t rows_max_dense, int64_t rows_max_bm25) {
  const char* e = getenv("AMDR_SCOPE_FUSED");
  if (e && e[0] == '0') return false;
  return nq >= 1 && kd >= 1 && kb >= 1 && kc >= 0 && kd + kb + kc <= 32 && rows_max_dense >= 0 && rows_max_bm25 >= 0 &&
         rows_max_dense <= scope_slab(kDense) && rows_max_bm25 <= scope_slab(kBm25);
}
size_t scope_hybrid_lds(int kd, int kb) {
  return scope_hybrid_dense_lds(topk_cap(kd)) + scope_bm25_lds(scope_slab(kBm25), topk_cap(kb));
}

struct ScHybridOut {  // device pointers: the two channel lists and the fused record
  float* dense_scores;
  int64_t* dense_ids;
  double* bm25_scores;
  int64_t* bm25_ids;
  int64_t* ids;
  double* vals;
  int32_t* mask;
  int32_t* count;
};
int sc_hybrid_run(amdr_dense_t* dense, const Bm25Raw& b, const float* Q, const int* q_terms, const long long* q_ptr,
                  const ScTable& td, const ScTable& tb, int nq, int kd, int kb, const amdr_fuse_params_t& P,
                  const int64_t* dense_row2uid, const int64_t* bm25_row2uid, const ChanIn& c2, const ScHybridOut& o,
                  hipStream_t st) {
  const float* X;
  long n;
  int d;
  dense_matrix(dense, &X, &n, &d);
  const int cap_d = topk_cap(kd), cap_b = topk_cap(kb), mo = kd + kb + c2.k;
  const size_t lds = scope_hybrid_lds(kd, kb);
  const ScBm25 B{b.term_ptr, b.post_doc, b.post_w, b.idf, b.n_terms, b.n_docs};
  const ScTab d_tab{td.scope_ptr, td.rows, td.qscope, td.n_scopes}, b_tab{tb.scope_ptr, tb.rows, tb.qscope, tb.n_scopes};
  const char* ov = getenv("AMDR_SCOPE_OVERLAP");  // "0" pins the sequential form (A/B and tests)
  const int overlap_docs = (ov && ov[0] == '0') ? -1 : 64;
  const ScFuse F{P, (const long long*)dense_row2uid, (const long long*)bm25_row2uid, c2, mo, (long long*)o.ids, o.vals, o.mask,
                 o.count};
#define AMDR_SCH_LAUNCH(W)                                                                                               \
  hipLaunchKernelGGL((scope_hybrid_kernel<W>), dim3(nq), dim3(kScWaves * 64), lds, st, F, X, n, d, Q, B, q_terms, q_ptr, \
                     d_tab, b_tab, scope_slab(kDense), scope_slab(kBm25), kd, kb, cap_d, cap_b, overlap_docs,          \
                     o.dense_scores,                                                                                    \
                     (long long*)o.dense_ids, o.bm25_scores, (long long*)o.bm25_ids)
  if (mo <= 16)  // (launch_fuse's choice: the same instantiation of the packed body as the separate fusion launch)
    AMDR_SCH_LAUNCH(16);
  else
    AMDR_SCH_LAUNCH(32);
#undef AMDR_SCH_LAUNCH
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

// the split-fp16 image a scoped MaxSim call needs (the pair form of maxsim_scores_h_kernel); AMDR_MAXSIM_F16X3=0 pins
// the fp32-input forms of the unscoped channel, which have no scoped counterpart
int sc_maxsim_raw(amdr_maxsim_t* h, int q_len, MaxsimRaw* r) {
  AMDR_REQUIRE(h != nullptr, "scope_maxsim: null handle");
  AMDR_REQUIRE(q_len >= 1 && q_len <= AMDR_MAXSIM_QLEN, "scope_maxsim: q_len=%d outside [1,%d]", q_len, AMDR_MAXSIM_QLEN);
  int rc = maxsim_raw(h, r);
  if (rc) return rc;
  const char* e = getenv("AMDR_MAXSIM_F16X3");
  AMDR_REQUIRE(!(e && e[0] == '0'), "scope_maxsim: AMDR_MAXSIM_F16X3=0 pins the fp32-input form; the scoped search has the split-fp16 form only");
  AMDR_REQUIRE(r->img != nullptr, "scope_maxsim: the store has no split-fp16 image (it holds a NaN or an infinity)");
  AMDR_REQUIRE(r->n_docs < (1ll << 32), "scope_maxsim: too many documents");
  return AMDR_OK;
}

// Host table -> device (stage buffer of the handle, on its stream), validated: scope_ptr monotone from >= 0, every
// scope's rows strictly ascending inside [0, n).  qscope may hold any value (outside [0, n_scopes): all padding).
// Layout of the stage buffer: scope_ptr | rows | qscope | operand bytes | scores | ids, each aligned.
struct ScStage {
  ScTable t;
  unsigned char* operand;
  unsigned char* scores;
  int64_t* ids;
};
int sc_stage(amdr_scope* s, const char* who, const int64_t* scope_ptr, const int64_t* rows, const int32_t* qscope,
             int n_scopes, int64_t n, int nq, int k, size_t operand_bytes, size_t score_size, ScStage* out) {
  AMDR_REQUIRE(scope_ptr[0] >= 0, "%s: scope_ptr[0] < 0", who);
  int64_t rows_max = 0;
  for (int i = 0; i < n_scopes; ++i) {
    AMDR_REQUIRE(scope_ptr[i + 1] >= scope_ptr[i], "%s: scope_ptr not monotone at %d", who, i);
    const int64_t len = scope_ptr[i + 1] - scope_ptr[i];
    rows_max = len > rows_max ? len : rows_max;
  }
  const int64_t total = scope_ptr[n_scopes];
  AMDR_REQUIRE(total == 0 || rows, "%s: null rows", who);
  for (int i = 0; i < n_scopes; ++i)
    for (int64_t j = scope_ptr[i]; j < scope_ptr[i + 1]; ++j) {
      AMDR_REQUIRE(rows[j] >= 0 && rows[j] < n, "%s: row %lld of scope %d outside [0,%lld)", who, (long long)rows[j], i,
                   (long long)n);
      AMDR_REQUIRE(j == scope_ptr[i] || rows[j] > rows[j - 1], "%s: rows of scope %d not strictly ascending", who, i);
    }
  const size_t b_ptr = align_up((size_t)(n_scopes + 1) * sizeof(int64_t)), b_rows = align_up((size_t)total * sizeof(int64_t)),
               b_qs = align_up((size_t)nq * sizeof(int32_t)), b_op = align_up(operand_bytes),
               b_sc = align_up((size_t)nq * k * score_size), b_id = align_up((size_t)nq * k * sizeof(int64_t));
  int rc = s->stage.ensure(b_ptr + b_rows + b_qs + b_op + b_sc + b_id);
  if (rc) return rc;
  unsigned char* p = s->stage.as<unsigned char>();
  AMDR_HIP(hipMemcpyAsync(p, scope_ptr, (size_t)(n_scopes + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s->stream));
  if (total) AMDR_HIP(hipMemcpyAsync(p + b_ptr, rows, (size_t)total * sizeof(int64_t), hipMemcpyHostToDevice, s->stream));
  AMDR_HIP(hipMemcpyAsync(p + b_ptr + b_rows, qscope, (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
  out->t = ScTable{reinterpret_cast<const long long*>(p), reinterpret_cast<const long long*>(p + b_ptr),
                   reinterpret_cast<const int*>(p + b_ptr + b_rows), n_scopes, rows_max};
  out->operand = p + b_ptr + b_rows + b_qs;
  out->scores = out->operand + b_op;
  out->ids = reinterpret_cast<int64_t*>(out->scores + b_sc);
  return AMDR_OK;
}
int sc_unstage(amdr_scope* s, const ScStage& g, int nq, int k, size_t score_size, void* scores_host, int64_t* ids_host) {
  AMDR_HIP(hipMemcpyAsync(scores_host, g.scores, (size_t)nq * k * score_size, hipMemcpyDeviceToHost, s->stream));
  AMDR_HIP(hipMemcpyAsync(ids_host, g.ids, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, s->stream));
  AMDR_HIP(hipStreamSynchronize(s->stream));
  return AMDR_OK;
}

}  // namespace

extern "C" {

int amdr_scope_create(int32_t device, amdr_scope_t** out) {
  AMDR_REQUIRE(out != nullptr, "scope_create: out is null");
  *out = nullptr;
  int rc = check_device(device);
  if (rc) return rc;
  amdr_scope* s = new (std::nothrow) amdr_scope();
  if (!s) return fail(AMDR_ENOMEM, "scope_create: host alloc");
  s->device = device;
  if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
    delete s;
    return fail(AMDR_EHIP, "scope_create: stream");
  }
  *out = s;
  return AMDR_OK;
}

int amdr_scope_reserve(amdr_scope_t* s, int32_t nq_max, int32_t k_max, int64_t rows_max) {
  AMDR_REQUIRE(s != nullptr, "scope_reserve: null handle");
  AMDR_REQUIRE(nq_max >= 1 && k_max >= 1 && k_max <= AMDR_MAX_K && rows_max >= 0, "scope_reserve: bad sizes");
  std::lock_guard<std::mutex> g(s->mu);
  AMDR_HIP(hipSetDevice(s->device));
  size_t off[3], len[3], total = 0;
  for (int c = 0; c < 3; ++c) {
    off[c] = total;
    len[c] = scope_region_bytes(c, nq_max, k_max, rows_max);
    total += len[c];
  }
  int rc = s->ws[0].ensure(total);
  if (rc) return rc;
  for (int c = 0; c < 3; ++c) s->off[c] = off[c], s->len[c] = len[c];
  s->nq_max = nq_max;
  s->k_max = k_max;
  s->rows_max = rows_max;
  return AMDR_OK;
}

int amdr_scope_workspace_plan(int32_t nq_max, int32_t k_max, int64_t rows_max_reserve, int32_t nq, int32_t k,
                              int64_t rows_max, int64_t* out6) {
  AMDR_REQUIRE(out6 != nullptr, "scope_workspace_plan: null");
  AMDR_REQUIRE(nq_max >= 1 && k_max >= 1 && k_max <= AMDR_MAX_K && nq >= 1 && k >= 1 && k <= AMDR_MAX_K &&
                   rows_max_reserve >= 0 && rows_max >= 0,
               "scope_workspace_plan: bad sizes");
  for (int c = 0; c < 3; ++c) {
    out6[c] = (int64_t)scope_region_bytes(c, nq_max, k_max, rows_max_reserve);
    out6[3 + c] = (int64_t)scope_region_bytes(c, nq, k, rows_max);
  }
  return AMDR_OK;
}

int amdr_scope_plan_info(const amdr_scope_t* s, int32_t nq, int32_t k, int64_t rows_max, char* buf, int32_t buf_len) {
  AMDR_REQUIRE(s && buf && buf_len > 0, "scope_plan_info: null");
  AMDR_REQUIRE(nq >= 1 && k >= 1 && k <= AMDR_MAX_K && rows_max >= 0, "scope_plan_info: bad sizes");
  const int sd = scope_slabs(kDense, rows_max), sb = scope_slabs(kBm25, rows_max), sm = scope_slabs(kMaxsim, rows_max);
  // the step of dense + BM25 at depth k each (amdr_hybrid_scope_device), without and with a ColBERT list of depth k
  const bool f2 = scope_hybrid_applies(nq, k, k, 0, rows_max, rows_max), f3 = scope_hybrid_applies(nq, k, k, k, rows_max, rows_max);
  snprintf(buf, buf_len,
           "scope_dense_kernel slabs=%d of <= %d rows%s; scope_bm25_kernel slabs=%d of <= %d%s; scope_maxsim_kernel slabs=%d of <= %d%s; "
           "step dense + bm25 + fusion: %s",
           sd, scope_slab(kDense), sd == 1 ? " (direct)" : " + merge_parts_kernel", sb, scope_slab(kBm25),
           sb == 1 ? " (direct)" : " + merge_parts_kernel", sm, scope_slab(kMaxsim),
           sm == 1 ? " (direct)" : " + merge_parts_kernel",
           f3   ? "scope_hybrid_kernel (one launch; also behind a ColBERT list of depth k)"
           : f2 ? "scope_hybrid_kernel (one launch; separate launches with a ColBERT list of depth k)"
                : "separate launches");
  return AMDR_OK;
}

int amdr_scope_dense_search_device(amdr_scope_t* s, amdr_dense_t* dense, const float* Q_dev, const int64_t* scope_ptr_dev,
                                   const int64_t* rows_dev, const int32_t* qscope_dev, int32_t n_scopes, int64_t rows_max,
                                   int32_t nq, int32_t k, float* scores_dev, int64_t* ids_dev, void* stream) {
  AMDR_REQUIRE(s && dense, "scope_dense: null handle");
  int rc = sc_check_table("scope_dense", scope_ptr_dev, rows_dev, qscope_dev, n_scopes, rows_max, nq, k);
  if (rc) return rc;
  AMDR_REQUIRE(nq == 0 || (Q_dev && scores_dev && ids_dev), "scope_dense: null buffer");
  AMDR_REQUIRE(dense_device_of(dense) == s->device, "scope_dense: handles on different devices");
  if (nq == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(s->mu);
  unsigned char* region;
  if ((rc = sc_device_region(s, kDense, nq, k, rows_max, &region))) return rc;
  AMDR_HIP(hipSetDevice(s->device));
  const ScTable t{(const long long*)scope_ptr_dev, (const long long*)rows_dev, qscope_dev, n_scopes, rows_max};
  return sc_dense_run(dense, Q_dev, t, nq, k, region, scores_dev, ids_dev, (hipStream_t)stream);
}

int amdr_scope_bm25_search_device(amdr_scope_t* s, amdr_bm25_t* bm25, const int32_t* q_terms_dev, const int64_t* q_ptr_dev,
                                  const int64_t* scope_ptr_dev, const int64_t* rows_dev, const int32_t* qscope_dev,
                                  int32_t n_scopes, int64_t rows_max, int32_t nq, int32_t k, double* scores_dev,
                                  int64_t* ids_dev, void* stream) {
  AMDR_REQUIRE(s && bm25, "scope_bm25: null handle");
  int rc = sc_check_table("scope_bm25", scope_ptr_dev, rows_dev, qscope_dev, n_scopes, rows_max, nq, k);
  if (rc) return rc;
  AMDR_REQUIRE(nq == 0 || (q_ptr_dev && scores_dev && ids_dev), "scope_bm25: null buffer");
  AMDR_REQUIRE(bm25_device_of(bm25) == s->device, "scope_bm25: handles on different devices");
  if (nq == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(s->mu);
  unsigned char* region;
  if ((rc = sc_device_region(s, kBm25, nq, k, rows_max, &region))) return rc;
  Bm25Raw b;
  if ((rc = bm25_small_raw(bm25, nq, k, &b))) return rc;
  AMDR_HIP(hipSetDevice(s->device));
  const ScTable t{(const long long*)scope_ptr_dev, (const long long*)rows_dev, qscope_dev, n_scopes, rows_max};
  return sc_bm25_run(b, q_terms_dev, (const long long*)q_ptr_dev, t, nq, k, region, scores_dev, ids_dev, (hipStream_t)stream);
}

int amdr_hybrid_scope_plan(int32_t nq, int32_t kd, int32_t kb, int32_t kc, int64_t rows_max_dense, int64_t rows_max_bm25,
                           int32_t* fused, int64_t* lds_bytes) {
  AMDR_REQUIRE(fused && lds_bytes, "hybrid_scope_plan: null");
  AMDR_REQUIRE(nq >= 1 && kd >= 1 && kd <= AMDR_MAX_K && kb >= 1 && kb <= AMDR_MAX_K && kc >= 0 && kc <= AMDR_MAX_K &&
                   rows_max_dense >= 0 && rows_max_bm25 >= 0,
               "hybrid_scope_plan: bad sizes");
  *fused = scope_hybrid_applies(nq, kd, kb, kc, rows_max_dense, rows_max_bm25) ? 1 : 0;
  *lds_bytes = *fused ? (int64_t)scope_hybrid_lds(kd, kb) : 0;
  return AMDR_OK;
}

int amdr_hybrid_scope_device(amdr_scope_t* s, amdr_dense_t* dense, amdr_bm25_t* bm25, const float* Q_dev,
                             const int32_t* q_terms_dev, const int64_t* q_ptr_dev, const int64_t* d_scope_ptr_dev,
                             const int64_t* d_rows_dev, const int32_t* d_qscope_dev, int32_t d_n_scopes, int64_t d_rows_max,
                             const int64_t* b_scope_ptr_dev, const int64_t* b_rows_dev, const int32_t* b_qscope_dev,
                             int32_t b_n_scopes, int64_t b_rows_max, int32_t nq, int32_t kd, int32_t kb,
                             const amdr_fuse_params_t* p, const int64_t* dense_row2uid, const int64_t* bm25_row2uid,
                             const int64_t* colbert_ids, const float* colbert_scores, int32_t kc,
                             const int64_t* colbert_row2uid, float* dense_scores, int64_t* dense_ids, double* bm25_scores,
                             int64_t* bm25_ids, int64_t* out_ids, double* out_vals, int32_t* out_mask, int32_t* out_count,
                             void* stream) {
  AMDR_REQUIRE(s && dense && bm25, "hybrid_scope: null handle");
  AMDR_REQUIRE(p != nullptr, "hybrid_scope: null params");
  AMDR_REQUIRE(p->method >= 0 && p->method <= 3, "hybrid_scope: unknown method %d", p->method);
  AMDR_REQUIRE(kc >= 0 && kc <= AMDR_MAX_K, "hybrid_scope: kc=%d outside [0,%d]", kc, AMDR_MAX_K);
  int rc = sc_check_table("hybrid_scope (dense)", d_scope_ptr_dev, d_rows_dev, d_qscope_dev, d_n_scopes, d_rows_max, nq, kd);
  if (rc) return rc;
  if ((rc = sc_check_table("hybrid_scope (bm25)", b_scope_ptr_dev, b_rows_dev, b_qscope_dev, b_n_scopes, b_rows_max, nq, kb)))
    return rc;
  AMDR_REQUIRE(nq == 0 || (Q_dev && q_ptr_dev && dense_scores && dense_ids && bm25_scores && bm25_ids), "hybrid_scope: null buffer");
  AMDR_REQUIRE(nq == 0 || kc == 0 || (colbert_ids && colbert_scores), "hybrid_scope: null ColBERT list");
  AMDR_REQUIRE(nq == 0 || (out_ids && out_vals && out_mask && out_count), "hybrid_scope: null output");
  AMDR_REQUIRE(dense_device_of(dense) == s->device && bm25_device_of(bm25) == s->device,
               "hybrid_scope: handles on different devices");
  if (nq == 0) return AMDR_OK;
  if (!scope_hybrid_applies(nq, kd, kb, kc, d_rows_max, b_rows_max)) {
    // every other shape: today's calls, in their own regions of the reserve (AMDR_EINVAL beyond it), then the fusion
    if ((rc = amdr_scope_dense_search_device(s, dense, Q_dev, d_scope_ptr_dev, d_rows_dev, d_qscope_dev, d_n_scopes, d_rows_max,
                                             nq, kd, dense_scores, dense_ids, stream)))
      return rc;
    if ((rc = amdr_scope_bm25_search_device(s, bm25, q_terms_dev, q_ptr_dev, b_scope_ptr_dev, b_rows_dev, b_qscope_dev,
                                            b_n_scopes, b_rows_max, nq, kb, bm25_scores, bm25_ids, stream)))
      return rc;
    return amdr_fuse_device(p, nq, dense_ids, dense_scores, kd, dense_row2uid, bm25_ids, bm25_scores, kb, bm25_row2uid,
                            colbert_ids, colbert_scores, kc, colbert_row2uid, out_ids, out_vals, out_mask, out_count,
                            s->device, stream);
  }
  Bm25Raw b;
  if ((rc = bm25_small_raw(bm25, nq, kb, &b))) return rc;
  AMDR_HIP(hipSetDevice(s->device));
  const ScTable td{(const long long*)d_scope_ptr_dev, (const long long*)d_rows_dev, d_qscope_dev, d_n_scopes, d_rows_max};
  const ScTable tb{(const long long*)b_scope_ptr_dev, (const long long*)b_rows_dev, b_qscope_dev, b_n_scopes, b_rows_max};
  const ChanIn c2 = kc ? ChanIn{(const long long*)colbert_ids, colbert_scores, (const long long*)colbert_row2uid, kc, 0}
                       : ChanIn::none();
  const ScHybridOut o{dense_scores, dense_ids, bm25_scores, bm25_ids, out_ids, out_vals, out_mask, out_count};
  return sc_hybrid_run(dense, b, Q_dev, q_terms_dev, (const long long*)q_ptr_dev, td, tb, nq, kd, kb, *p, dense_row2uid,
                       bm25_row2uid, c2, o, (hipStream_t)stream);
}

int amdr_scope_maxsim_search_device(amdr_scope_t* s, amdr_maxsim_t* maxsim, const float* Q_dev, int32_t q_len,
                                    const int64_t* scope_ptr_dev, const int64_t* rows_dev, const int32_t* qscope_dev,
                                    int32_t n_scopes, int64_t rows_max, int32_t nq, int32_t k, float* scores_dev,
                                    int64_t* ids_dev, void* stream) {
  AMDR_REQUIRE(s != nullptr, "scope_maxsim: null handle");
  MaxsimRaw r;
  int rc = sc_maxsim_raw(maxsim, q_len, &r);
  if (rc) return rc;
  if ((rc = sc_check_table("scope_maxsim", scope_ptr_dev, rows_dev, qscope_dev, n_scopes, rows_max, nq, k))) return rc;
  AMDR_REQUIRE(nq == 0 || (Q_dev && scores_dev && ids_dev), "scope_maxsim: null buffer");
  AMDR_REQUIRE(r.device == s->device, "scope_maxsim: handles on different devices");
  if (nq == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(s->mu);
  unsigned char* region;
  if ((rc = sc_device_region(s, kMaxsim, nq, k, rows_max, &region))) return rc;
  AMDR_HIP(hipSetDevice(s->device));
  const ScTable t{(const long long*)scope_ptr_dev, (const long long*)rows_dev, qscope_dev, n_scopes, rows_max};
  return sc_maxsim_run(r, Q_dev, q_len, t, nq, k, region, scores_dev, ids_dev, (hipStream_t)stream);
}

int amdr_scope_dense_search(amdr_scope_t* s, amdr_dense_t* dense, const float* Q_host, const int64_t* scope_ptr,
                            const int64_t* rows, const int32_t* qscope, int32_t n_scopes, int32_t nq, int32_t k,
                            float* scores_host, int64_t* ids_host) {
  AMDR_REQUIRE(s && dense, "scope_dense: null handle");
  int rc = sc_check_table("scope_dense", scope_ptr, rows, qscope, n_scopes, 0, nq, k);
  if (rc) return rc;
  AMDR_REQUIRE(nq == 0 || (Q_host && scores_host && ids_host), "scope_dense: null buffer");
  AMDR_REQUIRE(dense_device_of(dense) == s->device, "scope_dense: handles on different devices");
  if (nq == 0) return AMDR_OK;
  const float* X;
  long n;
  int d;
  dense_matrix(dense, &X, &n, &d);
  std::lock_guard<std::mutex> g(s->mu);
  AMDR_HIP(hipSetDevice(s->device));
  ScStage st;
  const size_t qb = (size_t)nq * d * sizeof(float);
  if ((rc = sc_stage(s, "scope_dense", scope_ptr, rows, qscope, n_scopes, n, nq, k, qb, sizeof(float), &st))) return rc;
  if ((rc = s->ws[1].ensure(scope_region_bytes(kDense, nq, k, st.t.rows_max)))) return rc;
  AMDR_HIP(hipMemcpyAsync(st.operand, Q_host, qb, hipMemcpyHostToDevice, s->stream));
  rc = sc_dense_run(dense, reinterpret_cast<const float*>(st.operand), st.t, nq, k, s->ws[1].as<unsigned char>(),
                    reinterpret_cast<float*>(st.scores), st.ids, s->stream);
  if (rc) return rc;
  return sc_unstage(s, st, nq, k, sizeof(float), scores_host, ids_host);
}

int amdr_scope_bm25_search(amdr_scope_t* s, amdr_bm25_t* bm25, const int32_t* q_terms, const int64_t* q_ptr,
                           const int64_t* scope_ptr, const int64_t* rows, const int32_t* qscope, int32_t n_scopes,
                           int32_t nq, int32_t k, double* scores_host, int64_t* ids_host) {
  AMDR_REQUIRE(s && bm25, "scope_bm25: null handle");
  int rc = sc_check_table("scope_bm25", scope_ptr, rows, qscope, n_scopes, 0, nq, k);
  if (rc) return rc;
  AMDR_REQUIRE(nq == 0 || (q_ptr && scores_host && ids_host), "scope_bm25: null buffer");
  AMDR_REQUIRE(bm25_device_of(bm25) == s->device, "scope_bm25: handles on different devices");
  if (nq == 0) return AMDR_OK;
  AMDR_REQUIRE(q_ptr[0] == 0, "scope_bm25: q_ptr[0] != 0");
  for (int i = 0; i < nq; ++i) AMDR_REQUIRE(q_ptr[i + 1] >= q_ptr[i], "scope_bm25: q_ptr not monotone");
  const int64_t tot = q_ptr[nq];
  AMDR_REQUIRE(tot == 0 || q_terms, "scope_bm25: null q_terms");
  std::lock_guard<std::mutex> g(s->mu);
  Bm25Raw b;
  if ((rc = bm25_small_raw(bm25, nq, k, &b))) return rc;
  AMDR_HIP(hipSetDevice(s->device));
  ScStage st;
  const size_t pb = align_up((size_t)(nq + 1) * sizeof(int64_t)), tb = (size_t)(tot + 1) * sizeof(int32_t);
  if ((rc = sc_stage(s, "scope_bm25", scope_ptr, rows, qscope, n_scopes, b.n_docs, nq, k, pb + tb, sizeof(double), &st)))
    return rc;
  if ((rc = s->ws[1].ensure(scope_region_bytes(kBm25, nq, k, st.t.rows_max)))) return rc;
  AMDR_HIP(hipMemcpyAsync(st.operand, q_ptr, (size_t)(nq + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s->stream));
  if (tot) AMDR_HIP(hipMemcpyAsync(st.operand + pb, q_terms, (size_t)tot * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
  rc = sc_bm25_run(b, reinterpret_cast<const int*>(st.operand + pb), reinterpret_cast<const long long*>(st.operand), st.t, nq,
                   k, s->ws[1].as<unsigned char>(), reinterpret_cast<double*>(st.scores), st.ids, s->stream);
  if (rc) return rc;
  return sc_unstage(s, st, nq, k, sizeof(double), scores_host, ids_host);
}

int amdr_scope_maxsim_search(amdr_scope_t* s, amdr_maxsim_t* maxsim, const float* Q_host, int32_t q_len,
                             const int64_t* scope_ptr, const int64_t* rows, const int32_t* qscope, int32_t n_scopes,
                             int32_t nq, int32_t k, float* scores_host, int64_t* ids_host) {
  AMDR_REQUIRE(s != nullptr, "scope_maxsim: null handle");
  MaxsimRaw r;
  int rc = sc_maxsim_raw(maxsim, q_len, &r);
  if (rc) return rc;
  if ((rc = sc_check_table("scope_maxsim", scope_ptr, rows, qscope, n_scopes, 0, nq, k))) return rc;
  AMDR_REQUIRE(nq == 0 || (Q_host && scores_host && ids_host), "scope_maxsim: null buffer");
  AMDR_REQUIRE(r.device == s->device, "scope_maxsim: handles on different devices");
  if (nq == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(s->mu);
  AMDR_HIP(hipSetDevice(s->device));
  ScStage st;
  const size_t qb = (size_t)nq * q_len * kDim * sizeof(float);
  if ((rc = sc_stage(s, "scope_maxsim", scope_ptr, rows, qscope, n_scopes, r.n_docs, nq, k, qb, sizeof(float), &st))) return rc;
  if ((rc = s->ws[1].ensure(scope_region_bytes(kMaxsim, nq, k, st.t.rows_max)))) return rc;
  AMDR_HIP(hipMemcpyAsync(st.operand, Q_host, qb, hipMemcpyHostToDevice, s->stream));
  rc = sc_maxsim_run(r, reinterpret_cast<const float*>(st.operand), q_len, st.t, nq, k, s->ws[1].as<unsigned char>(),
                     reinterpret_cast<float*>(st.scores), st.ids, s->stream);
  if (rc) return rc;
  return sc_unstage(s, st, nq, k, sizeof(float), scores_host, ids_host);
}

int amdr_scope_destroy(amdr_scope_t* s) {
  if (!s) return AMDR_OK;
  (void)hipSetDevice(s->device);
  if (s->stream) {
    (void)hipStreamSynchronize(s->stream);
    (void)hipStreamDestroy(s->stream);
  }
  s->ws[0].release();
  s->ws[1].release();
  s->stage.release();
  delete s;
  return AMDR_OK;
}

}  // extern "C"

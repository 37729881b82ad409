// The tails of the dense channel that end in the fusion: dense top-k + fusion in one kernel (dense_select_fuse_kernel),
// the second pass of the two-pass long-batch form (dense_hi_select_fuse_kernel) and the serving call in ONE launch
// (hybrid_small_kernel: BM25 + dense + fusion).  They call fuse_packed_body (fuse_core.hpp), bm25_block_query and
// dense_row_dot, each bit-compared with its separate launch: compiled with -ffp-contract=off like fuse.hip and bm25.hip.
#include "bm25_core.hpp"
#include "dense_dot.hpp"
#include "fuse_core.hpp"

#include <cfloat>
#include <cstdlib>

namespace amdr {

// Dense top-k + fusion in ONE kernel for the serving shape under a batch (dense + BM25, <= 1 024 rows, kd + kb <= 32):
// two queries per wave, lanes 0-31 / 32-63 — the mapping of scores_pair_topk_kernel AND of fuse_packed_kernel<32>.
// The half-wave ranks its row of the score matrix S (the same selector, the same bits), writes the dense channel's
// own (scores, ids) and keeps them in its lanes — lane j = list position j, exactly what the packed fusion wants —
// while the BM25 list it requested BEFORE the selection arrives.  Against the two launches: no store + reload of
// the dense list, one memory round trip of the fusion hidden behind the selection, one launch and one wave start
// fewer per two queries.  Mass ties at the cut (the selector's -1) rank the two rows one after the other with the
// staged selector, as scores_pair_topk_kernel does, and then fuse from its list.
__global__ __launch_bounds__(64) void dense_select_fuse_kernel(amdr_fuse_params_t P, const float* __restrict__ S,
                                                               long ldS, long n, int nq, int kd, int cap,
                                                               float* __restrict__ fin_scores,
                                                               long long* __restrict__ fin_ids, ChanIn c0, ChanIn c1,
                                                               int max_out, long long* __restrict__ out_ids,
                                                               double* __restrict__ out_vals, int* __restrict__ out_mask,
                                                               int* __restrict__ out_count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  C32* buf = reinterpret_cast<C32*>(smem);  // cap entries (>= 128): staged-selector list; the pair selector uses 64
  const int lane = threadIdx.x, sl = lane & 31;
  const int q = 2 * blockIdx.x + (lane >> 5);
  const bool has_q = q < nq;
  FusePre pre;
  pre.dense_bm25(c1, q, sl, has_q);  // the BM25 list: in flight during the selection
  C32 out = C32::pad();
  int got = select_row_pair_any(S, ldS, n, q, has_q, kd, lane, buf, out);
  if (got < 0) pair_rows_staged(S, ldS, n, 2 * blockIdx.x, nq, kd, cap, buf, lane, true, out, got);  // mass ties at the cut
  const bool v = sl < got;
  if (has_q && sl < kd) topk_store(out, v, sl, fin_scores + (size_t)q * kd, fin_ids + (size_t)q * kd);
  pre.dense(out, v);
  fuse_packed_body<32, true>(P, c0, c1, ChanIn::none(), nq, max_out, out_ids, out_vals, out_mask, out_count, pre, blockIdx.x * 2);
}

// ---- second pass of the two-pass long-batch dense form (round 4; first pass: dense_small_hi.hip) -----------------------
// S holds APPROXIMATE scores (fp16 roundings of both operands, exact products, fp32 sums) and eps[q] the proven bound on
// their distance from the exact dot products.  Per query (two per wave, a half-wave each, as dense_select_fuse_kernel):
//   1. the pair selector's first stage (rows at or above the k-th best lane maximum, sorted: the first k are the k best
//      approximate scores), then the rows at or above (k-th best approximate score) - 2 eps — every row that can be in the
//      exact top-k: a prefix of that list, or one more sweep of the row when the margin reaches below the first threshold;
//   2. their EXACT fp32 dot products, one candidate at a time, the half-wave's 32 lanes across the row (512-byte loads, a
//      butterfly sum);
//   3. sorted by (exact score, lower id first): the dense channel's top-k — then the fusion, as before.
// More than 32 rows inside the margin (mass near-ties), or no bound for the query (eps NaN): the half-wave re-scores EVERY
// row exactly (over its own row of S) and the plain selectors run on that.  margin_scale (test hook) widens the margin.
template <int V>
__device__ __forceinline__ int select_row_pair_margin(const float* __restrict__ S, long ldS, long n, int q, bool has_q, int k,
                                                      float margin, int lane, C32* scratch, C32& out, int& need) {
  const float* row = S + (size_t)q * ldS;
  const int j = lane & 31;
  f32x4 blk[V / 4];
#pragma unroll
  for (int u = 0; u < V / 4; ++u) {
    const long c0 = 128L * u + 4 * j;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    blk[u] = (has_q && c0 < ldS) ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(row + c0)) : z;  // read once
  }
  u32 sk[V];
#pragma unroll
  for (int u = 0; u < V / 4; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long r = 128L * u + 4 * j + e;
      sk[4 * u + e] = (has_q && r < n) ? ord32(blk[u][e]) : 0u;
    }
  K32 lb;
  lb.c = 0u;
#pragma unroll
  for (int v = 0; v < V; ++v) lb.c = sk[v] > lb.c ? sk[v] : lb.c;
  const K32 sorted_best = wave_sortN_desc<K32, 32>(lb, lane);
  const int kk = (k - 1 < 31 ? k - 1 : 31);
  // (cross-lane reads at wave-uniform positions are two v_readlane and a select; the prefix sum below is five DPP row
  // operations — __shfl / __shfl_up are LDS round trips, eight of them per call of this selector before)
  auto half_lane = [&](int x, int pos) -> int {  // lane `pos` of this lane's half
    const int a = __builtin_amdgcn_readlane(x, pos), b = __builtin_amdgcn_readlane(x, 32 + pos);
    return (lane & 32) ? b : a;
  };
  const u32 T = (u32)half_lane((int)sorted_best.c, kk);  // k-th lane best of this half: <= the k-th best score
  // the rows at or above a key threshold -> this half's 32 scratch slots, sorted into the lanes; -1: more than 32
  auto gather = [&](u32 Te, C32& c) -> int {
    int mine = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) mine += (sk[v] >= Te) ? 1 : 0;
    int incl = mine;  // inclusive prefix sum over the 32 lanes of the half (rows of 16, then row 0 -> 1, 2 -> 3)
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, false);  // row_shr:1
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, false);  // row_shr:2
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xf, false);  // row_shr:4
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xf, false);  // row_shr:8
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1, 3
    const int cnt = half_lane(incl, 31);
    if (cnt > 32) return -1;
    int at = (lane & 32) + incl - mine;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (sk[v] >= Te) {
        C32 e;
        e.c = ((u64)sk[v] << 32) | (u64)(0xffffffffu - (u32)(128 * (v >> 2) + 4 * j + (v & 3)));
        scratch[at++] = e;
      }
    }
    wave_lds_fence();
    c = (j < cnt) ? scratch[lane] : C32::pad();
    c = wave_sortN_desc<C32, 32>(c, lane);
    wave_lds_fence();
    return cnt;
  };
  // stage 1, the exact form's own selection: the rows at or above the k-th LANE maximum (a few more than k: its first k
  // are the k best approximate scores).  With the margin already taken off that threshold (the first version), depths from
  // ~14 up had more than 32 survivors on most queries and fell back to re-scoring the whole row: 732 against 559 us at
  // k = 16, 3.4 against 0.6 ms at k = 20 (1 024 x 768, 37 376 queries).
  const u32 Te1 = T > 1u ? T : 1u;  // (T == 0: fewer than k rows — every row)
  C32 c;
  int cnt = gather(Te1, c);
  if (cnt < 0) return -1;  // (this lane's half; the caller votes)
  // stage 2: everything at or above (k-th best approximate score) - margin.  Usually a prefix of the sorted survivors;
  // when the margin reaches below the lane-maximum threshold the row is swept again with the cut itself.
  u32 cut = 1u;
  if (cnt > kk) {
    const float tk_f = __int_as_float(half_lane(__float_as_int(c.score()), kk));
    cut = ord32(tk_f - margin);
    cut = cut > 1u ? cut : 1u;
  }
  if (cut < Te1) {  // (half-uniform)
    cnt = gather(cut, c);
    if (cnt < 0) return -1;
    need = cnt;
  } else {
    const unsigned long long m = __ballot(j < cnt && (u32)(c.c >> 32) >= cut);
    need = __popcll((lane & 32) ? (m >> 32) : (m & 0xffffffffull));
  }
  out = c;
  return cnt;
}

template <bool FUSE, int D128>  // D128 = d / 128 (the row a half-wave re-scores: D128 16-byte pieces per lane)
__global__ __launch_bounds__(64) void dense_hi_select_fuse_kernel(amdr_fuse_params_t P, const float* __restrict__ S, long ldS, long n,
                                                                  int nq, int kd, const float* __restrict__ X,
                                                                  const float* __restrict__ Q, int d,
                                                                  const float* __restrict__ eps, float margin_scale,
                                                                  float* __restrict__ fin_scores, long long* __restrict__ fin_ids,
                                                                  ChanIn c0, ChanIn c1, int max_out,
                                                                  long long* __restrict__ out_ids, double* __restrict__ out_vals,
                                                                  int* __restrict__ out_mask, int* __restrict__ out_count,
                                                                  unsigned int* __restrict__ fallbacks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  C32* buf = reinterpret_cast<C32*>(smem);  // 128 entries: the selectors' scratch
  const int lane = threadIdx.x, sl = lane & 31, half = lane >> 5;
  const int q = 2 * blockIdx.x + half;
  const bool has_q = q < nq;
  // (FusePre::dense_bm25 written out: through the helper every <true, D> instantiation takes 1-5 more vector registers)
  FusePre pre;
  pre.have[0] = pre.have[1] = true;
  pre.have[2] = false;
  pre.id[1] = -1;
  pre.s[1] = 0.0;
  if (FUSE && has_q && sl < c1.k) {  // the BM25 list: in flight during the selection
    pre.id[1] = c1.ids[(size_t)q * c1.k + sl];
    pre.s[1] = chan_score(c1, q, sl);
  }
  const float e_q = has_q ? eps[q] : 0.f;
  const float margin = 2.f * e_q * margin_scale;
  bool exact_all = has_q && !(margin == margin && margin <= FLT_MAX);  // no bound for this query
  // this half's query, spread over its 32 lanes: lane sl holds components 128 u + 4 sl .. + 3
  f32x4 qv[D128];
#pragma unroll
  for (int u = 0; u < D128; ++u) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    qv[u] = has_q ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(Q + (size_t)q * d + 128 * u + 4 * sl)) : z;  // (the
    // streamed score rows and queries are read once: non-temporal, so that the chunk rows the candidates re-read stay in L2)
  }
  // the sum of a value over the 32 lanes of each half, in every lane of the half: five DPP row operations leave the halves'
  // sums in lanes 31 and 63 (dense_dot.hpp), two v_readlane hand them out — no LDS round trips (ds_bpermute shuffles made
  // the re-scoring a chain of ~10 of them per candidate)
  auto half_sum = [&](float v) -> float {
    v = dpp_add<0x111, 0xf>(v);
    v = dpp_add<0x112, 0xf>(v);
    v = dpp_add<0x114, 0xf>(v);
    v = dpp_add<0x118, 0xf>(v);
    v = dpp_add<0x142, 0xa>(v);
    const float s0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 31));
    const float s1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
    return half ? s1 : s0;
  };
  auto row_load = [&](long r, f32x4 (&xv)[D128]) {
    const float* xr = X + (size_t)r * d + 4 * sl;
#pragma unroll
    for (int u = 0; u < D128; ++u) xv[u] = *reinterpret_cast<const f32x4*>(xr + 128 * u);
  };
  auto row_fma = [&](const f32x4 (&xv)[D128]) -> float {
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < D128; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = fmaf(xv[u][e], qv[u][e], acc);
    return half_sum(acc);
  };
  auto row_dot = [&](long r) -> float {  // every lane of the half returns <Q[q], X[r]> (r: uniform in the half)
    f32x4 xv[D128];
    row_load(r, xv);
    return row_fma(xv);
  };
  C32 out = C32::pad();
  int need = 0, got = 0;
  {
    // (a half without a bound runs the selector on whatever its row holds and discards the result: the other half of the
    // wave needs its own)
    const float mg = (has_q && !exact_all) ? margin : 0.f;
    if (n <= 256)
      got = select_row_pair_margin<8>(S, ldS, n, q, has_q, kd, mg, lane, buf, out, need);
    else if (n <= 512)
      got = select_row_pair_margin<16>(S, ldS, n, q, has_q, kd, mg, lane, buf, out, need);
    else if (n <= 640)
      got = select_row_pair_margin<20>(S, ldS, n, q, has_q, kd, mg, lane, buf, out, need);
    else
      got = select_row_pair_margin<32>(S, ldS, n, q, has_q, kd, mg, lane, buf, out, need);
    exact_all = exact_all || (has_q && got < 0);
    if (exact_all) need = 0;
  }
  if (__any(exact_all)) {  // wave-uniform: one of the two halves (or both) re-scores its whole row
    const unsigned long long fbm = __ballot(exact_all && sl == 0);  // (one lane per half)
    if (lane == 0 && fallbacks) atomicAdd(fallbacks, (unsigned int)__popcll(fbm));
    const C32 keep = out;
    const int keep_need = need, keep_got = got;
    // the exact scores of the half's whole row, written over its own row of S (the selector above has read it into
    // registers, and this block is its only reader), then the plain selectors on them.  (They were two rows of 1 024
    // floats in LDS: 8 KiB in every block for a path the headline takes for no query, and the LDS capped the kernel at
    // three waves per SIMD where its registers allow four.)  Rows r >= n are never read: the selectors mask them.
    float* xs = const_cast<float*>(S);
    for (long r = 0; r < n; ++r) {
      const float v = row_dot(r);
      if (exact_all && sl == 0) xs[(size_t)q * ldS + r] = v;
    }
    __threadfence_block();  // the stores are complete before the wave reads them back (one CU: its L1 is write-through)
    C32 o2 = C32::pad();
    int g2 = select_row_pair_any(xs, ldS, n, q, has_q && exact_all, kd, lane, buf, o2);
    // mass ties at the cut among EXACT scores: the staged selector, one half after the other
    if (g2 < 0) pair_rows_staged(xs, ldS, n, 2 * blockIdx.x, nq, kd, 128, buf, lane, exact_all, o2, g2);
    if (exact_all) {  // this half's list is final: exact scores already
      out = o2;
      got = g2 < kd ? g2 : kd;
      need = 0;
    } else {
      out = keep;
      got = keep_got;
      need = keep_need;
    }
  }
  // ---- exact scores of the candidates (the first `need` survivors of each half), one per step
  const int steps = __builtin_amdgcn_readfirstlane(max(__shfl(need, 0), __shfl(need, 32)));
  float mine_exact = 0.f;
  const int my_id = (int)out.id();
  // two candidates per step: both rows requested before either is summed.  (Tried: the NEXT step's rows requested before
  // this step's are summed, two register sets in ping-pong — 146 VGPRs, three waves per SIMD instead of four: 119.5 against
  // 119.1 us; the kernel issues 2 289 vector instructions per wave = 56 % of its time and waits on memory for half of it.
  // The other direction, amdgpu_waves_per_eu(5) / (6): registers capped at 96 / 80, the rest spilled (4 / 172 at d = 384, more at 768) — the d = 768 step 0.258 -> 0.279 / 0.291 ms.)
  for (int c = 0; c < steps; c += 2) {  // (steps: wave-uniform)
    // candidates c, c + 1 of each half: their lanes are wave-uniform (v_readlane), the half picks its own
    const int c1 = c + 1 < 32 ? c + 1 : 31;
    const int ra0 = __builtin_amdgcn_readlane(my_id, c), ra1 = __builtin_amdgcn_readlane(my_id, 32 + c);
    const int rb0 = __builtin_amdgcn_readlane(my_id, c1), rb1 = __builtin_amdgcn_readlane(my_id, 32 + c1);
    const bool la = c < need, lb = c + 1 < need;
    f32x4 xa[D128], xb[D128];
    row_load(la ? (long)(half ? ra1 : ra0) : 0, xa);
    row_load(lb ? (long)(half ? rb1 : rb0) : 0, xb);
    const float va = row_fma(xa), vb = row_fma(xb);
    if (la && sl == c) mine_exact = va;
    if (lb && sl == c + 1) mine_exact = vb;
  }
  if (need > 0) {
    C32 c = (sl < need) ? C32::make(mine_exact, (u32)out.id()) : C32::pad();
    c = wave_sortN_desc<C32, 32>(c, lane);
    out = c;
    got = need < kd ? need : kd;
  }
  const bool v = sl < got && sl < kd;
  if (has_q && sl < kd) topk_store(out, v, sl, fin_scores + (size_t)q * kd, fin_ids + (size_t)q * kd);
  if (FUSE) {
    pre.dense(out, v);
    fuse_packed_body<32, true>(P, c0, c1, ChanIn::none(), nq, max_out, out_ids, out_vals, out_mask, out_count, pre, blockIdx.x * 2);
  }
}

// ---- the serving call in ONE launch ------------------------------------------------------------------------------------
// HybridRetriever.search() issues one query at a time (hybrid_retriever.py:282-384); on a serving corpus (591 / 1 260
// chunks) its dense + BM25 step was FOUR short launches — BM25 scoring + top-k, one wave per (query, row) of dense scores,
// the dense top-k, the fusion — 45 us of which ~15 are kernels.  Here one launch does all four for 1-4 queries on a
// corpus of <= 2 048 chunks: blocks take ROLES — block 0 of a query is its BM25 wave (bm25_core.hpp bm25_block_query: the
// channel's own code), blocks 1.. take 16 chunk rows each (dense_dot.hpp dense_row_dot: one wave per row, the GEMV
// form's instruction sequence) — and hand over through two self-resetting arrival counters per query (a wave
// drains its stores, releases at agent scope and takes a ticket; the last ticket holder acquires — MI355X_MICROARCH.md,
// inter-workgroup visibility): the LAST dense block to arrive ranks the score row (the register selector of the slab
// top-k) while the BM25 wave is still scoring, and the SECOND of the two finished channel lists to arrive fuses
// (fuse_packed_body, the packed fusion's code).  The same instructions as the four launches, hence the same bits
// (tests/test_hybrid_small_gpu.py).
struct SmallArgs {
  // BM25 role
  const long long* term_ptr;
  const int* post_doc;
  const double* post_w;
  const double* idf;
  long n_terms, n_docs;
  const int* q_terms;
  const long long* q_ptr;
  int kb, cap, slab, use_select;
  double* bm_scores;     // [nq, kb]
  long long* bm_ids;
  // dense role
  const float* X;
  const float* Q;
  long n_rows;
  int d, rows_per_block, blocks_per_query;
  float* S;              // [nq, ldS]
  long ldS;
  int kd, cap_sel;
  float* d_scores;       // [nq, kd]
  long long* d_ids;
  int* ticket;           // [>= nq] zero before the launch, zero after
};

// one wave's arrival at a counter: its stores are out and released at agent scope; returns the ticket (wave-uniform)
__device__ __forceinline__ int small_arrive(int* counter, int lane) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  int t = 0;
  if (lane == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    t = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return __builtin_amdgcn_readfirstlane(t);
}
__device__ __forceinline__ void small_acquire(int* counter, int lane) {
  if (lane == 0) __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int NVT>
__global__ __launch_bounds__(256) void hybrid_small_kernel(SmallArgs A, amdr_fuse_params_t P, ChanIn c0, ChanIn c1, int nq,
                                                           int max_out, long long* __restrict__ out_ids,
                                                           double* __restrict__ out_vals, int* __restrict__ out_mask,
                                                           int* __restrict__ out_count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int q = blockIdx.y, role = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int* rows_done = A.ticket + q;       // arrivals of the dense blocks of query q
  int* lists_done = A.ticket + 32 + q; // arrivals of its two channel lists
  const int sl = lane & 31;
  C32 dense_mine = C32::pad();  // list position sl of the dense channel, when this wave ranked the row itself
  bool have_dense = false, dense_valid = false;
  if (role == 0) {
    // ---- the BM25 channel of query q: one wave, the channel's own code; the other three have nothing to do
    if (wave != 0) return;
    bm25_block_query<1, NVT>(A.term_ptr, A.post_doc, A.post_w, A.idf, A.n_terms, A.n_docs, A.q_terms, A.q_ptr, nq, A.kb,
                             A.cap, A.slab, A.use_select, nullptr, nullptr, A.bm_scores, A.bm_ids, q, 0, smem);
  } else {
    // ---- rows_per_block chunk rows of the dense channel, one wave per row (the GEMV form's dot product)
    const long r0 = (long)(role - 1) * A.rows_per_block;
    long r1 = r0 + A.rows_per_block;
    if (r1 > A.n_rows) r1 = A.n_rows;
    for (long r = r0 + wave; r < r1; r += 4) {
      const float acc = dense_row_dot(A.X + (size_t)r * A.d, A.Q + (size_t)q * A.d, A.d, lane);
      if (lane == 63) A.S[(size_t)q * A.ldS + r] = acc;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // every wave's scores are out
    if (wave != 0) return;
    if (small_arrive(rows_done, lane) != A.blocks_per_query - 2) return;
    // ---- the last dense block to arrive: top-k of row q (scores_slab_topk_kernel<1>'s selection)
    small_acquire(rows_done, lane);
    C32* buf = reinterpret_cast<C32*>(smem);
    const float* row = A.S + (size_t)q * A.ldS;
    const long n = A.n_rows;
    WaveTopK<C32> tk;
    tk.init(buf, A.cap_sel, A.kd);
    const int got = select_row_any(row, 0, n, A.kd, lane, tk.buf);
    if (got >= 0)
      tk.cnt = got;
    else  // mass ties at the cut: the staged selector
      wave_topk_sweep(tk, row, 0, n, lane);
    wave_lds_fence();
    const bool v = lane < 32 && sl < tk.cnt;
    const C32 mine = v ? tk.buf[sl] : C32::pad();
    if (lane < A.kd) topk_store(mine, v, lane, A.d_scores + (size_t)q * A.kd, A.d_ids + (size_t)q * A.kd);
    dense_mine = mine;
    dense_valid = v;
    have_dense = true;
    wave_lds_fence();
  }
  // ---- a finished channel list; the second of the two to arrive fuses (the BM25 wave while the dense rows were being
  // ranked elsewhere, or the ranking wave when BM25 finished first)
  if (small_arrive(lists_done, lane) != 1) return;
  small_acquire(lists_done, lane);
  long long dense_id = -1;
  double dense_s = 0.0;
  if (!have_dense && lane < 32 && sl < A.kd) {
    dense_id = A.d_ids[(size_t)q * A.kd + sl];
    dense_s = dense_id >= 0 ? (double)A.d_scores[(size_t)q * A.kd + sl] : 0.0;
  }
  FusePre pre;
  pre.dense_bm25(c1, q, sl, lane < 32);
  if (have_dense) {
    pre.dense(dense_mine, dense_valid);
  } else {
    pre.id[0] = dense_id;
    pre.s[0] = dense_s;
  }
  // segment 0 (lanes 0-31) = query q, segment 1 has no query (q + 1 >= the limit handed in)
  fuse_packed_body<32, true>(P, c0, c1, ChanIn::none(), q + 1, max_out, out_ids, out_vals, out_mask, out_count, pre, q);
}

bool dense_select_fuse_applies(long n, int slabs, int m, int kd, int kb) {
  const char* e = getenv("AMDR_DENSE_FUSE");  // "0" pins the two-launch form (A/B, tests)
  if (e && e[0] == '0') return false;
  return slabs == 1 && n >= 1 && n <= 1024 && kd >= 1 && kd <= 32 && kb >= 0 && kd + kb <= 32 && m >= 1;
}

int dense_select_fuse_launch(const FuseTail& t, int q0, const float* S, long ldS, long n, int m, int kd, int cap,
                             float* fin_scores, int64_t* fin_ids, hipStream_t st) {
  const FuseTailArgs a = fuse_tail_args(t, q0, kd, nullptr, nullptr);
  hipLaunchKernelGGL(dense_select_fuse_kernel, dim3((m + 1) / 2), dim3(64), (size_t)cap * sizeof(C32), st, *t.p, S, ldS, n,
                     m, kd, cap, fin_scores, (long long*)fin_ids, a.c0, a.c1, a.mo, a.ids, a.vals, a.mask, a.count);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

// one launch of dense_hi_select_fuse_kernel<FUSE, d / 128> over m queries
template <bool FUSE, class... Args>
static void hi_select_dispatch(int d, int m, size_t lds, hipStream_t st, Args... args) {
#define AMDR_HSF(D) \
  hipLaunchKernelGGL((dense_hi_select_fuse_kernel<FUSE, D>), dim3((m + 1) / 2), dim3(64), lds, st, args...)
  switch (d >> 7) {
    case 1: AMDR_HSF(1); break;
    case 2: AMDR_HSF(2); break;
    case 3: AMDR_HSF(3); break;
    case 4: AMDR_HSF(4); break;
    case 5: AMDR_HSF(5); break;
    case 6: AMDR_HSF(6); break;
    case 7: AMDR_HSF(7); break;
    default: AMDR_HSF(8); break;
  }
#undef AMDR_HSF
}

// second pass of the two-pass long-batch form (dense_hi_select_fuse_kernel); t == nullptr: the dense lists only.
// S is the caller's scratch score matrix: a query that takes the whole-row fallback gets its row overwritten with exact
// scores.
int dense_hi_select_launch(const FuseTail* t, int q0, const float* S, long ldS, long n, int m, int kd, const float* X,
                           const float* Q, int d, const float* eps, float* fin_scores, int64_t* fin_ids,
                           unsigned int* fallbacks, hipStream_t st) {
  const char* ms = getenv("AMDR_DENSE_SMALL_HI_MARGIN");  // test hook: widens the candidate margin (a huge one: every
  const float margin_scale = ms ? (float)atof(ms) : 1.f;  // query takes the exact fallback inside the kernel)
  const size_t lds = 128 * sizeof(C32);  // the selectors' scratch (the whole-row fallback re-uses the rows of S)
  const amdr_fuse_params_t P0{};
  const FuseTailArgs a = t ? fuse_tail_args(*t, q0, kd, nullptr, nullptr)
                           : FuseTailArgs{ChanIn::none(), ChanIn::none(), 0, nullptr, nullptr, nullptr, nullptr};
  if (t)
    hi_select_dispatch<true>(d, m, lds, st, *t->p, S, ldS, n, m, kd, X, Q, d, eps, margin_scale, fin_scores,
                             (long long*)fin_ids, a.c0, a.c1, a.mo, a.ids, a.vals, a.mask, a.count, fallbacks);
  else
    hi_select_dispatch<false>(d, m, lds, st, P0, S, ldS, n, m, kd, X, Q, d, eps, margin_scale, fin_scores,
                              (long long*)fin_ids, a.c0, a.c1, a.mo, a.ids, a.vals, a.mask, a.count, fallbacks);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

// AMDR_HYBRID_SMALL=0 pins the separate launches (A/B and tests)
bool hybrid_small_applies(long n_dense, long n_bm25, int nslabs, int nq, int kd, int kb) {
  const char* e = getenv("AMDR_HYBRID_SMALL");
  if (e && e[0] == '0') return false;
  return nq >= 1 && nq <= 4 && n_dense >= 1 && n_dense <= kSelectRowsMax && n_bm25 >= 1 && nslabs == 1 && kd >= 1 && kb >= 1 &&
         kd + kb <= 32;
}

// chunk rows per dense block (4 waves).  Every block costs an arrival (one atomic on the query's counter) and a block
// start; measured on 591 x 384 ... 2 048 x 768, 1-4 queries (scripts/ab_hybrid_small.py): 16 rows up to ~2 500
// (query, row) pairs, 32 beyond.  AMDR_HYBRID_SMALL_ROWS pins a value (multiple of 4).
static int hybrid_small_rows(long n, int nq) {
  static const int pinned = [] {
    const char* e = getenv("AMDR_HYBRID_SMALL_ROWS");
    int r = e ? atoi(e) : 0;
    if (r <= 0) return 0;
    if (r < 4) r = 4;
    if (r > 64) r = 64;
    return (r + 3) / 4 * 4;
  }();
  if (pinned) return pinned;
  return n * nq <= 2560 ? 16 : 32;
}

int hybrid_small_launch(const DenseRaw& dr, const Bm25Raw& br, const float* Q, const int* q_terms, const long long* q_ptr,
                        int nq, int kd, int kb, const amdr_fuse_params_t& P, const int64_t* dense_row2uid,
                        const int64_t* bm25_row2uid, float* dense_scores, int64_t* dense_ids, double* bm25_scores,
                        int64_t* bm25_ids, int64_t* out_ids, double* out_vals, int32_t* out_mask, int32_t* out_count,
                        hipStream_t st) {
  SmallArgs A;
  A.term_ptr = br.term_ptr;
  A.post_doc = br.post_doc;
  A.post_w = br.post_w;
  A.idf = br.idf;
  A.n_terms = br.n_terms;
  A.n_docs = br.n_docs;
  A.q_terms = q_terms;
  A.q_ptr = q_ptr;
  A.kb = kb;
  A.cap = br.cap;
  A.slab = br.slab;
  A.use_select = br.select_on ? 1 : 0;
  A.bm_scores = bm25_scores;
  A.bm_ids = (long long*)bm25_ids;
  A.X = dr.X;
  A.Q = Q;
  A.d = dr.d;
  A.n_rows = dr.n;
  A.rows_per_block = hybrid_small_rows(dr.n, nq);
  const int dense_blocks = (int)((dr.n + A.rows_per_block - 1) / A.rows_per_block);
  A.blocks_per_query = 1 + dense_blocks;
  A.S = dr.S;
  A.ldS = dr.ld;
  A.kd = kd;
  int cap_sel = topk_cap(kd);
  if (cap_sel < 128) cap_sel = 128;
  A.cap_sel = cap_sel;
  A.d_scores = dense_scores;
  A.d_ids = (long long*)dense_ids;
  A.ticket = br.ticket;
  size_t lds = br.lds;
  if (lds < (size_t)cap_sel * sizeof(C32)) lds = (size_t)cap_sel * sizeof(C32);
  const int mo = kd + kb;
  ChanIn c0{nullptr, nullptr, (const long long*)dense_row2uid, kd, 0};
  ChanIn c1{(const long long*)bm25_ids, (const void*)bm25_scores, (const long long*)bm25_row2uid, kb, 1};
  // grid y: the one-launch step serves nq <= 4 (hybrid_small_applies)
#define AMDR_HS_LAUNCH(NVT)                                                                                        \
  hipLaunchKernelGGL((hybrid_small_kernel<NVT>), dim3(A.blocks_per_query, nq), dim3(256), lds, st, A, P, c0, c1, nq, mo, \
                     (long long*)out_ids, out_vals, out_mask, out_count)
  const int nv = br.nvt;  // (bm_run's choice of register bucket)
  if (nv <= 4) AMDR_HS_LAUNCH(4);
  else if (nv <= 8) AMDR_HS_LAUNCH(8);
  else if (nv <= 10) AMDR_HS_LAUNCH(10);
  else if (nv <= 16) AMDR_HS_LAUNCH(16);
  else if (nv <= 20) AMDR_HS_LAUNCH(20);
  else AMDR_HS_LAUNCH(32);
#undef AMDR_HS_LAUNCH
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

}  // namespace amdr

using namespace amdr;

extern "C" {

int amdr_hybrid_small_device(amdr_dense_t* dense, amdr_bm25_t* bm25, const float* Q_dev, const int32_t* q_terms_dev,
                             const int64_t* q_ptr_dev, int32_t nq, int32_t kd, int32_t kb, const amdr_fuse_params_t* p,
                             const int64_t* dense_row2uid, const int64_t* bm25_row2uid, float* dense_scores_dev,
                             int64_t* dense_ids_dev, double* bm25_scores_dev, int64_t* bm25_ids_dev, int64_t* out_ids,
                             double* out_vals, int32_t* out_mask, int32_t* out_count, void* stream) {
  AMDR_REQUIRE(dense && bm25, "hybrid_small: null index handle");
  AMDR_REQUIRE(p != nullptr, "hybrid_small: null params");
  AMDR_REQUIRE(p->method >= 0 && p->method <= AMDR_FUSE_WEIGHTED_SUM, "hybrid_small: method=%d", p->method);
  AMDR_REQUIRE(nq >= 0 && kd >= 1 && kd <= AMDR_MAX_K && kb >= 1 && kb <= AMDR_MAX_K, "hybrid_small: bad sizes");
  if (nq == 0) return AMDR_OK;
  AMDR_REQUIRE(Q_dev && q_terms_dev && q_ptr_dev, "hybrid_small: null query buffers");
  AMDR_REQUIRE(dense_scores_dev && dense_ids_dev && bm25_scores_dev && bm25_ids_dev, "hybrid_small: null channel lists");
  AMDR_REQUIRE(out_ids && out_vals && out_mask && out_count, "hybrid_small: null output");
  int64_t nd = 0, nb = 0;
  int rc;
  if ((rc = amdr_dense_ntotal(dense, &nd))) return rc;
  if ((rc = amdr_bm25_ndocs(bm25, &nb))) return rc;
  AMDR_REQUIRE(kd <= nd || nd == 0, "hybrid_small: kd=%d > %lld rows", kd, (long long)nd);
  bool one = false;
  if (nd >= 1 && nb >= 1 && nq <= 4 && dense_device_of(dense) >= 0) {
    std::lock_guard<std::mutex> gd(dense_mutex(dense));
    std::lock_guard<std::mutex> gb(bm25_mutex(bm25));
    AMDR_HIP(hipSetDevice(dense_device_of(dense)));
    Bm25Raw br;
    if ((rc = bm25_small_raw(bm25, nq, kb, &br))) return rc;
    if (hybrid_small_applies((long)nd, (long)nb, br.nslabs, nq, kd, kb)) {
      DenseRaw dr;
      if ((rc = dense_small_raw(dense, nq, &dr))) return rc;
      one = true;
      rc = hybrid_small_launch(dr, br, Q_dev, q_terms_dev, (const long long*)q_ptr_dev, nq, kd, kb, *p, dense_row2uid,
                               bm25_row2uid, dense_scores_dev, dense_ids_dev, bm25_scores_dev, bm25_ids_dev, out_ids,
                               out_vals, out_mask, out_count, (hipStream_t)stream);
    }
  }
  if (one) return rc;
  if ((rc = amdr_bm25_search_device(bm25, q_terms_dev, q_ptr_dev, nq, kb, bm25_scores_dev, bm25_ids_dev, stream))) return rc;
  return amdr_dense_search_fuse_device(dense, Q_dev, nq, kd, p, dense_row2uid, bm25_ids_dev, bm25_scores_dev, kb,
                                       bm25_row2uid, dense_scores_dev, dense_ids_dev, out_ids, out_vals, out_mask,
                                       out_count, stream);
}

}  // extern "C"

// ColBERT channel: exhaustive late-interaction MaxSim for gfx950.
//
// Replaces `Searcher.search(query, k)` (legalrag/retrieval/colbert_retriever.py:152):
//   score(q, doc) = sum_{i < q_len} max_{j < len(doc)} <q_i, d_j>,  dim = 128, fp32.
// A wave scores (query, document) pairs tile by tile: the 32 query tokens x 32 document tokens
// similarity tile is a genuine small matrix product, so it runs on the matrix cores with the
// fp32-input v_mfma_f32_16x16x4_f32 (exact fp32 products and sums, the peak rate of the vector
// ALU, no cross-lane reduction, no LDS broadcast traffic), four 16x16 accumulator blocks:
//   A (16 doc tokens x 4)   : lane (i16 = l&15, kq = l>>4) holds D[tok0 + 16 bi + i16][16-B slots 4t + kq]
//   B (4 x 16 query tokens) : lane (i16, kq)              holds Q[16 bj + i16][16-B slots 4t + kq]
// (t = 0..7: the k index is permuted, identically for both operands — a dot product does not
// care.)  C[doc token][query token] comes back with the query token on the lane (l & 15) and
// 4 doc tokens per accumulator block in the lane's registers, so max-over-tokens is in-register
// plus two lane exchanges, and the final sum over query tokens is one DPP reduction per document.
// (First built on v_mfma_f32_32x32x2_f32; the 16x16 form holds a higher clock, see dense_mfma.hip.)
// Algorithmic bytes per (query, shard): sum_docs len*128*4; flops 2*32*128*sum len.
// (The token store — its statistics, images and updates — is maxsim_store.hip; the handle is maxsim_handle.hpp.)
#include "common.hpp"
#include "lds_ring.hpp"
#include "maxsim_core.hpp"
#include "maxsim_handle.hpp"
#include "topk.hpp"

#include <cfloat>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>

namespace amdr {

// One 32x32 tile: 8 slots x 4 components x (2 x 2 accumulator blocks) = 128 MFMAs of 32 cycles.
// a[bi][t] / q[bj][t]: the lane's 16-B slot 4t + kq of document-token row 16 bi + i16 / query-token
// row 16 bj + i16.  Returns, per query-token block bj, the maximum over this lane's 8 document
// tokens (rows 16 bi + 4 kq + r), rows >= remain masked out.
// NBI = 1: the tile holds at most 16 document tokens (the tail of a document): the second row block
// would be masked out entirely, so its 64 MFMAs (and the caller's 8 fragment reads) are skipped —
// same results, and documents are short (Civil-Code articles: 77 tokens on average, 17 % of the
// 32-token tile slots were padding).
template <int NBI>
__device__ __forceinline__ void ms_tile(const f32x4 (&a)[2][8], const f32x4 (&q)[2][8], int kq, int remain,
                                        float (&best)[2]) {
  f32x4 acc[NBI][2];
#pragma unroll
  for (int bi = 0; bi < NBI; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int bi = 0; bi < NBI; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[bi][t][e], q[bj][t][e], acc[bi][bj], 0, 0, 0);
#pragma unroll
  for (int bi = 0; bi < NBI; ++bi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool off = remain < 32 && (16 * bi + 4 * kq + r) >= remain;
#pragma unroll
      for (int bj = 0; bj < 2; ++bj) best[bj] = fmaxf(best[bj], off ? -FLT_MAX : acc[bi][bj][r]);
    }
}


// Document score from the per-lane maxima: max over the four kq groups, then sum over the
// q_len query tokens (lane group kq = 0 holds token 16 bj + i16 in best[bj]).
__device__ __forceinline__ float ms_finish(const float (&best)[2], int i16, int kq, int q_len) {
  float contrib = 0.f;
#pragma unroll
  for (int bj = 0; bj < 2; ++bj) {
    float b = best[bj];
    b = fmaxf(b, __uint_as_float(lane_xor<16>(__float_as_uint(b))));
    b = fmaxf(b, __uint_as_float(lane_xor<32>(__float_as_uint(b))));
    if (kq == 0 && 16 * bj + i16 < q_len) contrib += b;
  }
  return ms_wave_sum(contrib);
}

// The lane's fragment of a 32-row x 128-float operand in global memory: rows row0 + 16 b + i16
// (clamped to row_max), 16-B slots 4t + kq.
__device__ __forceinline__ void ms_load_frag(const float* __restrict__ base, long row0, long row_max, int i16, int kq,
                                             bool zero, f32x4 (&f)[2][8]) {
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    long row = row0 + 16 * b + i16;
    const bool out = zero && row > row_max;
    if (row > row_max) row = row_max;
    const float* p = base + (size_t)row * kDim + kq * 4;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p + 16 * t);
      f[b][t] = out ? f32x4{0.f, 0.f, 0.f, 0.f} : v;
    }
  }
}

// grid: (x = ceil(n_docs / 4), y = queries); one wave per document (1-7 queries: latency form), fp32-input form.
__global__ __launch_bounds__(256) void maxsim_scores_kernel(const float* __restrict__ D,
                                                             const long long* __restrict__ doc_ptr, long n_docs,
                                                             const float* __restrict__ Q, int q_len,
                                                             float* __restrict__ scores /*[nq, n_docs]*/) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long doc = (long)blockIdx.x * kMsWaves + wave;
  if (doc >= n_docs) return;  // whole wave exits together
  const int qi = blockIdx.y;
  const int i16 = lane & 15, kq = lane >> 4;

  f32x4 qf[2][8];  // query tokens past q_len are zero rows
  ms_load_frag(Q + (size_t)qi * q_len * kDim, 0, q_len - 1, i16, kq, true, qf);

  const long t_lo = doc_ptr[doc], t_hi = doc_ptr[doc + 1];
  const int len = (int)(t_hi - t_lo);
  float best[2] = {-FLT_MAX, -FLT_MAX};
  for (int tok0 = 0; tok0 < len; tok0 += 32) {
    f32x4 af[2][8];  // rows past the document end are clamped here and masked in ms_tile
    ms_load_frag(D, t_lo + tok0, t_hi - 1, i16, kq, false, af);
    if (len - tok0 <= 16)
      ms_tile<1>(af, qf, kq, len - tok0, best);
    else
      ms_tile<2>(af, qf, kq, len - tok0, best);
  }
  const float total = ms_finish(best, i16, kq, q_len);
  if (lane == 0) scores[(size_t)qi * n_docs + doc] = total;
}

// The same, split-fp16 form: fragments straight from the [hi | lo] image (rows past the end of the document read on
// into the next document's tokens — the image is padded by one tile — and are masked by ms_tile_h).
__global__ __launch_bounds__(256) void maxsim_scores_h_kernel(const unsigned char* __restrict__ img,
                                                               const long long* __restrict__ doc_ptr, long n_docs,
                                                               const float* __restrict__ Q, int q_len,
                                                               float* __restrict__ scores /*[nq, n_docs]*/,
                                                               float unscale_d) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long doc = (long)blockIdx.x * kMsWaves + wave;
  if (doc >= n_docs) return;
  const int qi = blockIdx.y;
  const int r32 = lane & 31, h = lane >> 5;
  h8 qh[8], ql[8];
  float unscale;
  ms_load_query_h(Q + (size_t)qi * q_len * kDim, q_len, true, r32, h, qh, ql, unscale);
  unscale *= unscale_d;
  const long t_lo = doc_ptr[doc];
  const int len = (int)(doc_ptr[doc + 1] - t_lo);
  const float total = ms_pair_doc_h(img, t_lo, len, qh, ql, r32, h, q_len, unscale);
  if (lane == 0) scores[(size_t)qi * n_docs + doc] = total;
}


// Blocked form for query batches: a block = 8 waves = 8 queries, and walks kMsDocs documents.
// The one-wave-per-(query, document) kernel above re-reads every document's tokens for every
// query (PMC, UCC-en step of 1 168 queries: 23-46 GB of L2-miss reads against 68 MB of
// algorithmic bytes); here a 32-token document tile is fetched ONCE per block with coalesced
// 16-B/lane loads into a double-buffered, XOR-swizzled 16-KiB LDS tile and feeds all eight
// queries' MFMAs (query fragments live in registers for the whole block); the next tile —
// across document boundaries — is in flight while the current one is multiplied.  Blocks that
// share a document group have consecutive ids (query group = fast grid index), so they run
// together and the group stays in every XCD's L2.  Same MFMA operands and k order as above:
// bit-identical scores.
constexpr int kMsQ = 8;     // queries (waves) per block
constexpr int kMsDocs = 8;  // documents per block

// LDS tile: token row j (0..31) at byte j*512, swizzled by tile_off<512> (a ds_read_b128 lane group reads slots 4t + kq
// and 4t + (kq ^ 1) of 16 distinct rows); a staging write of one row (32 consecutive threads) covers the row's 512 B.
__global__ __launch_bounds__(kMsQ * 64) void maxsim_scores_blocked_kernel(const float* __restrict__ D,
                                                                           const long long* __restrict__ doc_ptr,
                                                                           long n_docs, const float* __restrict__ Q,
                                                                           int nq, int q_len,
                                                                           float* __restrict__ scores /*[nq, n_docs]*/) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[2][32 * 512];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, kq = lane >> 4;
  const int qi = blockIdx.x * kMsQ + wave;
  const bool live = qi < nq;
  const long d0 = (long)blockIdx.y * kMsDocs;
  long d1 = d0 + kMsDocs;
  if (d1 > n_docs) d1 = n_docs;

  f32x4 qf[2][8];
  if (live) {
    ms_load_frag(Q + (size_t)qi * q_len * kDim, 0, q_len - 1, i16, kq, true, qf);
  } else {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int t = 0; t < 8; ++t) qf[b][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // loader role: two 16-B pieces per thread and tile (elements tid and tid + 512 of 1024)
  const int lrow0 = tid >> 5, lslot = tid & 31;  // rows lrow0 and lrow0 + 16
  long doc = d0;
  long t_lo = doc_ptr[doc];
  int len = (int)(doc_ptr[doc + 1] - t_lo);
  int tok0 = 0;
  f32x4 g[2];
#define AMDR_MS_LOAD(TLO, LEN, TOK0)                                                                   \
  _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                      \
    int j_ = (TOK0) + lrow0 + 16 * u;                                                                  \
    if (j_ >= (LEN)) j_ = (LEN)-1; /* rows past the document end are masked after the MFMAs */         \
    g[u] = *reinterpret_cast<const f32x4*>(D + (size_t)((TLO) + j_) * kDim + lslot * 4);                 \
  }
#define AMDR_MS_STAGE(BUF)                                                                             \
  _Pragma("unroll") for (int u = 0; u < 2; ++u)                                                        \
      *reinterpret_cast<f32x4*>(tile[BUF] + tile_off<512>(lrow0 + 16 * u, lslot)) = g[u];
  AMDR_MS_LOAD(t_lo, len, tok0)
  AMDR_MS_STAGE(0)
  __syncthreads();
  int buf = 0;
  float best[2] = {-FLT_MAX, -FLT_MAX};
  while (true) {
    // coordinates of the next tile (wave-uniform)
    long ndoc = doc;
    int ntok = tok0 + 32;
    long nt_lo = t_lo;
    int nlen = len;
    if (ntok >= len) {
      ndoc = doc + 1;
      ntok = 0;
      if (ndoc < d1) {
        nt_lo = doc_ptr[ndoc];
        nlen = (int)(doc_ptr[ndoc + 1] - nt_lo);
      }
    }
    const bool has_next = ndoc < d1;
    if (has_next) { AMDR_MS_LOAD(nt_lo, nlen, ntok) }

    f32x4 af[2][8];
    if (len - tok0 <= 16) {  // wave-uniform: the tail of a document fits one 16-token row block
#pragma unroll
      for (int t = 0; t < 8; ++t)
        af[0][t] = *reinterpret_cast<const f32x4*>(tile[buf] + tile_off<512>(i16, 4 * t + kq));
      ms_tile<1>(af, qf, kq, len - tok0, best);
    } else {
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int t = 0; t < 8; ++t)
          af[b][t] = *reinterpret_cast<const f32x4*>(tile[buf] + tile_off<512>(16 * b + i16, 4 * t + kq));
      ms_tile<2>(af, qf, kq, len - tok0, best);
    }
    if (ntok == 0) {  // last tile of this document
      const float total = ms_finish(best, i16, kq, q_len);
      if (live && lane == 0) scores[(size_t)qi * n_docs + doc] = total;
      best[0] = best[1] = -FLT_MAX;
    }
    if (!has_next) break;
    AMDR_MS_STAGE(buf ^ 1)
    __syncthreads();
    buf ^= 1;
    doc = ndoc;
    tok0 = ntok;
    t_lo = nt_lo;
    len = nlen;
  }
#undef AMDR_MS_LOAD
#undef AMDR_MS_STAGE
}

// ---- ring form of the blocked kernel (split-fp16 tiles) ---------------------------------------------------------
// A wave's 24 MFMAs of a split-fp16 tile take 768 cycles — less than one trip to L2 / the Infinity Cache — so the
// one-tile-ahead, register-staged pipeline of the kernel above cannot feed them.  Here the document tiles go through
// the LDS-DMA ring of lds_ring.hpp (protocol, waits and their reasons: there) with NBUF 16-KiB stages.  128 VGPRs and
// NBUF x 16 KiB of LDS: two blocks = four waves per SIMD per CU, so one block's barrier / DMA wait runs under the
// other's MFMAs.  Tried on the way (same-box A/B, scripts/ab_maxsim.py): 2 / 3 / 4 / 6 stages 2.55 / 2.31 / 2.24 /
// 2.44 ms per 1 168 UCC-en queries; 8 / 16 / 32 / 64 documents per block 2.27 / 2.23 / 2.24 / 2.37; a second fragment
// register set filled one tile ahead (254 VGPRs) +- 0.
// A stage is 16 pieces of 1 KiB (piece_offs, tile_swizzle.hpp) of whole token rows (512 B: the [hi | lo] image, 256: the
// hi-only image).  Rows past the end of a document read on into the next document's tokens (the images are padded by
// one tile at their end) and are masked after the MFMAs.
// A position in a block's tile sequence (wave-uniform): tiles of TOK tokens of documents d0 .. d1 - 1.
template <int TOK>
struct MsDocCursor {
  long doc, t_lo;
  int len, tok0;
  __device__ __forceinline__ void first(const long long* __restrict__ doc_ptr, long d0) {
    doc = d0;
    t_lo = doc_ptr[d0];
    len = (int)(doc_ptr[d0 + 1] - t_lo);
    tok0 = 0;
  }
  __device__ __forceinline__ void advance(const long long* __restrict__ doc_ptr, long d1) {
    tok0 += TOK;
    if (tok0 >= len) {
      doc += 1;
      tok0 = 0;
      if (doc < d1) {
        t_lo = doc_ptr[doc];
        len = (int)(doc_ptr[doc + 1] - t_lo);
      }
    }
  }
};

template <int NBUF>
__global__ __launch_bounds__(kMsQ * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void maxsim_scores_ring_kernel(const unsigned char* __restrict__ img,
                                                                        const long long* __restrict__ doc_ptr,
                                                                        long n_docs, int docs_per_block,
                                                                        const float* __restrict__ Q, int nq, int q_len,
                                                                        float* __restrict__ scores /*[nq, n_docs]*/,
                                                                        float unscale_d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ring[];  // [NBUF][32 * 512]
  constexpr int kStage = 32 * 512;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, h = lane >> 5;
  const int qi = blockIdx.x * kMsQ + wave;
  const bool live = qi < nq;
  const long d0 = (long)blockIdx.y * docs_per_block;
  long d1 = d0 + docs_per_block;
  if (d1 > n_docs) d1 = n_docs;

  h8 qh[8], ql[8];
  float unscale;
  ms_load_query_h(Q + (size_t)(live ? qi : 0) * q_len * kDim, q_len, live, r32, h, qh, ql, unscale);
  unscale *= unscale_d;

  // DMA role: pieces 2 wave, 2 wave + 1 of a tile (two token rows of 512 B each)
  long poff[2];
  piece_offs<2, 512>(2 * wave, lane, poff);
  // fragment read addresses: row r32, chunk 2 s + h (the lo part sits 256 B behind the hi part: slots c and 16 + c
  // differ in bit 4, which the XOR with row & 15 leaves alone)
  int foff[8];
#pragma unroll
  for (int st = 0; st < 8; ++st) foff[st] = tile_off<512>(r32, 2 * st + h);

  MsDocCursor<32> prod, cur;
  prod.first(doc_ptr, d0);
  cur = prod;
  int issued = 0, done = 0;
  auto produce = [&]() {
    if (prod.doc >= d1) return;
    ring_issue_tile<2>(img + (size_t)(prod.t_lo + prod.tok0) * 512, poff, ring + (issued % NBUF) * kStage + 2 * wave * 1024);
    ++issued;
    prod.advance(doc_ptr, d1);
  };
#pragma unroll
  for (int i = 0; i < NBUF - 1; ++i) produce();
  float best = -FLT_MAX;
  while (cur.doc < d1) {
    wait_tile<2, NBUF - 1>(issued - done - 1);  // this wave's pieces of tile `done`
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    produce();  // into the stage of tile done - 1
    const unsigned char* tile = ring + (done % NBUF) * kStage;
    h8 ah[8], al[8];
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      const unsigned char* fp = tile + foff[st];
      ah[st] = *reinterpret_cast<const h8*>(fp);
      al[st] = *reinterpret_cast<const h8*>(fp + 256);
    }
    const int remain = cur.len - cur.tok0;
    ms_tile_h(ah, al, qh, ql, h, remain, best);
    if (remain <= 32) {  // last tile of this document
      const float total = ms_finish_h(best, r32, h, q_len, unscale);
      if (live && lane == 0) scores[(size_t)qi * n_docs + cur.doc] = total;
      best = -FLT_MAX;
    }
    ++done;
    cur.advance(doc_ptr, d1);
  }
}

// ---- two-pass top-k: a cheap first pass picks the documents worth the full arithmetic ---------------------------
// `search` needs the k best documents, not every score.  Pass 1 scores every (query, document) with the hi parts only
// (ONE fp16 MFMA per block instead of three, a 256-byte-per-token image instead of 512: a third of the matrix cycles and
// half the bytes).  |a_hi . b_hi - a . b| <= (2^-10 + 2^-22) |a| |b| (each fp16 rounding is 2^-11 relative, per
// component), so a document's first-pass score is within
//     eps_q = [1.5 * 2^-10 * (sum_i |q'_i|) * max_token |d'| * 1.0001 + q_len * 256 * 2^-25] * unscale_q * unscale_d
// of its full-form score: q' = q * scale_q and d' = d * scale_d are the SCALED operands (largest |component| in
// [0.5, 1)), which is what fp16 rounds and what both norms are taken on (ms_split_query_wave, ms_tokmax_kernel) — the
// bracket is in scaled units and the two unscales carry it to the units of the scores exactly, as they carry the scores.
// (The 1.5 covers the fp32 accumulation and the full form's own 2e-6, the 1.0001 the fp32 rounding of the norms, the
// second term operands in fp16's subnormal range.)  The bound has NO scale range of its own: it holds wherever
// unscale_q * unscale_d is a normal fp32 number, i.e. wherever the scores are; outside (and for a query holding a NaN
// or an infinity) maxsim_select_kernel makes every document a candidate, which is the one-pass form.  (Until the norms
// were taken on the scaled operands, a store or a query below ~2^-75 squared to 0 and lost every true top-k document,
// and one above ~2^63 squared to infinity.)  If T is the k-th best
// first-pass score, every document that can be among the k best full-form scores — ties at the cut included — has a
// first-pass score >= T - 2 eps_q (at most k - 1 documents score above the k-th best s_k, hence T <= s_k + eps, and a
// top-k document has a >= s_k - eps >= T - 2 eps).  Pass 2 re-scores exactly those documents with the full form
// (the tile function of the one-pass kernels: the same bits) and the final top-k runs on the re-scored values:
// identical ids and scores by construction, and by test against the one-pass form.  On the UCC-en / Civil-Code-zh
// stores 11-13 of 591 / 1 260 documents per query pass the cut at k = 10 (about 90 at k = 80).  A query with more than
// `cap` candidates (mass near-ties) re-scores every document instead (maxsim_overflow_kernel).
// Pass 1: a ring kernel like the one above with 64-token tiles of the hi-only image (16-KiB stages again, half the
// barriers per document), no fma in the epilogue.

// Pass 1, two queries per wave.  PMC / arithmetic on the first form of pass 1 (one query per wave, 16 MFMAs and 16
// ds_read_b128 per tile; retired): a wave reads the whole 16-KiB tile from LDS for 16 MFMAs of 32 cycles — 16 waves per CU x 16 KiB per 2 048 pipe cycles = 125 B per clock, the LDS's whole bandwidth: it
// ran at half its matrix floor (1.0 ms against 0.52).  Here a wave keeps the hi fragments of TWO queries (64 VGPRs) and
// feeds both from one read of the tile: half the LDS bytes per MFMA.  A block = 4 waves = 8 queries (the tile is shared
// by as many queries as before), 3 stages = 48 KiB, three blocks per CU.
constexpr int kMsQ2 = 4;  // waves per block; 2 queries each

__device__ __forceinline__ void ms_load_query_img_hi(const unsigned char* __restrict__ img_q, int qi, int r32, int h,
                                                     h8 (&qh)[8]) {
  const unsigned char* p = img_q + ((size_t)qi * 32 + r32) * 512 + 16 * h;
#pragma unroll
  for (int st = 0; st < 8; ++st) qh[st] = *reinterpret_cast<const h8*>(p + 32 * st);
}

__device__ __forceinline__ float ms_max3(float a, float b, float c) {  // max(a, b, c) in one instruction (no NaNs reach it)
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

template <int NBUF>
__global__ __launch_bounds__(kMsQ2 * 64) __attribute__((amdgpu_waves_per_eu(3, NBUF == 2 ? 5 : 3))) void maxsim_hi2_ring_kernel(
    const unsigned char* __restrict__ img_hi, const long long* __restrict__ doc_ptr, long n_docs, int docs_per_block,
    int nq, int q_len, float* __restrict__ approx /*[nq, n_docs]*/, float unscale_d,
    const unsigned char* __restrict__ img_q /* the queries' split images (maxsim_split_queries_kernel) */,
    const float* __restrict__ unscale_q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ring[];  // [NBUF][64 * 256]
  constexpr int kStage = 64 * 256;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, h = lane >> 5;
  const int qa = (blockIdx.x * kMsQ2 + wave) * 2, qb = qa + 1;
  const bool live_a = qa < nq, live_b = qb < nq;
  const long d0 = (long)blockIdx.y * docs_per_block;
  long d1 = d0 + docs_per_block;
  if (d1 > n_docs) d1 = n_docs;

  // the fragments as maxsim_split_queries_kernel left them (a query is scored by n_docs / docs_per_block blocks: splitting
  // it in each of them was 10-20 % of this kernel's vector instructions); a dead wave takes query 0's
  h8 qha[8], qhb[8];
  ms_load_query_img_hi(img_q, live_a ? qa : 0, r32, h, qha);
  ms_load_query_img_hi(img_q, live_b ? qb : 0, r32, h, qhb);
  const float unscale_a = unscale_q[live_a ? qa : 0] * unscale_d;
  const float unscale_b = unscale_q[live_b ? qb : 0] * unscale_d;

  // DMA role: pieces 4 wave .. 4 wave + 3 of the tile's 16 (1 KiB = 4 token rows of 256 B each)
  long poff[4];
  piece_offs<4, 256>(4 * wave, lane, poff);
  int foff[8];
#pragma unroll
  for (int st = 0; st < 8; ++st) foff[st] = tile_off<256>(r32, 2 * st + h);

  MsDocCursor<64> prod, cur;
  prod.first(doc_ptr, d0);
  cur = prod;
  int issued = 0, done = 0;
  auto produce = [&]() {
    if (prod.doc >= d1) return;
    ring_issue_tile<4>(img_hi + (size_t)(prod.t_lo + prod.tok0) * 256, poff, ring + (issued % NBUF) * kStage + 4 * wave * 1024);
    ++issued;
    prod.advance(doc_ptr, d1);
  };
#pragma unroll
  for (int i = 0; i < NBUF - 1; ++i) produce();
  float best_a = -FLT_MAX, best_b = -FLT_MAX;
  while (cur.doc < d1) {
    wait_tile<4, NBUF - 1>(issued - done - 1);  // this wave's 4 pieces of tile `done`
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    produce();  // into the stage of tile done - 1
    const unsigned char* tile = ring + (done % NBUF) * kStage;
    const int remain = cur.len - cur.tok0;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      if (blk == 1 && remain <= 32) break;  // wave-uniform: the second 32-token row block holds no token of this document
      h8 a[8];
#pragma unroll
      for (int st = 0; st < 8; ++st) a[st] = *reinterpret_cast<const h8*>(tile + blk * (32 * 256) + foff[st]);
      f32x16 ca, cb;
#pragma unroll
      for (int j = 0; j < 16; ++j) ca[j] = cb[j] = 0.f;
#pragma unroll
      for (int st = 0; st < 8; ++st) {
        ca = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[st], qha[st], ca, 0, 0, 0);
        cb = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[st], qhb[st], cb, 0, 0, 0);
      }
      if (remain < 32 * (blk + 1)) {  // last row block of a document: rows >= remain are no tokens of it
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (32 * blk + mfma32_row(j, h) >= remain) ca[j] = cb[j] = -FLT_MAX;
      }
      // 16 values -> 1 per query and row block as EIGHT v_max3_f32 (hipcc fused only a quarter of the fmaxf pairs: 56
      // v_max per 32 MFMAs; the pass issued ~5 other vector instructions per MFMA with its matrix pipe busy half the
      // time: 975 -> 891 us per 1 168 UCC-en queries).  Tried after it and dropped: FOUR queries per wave (64 MFMAs per
      // tile read and barrier, 16 queries per tile, two waves per SIMD): 1.08 against 1.09 ms per hybrid step.  Also
      // tried and dropped: the fragment reads of the NEXT 32-token row block issued before the current block's 32 MFMAs
      // (the compiler's order here is two reads, s_waitcnt lgkmcnt(0), four MFMAs, eight times per tile) with a second
      // fragment set — 64 more VGPRs, two waves per SIMD, four ring stages: 1.136 against 1.101 ms per hybrid step, slower
      // at every block size.  Neither the reads per MFMA nor their latency is what keeps
      // the matrix pipe at half duty.
#pragma unroll
      for (int j = 0; j < 16; j += 2) {
        best_a = ms_max3(best_a, ca[j], ca[j + 1]);
        best_b = ms_max3(best_b, cb[j], cb[j + 1]);
      }
    }
    if (remain <= 64) {
      const float ta = ms_finish_h(best_a, r32, h, q_len, unscale_a);
      const float tb = ms_finish_h(best_b, r32, h, q_len, unscale_b);
      if (lane == 0) {
        if (live_a) approx[(size_t)qa * n_docs + cur.doc] = ta;
        if (live_b) approx[(size_t)qb * n_docs + cur.doc] = tb;
      }
      best_a = best_b = -FLT_MAX;
    }
    ++done;
    cur.advance(doc_ptr, d1);
  }
}

// One wave splits one query into the [hi | lo] image of the re-scoring pass (512 B per token row, 32 rows, rows past q_len
// zero) and stores its power-of-two unscale — the scale rule and ms_split of ms_load_query_h: identical fragments.  The
// re-scoring pass takes a query's fragments for every (document, query) item it serves, 15 k times per UCC-en batch:
// splitting them in the scoring wave each time cost ~500 vector instructions per item and wave.
// `norm_sum`: the sum of the SCALED token rows' Euclidean norms (rows x the query's power of two, as ms_split takes them:
// squares of raw components underflow to 0 for a query below ~2^-75 and overflow above ~2^63), which the candidate margin
// of the two-pass top-k is built on (maxsim_select_kernel) — the rows are in this wave's registers anyway.  A NaN or an
// infinity in the query makes it NaN or infinite (the scale of such a query is 1), which the select kernel reads as "no
// bound".
__device__ __forceinline__ void ms_split_query_wave(const float* __restrict__ Qq, int q_len, int lane,
                                                    unsigned char* __restrict__ img, float* __restrict__ unscale,
                                                    float* __restrict__ norm_sum) {
  // one pass over the query: lane holds (row, group of 8 components) g = lane + 64 it — 16 lanes per row, 4 rows per step
  float x[8][8];
  float m = 0.f, nsum = 0.f;
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int g = lane + 64 * it, row = g >> 4, grp = g & 15;
    if (row < q_len) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(Qq + (size_t)row * kDim + 8 * grp);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(Qq + (size_t)row * kDim + 8 * grp + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[it][j] = v0[j], x[it][4 + j] = v1[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) x[it][j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(x[it][j]));
  }
#pragma unroll
  for (int sft = 1; sft < 64; sft <<= 1) m = fmaxf(m, __shfl_xor(m, sft));
  const int e = pow2_exp(m);
  const float sc = pow2_scale(e);
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = x[it][j] * sc;  // what ms_split rounds
      ss += v * v;
    }
#pragma unroll
    for (int sft = 1; sft < 16; sft <<= 1) ss += __shfl_xor(ss, sft);  // the row's 16 lanes
    nsum += sqrtf(ss);  // (every lane of the row holds it; counted once below)
  }
  nsum += __shfl_xor(nsum, 16);  // the four rows of a step sit in the four 16-lane groups
  nsum += __shfl_xor(nsum, 32);
  if (lane == 0) {
    *unscale = pow2_scale(-e);
    *norm_sum = nsum;
  }
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int g = lane + 64 * it, row = g >> 4, grp = g & 15;
    h8 hi, lo;
    ms_split(x[it], sc, hi, lo);
    unsigned char* dst = img + (size_t)row * 512 + 16 * grp;
    *reinterpret_cast<h8*>(dst) = hi;
    *reinterpret_cast<h8*>(dst + 256) = lo;
  }
}

// Ahead of pass 1 (round 4), one wave per query: both passes take their query fragments from these images.
__global__ __launch_bounds__(256) void maxsim_split_queries_kernel(const float* __restrict__ Q, int nq, int q_len,
                                                                   unsigned char* __restrict__ img_q,
                                                                   float* __restrict__ unscale_out,
                                                                   float* __restrict__ norm_sum) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  ms_split_query_wave(Q + (size_t)q * q_len * kDim, q_len, threadIdx.x & 63, img_q + (size_t)q * 32 * 512,
                      unscale_out + q, norm_sum + q);
}

// Between the passes, one wave per query: T = the k-th best first-pass score, eps from the query's token norms, the
// list of documents with a first-pass score >= T - 2 eps (ascending ids, at most cap; more -> overflow).
__global__ __launch_bounds__(64) void maxsim_select_kernel(const float* __restrict__ approx, long n_docs, int q_len, int k,
                                                           int cap_sel, float d_norm_max /* of the scaled store */,
                                                           float unscale_d, int cap,
                                                           int* __restrict__ cand /*[nq, cap]*/, int* __restrict__ cnt,
                                                           int* __restrict__ overflow, int* __restrict__ dcnt,
                                                           int* __restrict__ dlist /*[n_docs][nq]*/, int nq,
                                                           const float* __restrict__ norm_sum /* with the split images */,
                                                           const float* __restrict__ unscale_in /* (split_queries) */) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  C32* buf = reinterpret_cast<C32*>(smem);
  const int lane = threadIdx.x & 63, q = blockIdx.x;
  const float* row = approx + (size_t)q * n_docs;
  WaveTopK<C32> tk;
  tk.init(buf, cap_sel, k);
  // T: short rows in registers (the slab top-k's selector: 47 -> ~20 us per 1 168 UCC-en queries together with the two
  // changes below), otherwise — and on mass ties at the cut — the staged selector
  int got = -1;
  if (k <= 64 && n_docs <= kSelectRowsMax && cap_sel >= 128) {
    if (n_docs <= 640)
      got = select_row<10>(row, 0, n_docs, k, lane, tk.buf);
    else if (n_docs <= 1280)
      got = select_row<20>(row, 0, n_docs, k, lane, tk.buf);
    else
      got = select_row<32>(row, 0, n_docs, k, lane, tk.buf);
  }
  if (got >= 0) {
    tk.cnt = got;
  } else {
    wave_topk_sweep(tk, row, 0, n_docs, lane);
  }
  wave_lds_fence();
  const float T = tk.cnt >= k ? tk.buf[k - 1].score() : -FLT_MAX;  // fewer than k documents: every one is a candidate
  wave_lds_fence();
  // eps in SCALED units (norms of the scaled operands: nsum <= 32 sqrt(128), d_norm_max <= sqrt(128), whatever the
  // magnitudes of store and query), then times the two unscales — the powers of two that the scoring kernels undo on the
  // scores themselves (maxsim_split_queries_kernel).  No bound — every document is a candidate, the overflow path or the
  // items re-score them all and the result is the one-pass form's — where the arithmetic gives none: a NaN or an infinity
  // in the query (nsum NaN / infinite), or unscales whose product is no normal fp32 number (then the scores themselves
  // have left fp32's range).
  const float nsum = norm_sum[q], unscale = unscale_in[q] * unscale_d;
  const float eps = (1.5f * 9.765625e-4f * nsum * d_norm_max * 1.0001f +
                     (float)q_len * 256.f * 2.98023224e-8f /* operands in fp16's subnormal range */) * unscale;
  const bool bound = unscale >= FLT_MIN && eps <= FLT_MAX;  // (false on NaN)
  const float thr = (T == -FLT_MAX || !bound) ? -FLT_MAX : T - 2.f * eps;
  int n = 0;
  for (long base = 0; base < n_docs; base += 64) {
    const long d = base + lane;
    const bool v = d < n_docs;
    const float a = v ? row[d] : 0.f;
    const bool pass = v && (a >= thr || thr == -FLT_MAX);
    const unsigned long long m = __ballot(pass);
    const int at = n + __popcll(lane ? (m & (~0ull >> (64 - lane))) : 0ull);
    if (pass && at < cap) cand[(size_t)q * cap + at] = (int)d;
    n += __popcll(m);
  }
  if (lane == 0) {
    overflow[q] = n > cap ? 1 : 0;
    cnt[q] = n > cap ? 0 : n;
  }
  if (n <= cap) {
    // round 4: the re-scoring pass walks the pairs BY DOCUMENT — the query joins the list of each of its candidates
    // (row d of dlist, one slot per query at most: no offsets to compute, no second pass to fill them)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's own list, just written
    for (int j = lane; j < n; j += 64) {
      const int d = cand[(size_t)q * cap + j];
      dlist[(size_t)d * nq + atomicAdd(dcnt + d, 1)] = q;  // the order inside a document's list does not matter
    }
  }
}

// Full-form score of one (query, document) by ONE wave, the document's tiles staged through a wave-private 16-KiB LDS
// stage by LDS-DMA (16 pieces of 1 KiB per tile: whole 512-byte token rows per request).  The first version
// fetched the MFMA fragments straight from global memory, as maxsim_scores_h_kernel does for a single query: 16-byte
// pieces of 32 different rows per load instruction — 15 k candidate pairs per launch then moved ~8x their bytes through
// the L1s and pass 2 took as long as pass 1 (0.98 ms).  Same tile function, same operands: the same bits.
__device__ __forceinline__ float ms_exact_doc_lds(const unsigned char* __restrict__ img,
                                                  const long long* __restrict__ doc_ptr, long doc, const h8 (&qh)[8],
                                                  const h8 (&ql)[8], int lane, int q_len, float unscale,
                                                  unsigned char* stage /* this wave's 16 KiB */) {
  const int r32 = lane & 31, h = lane >> 5;
  const long t_lo = doc_ptr[doc];
  const int len = (int)(doc_ptr[doc + 1] - t_lo);
  long poff[16];  // the whole tile is this wave's
  piece_offs<16, 512>(0, lane, poff);
  int foff[8];
#pragma unroll
  for (int st = 0; st < 8; ++st) foff[st] = tile_off<512>(r32, 2 * st + h);
  float best = -FLT_MAX;
  for (int tok0 = 0; tok0 < len; tok0 += 32) {
    wait_lgkm0();  // the fragment reads of the previous tile are done: the stage may be refilled
    ring_issue_tile<16>(img + (size_t)(t_lo + tok0) * 512, poff, stage);
    wait_vm0();  // the tile has landed (the other waves of the CU cover the wait)
    asm volatile("" ::: "memory");
    h8 ah[8], al[8];
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      const unsigned char* fp = stage + foff[st];
      ah[st] = *reinterpret_cast<const h8*>(fp);
      al[st] = *reinterpret_cast<const h8*>(fp + 256);
    }
    ms_tile_h(ah, al, qh, ql, h, len - tok0, best);
  }
  return ms_finish_h(best, r32, h, q_len, unscale);
}

__device__ __forceinline__ void ms_load_query_img(const unsigned char* __restrict__ img_q, int qi, int r32, int h,
                                                  h8 (&qh)[8], h8 (&ql)[8]) {
  const unsigned char* p = img_q + ((size_t)qi * 32 + r32) * 512 + 16 * h;
#pragma unroll
  for (int st = 0; st < 8; ++st) {
    qh[st] = *reinterpret_cast<const h8*>(p + 32 * st);
    ql[st] = *reinterpret_cast<const h8*>(p + 256 + 32 * st);
  }
}

// ---- Pass 2, round 4: the candidate pairs grouped BY DOCUMENT ------------------------------------------------------
// One wave per pair shared nothing: 15 k pairs x a document image of ~80 KB = 0.93 GB through the fabric for 68 MB of
// token store (PMC, profiles/r03_pmc.md), 145 us.  A document is a candidate of ~25 queries on the serving corpora, so
// the pairs are inverted to per-document query lists and a block takes (document, 8 of its queries): the document's
// tiles go ONCE through the block's LDS ring (the one-pass ring kernel's, same fragments, same tile function: the same
// bits) and feed 8 queries' MFMAs.
//   maxsim_select_kernel        also appends the query to the list of each of its candidate documents (dlist, dcnt)
//   maxsim_items_kernel         the item table, longest documents first (the first version of this round also
//                               prefix-summed per-document offsets and filled a packed pair list with a third kernel:
//                               fixed-stride lists written by the select kernel itself took both away)
//   maxsim_rescore_ring_kernel  persistent blocks of 8 waves walk the items
struct MsItem {  // one unit of the re-scoring pass: a document (its token range) and up to 8 of its queries
  int doc, p0, cnt, len;
  long long t_lo, pad;
};
__global__ __launch_bounds__(256) void maxsim_items_kernel(const int* __restrict__ dcnt, long n_docs,
                                                           const long long* __restrict__ doc_ptr,
                                                           int* __restrict__ n_items, MsItem* __restrict__ items) {
  __shared__ int bucket[16], bpos[16];
  if (threadIdx.x < 16) bucket[threadIdx.x] = 0;
  __syncthreads();
  // items per cost class: a document's items (8 of its queries each) cost its tiles
  for (long i = threadIdx.x; i < n_docs; i += 256) {
    const int it = (dcnt[i] + kMsQ - 1) / kMsQ;
    if (it) {
      const int tiles = (int)((doc_ptr[i + 1] - doc_ptr[i] + 31) >> 5);
      atomicAdd(&bucket[15 - (tiles < 15 ? tiles : 15)], it);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int at = 0;
    for (int c = 0; c < 16; ++c) {
      bpos[c] = at;
      at += bucket[c];
    }
    *n_items = at;
  }
  __syncthreads();
  // The item table, LONGEST DOCUMENTS FIRST (a counting sort over the tile count): the re-scoring blocks take items
  // b, b + grid, b + 2 grid, ... — dealt from a descending order every block's share costs about the same.  In document
  // order a block's 4-5 items ranged from 1 to 7 tiles each and the waves were alive for 65 % of the launch (SQ_WAVE_CYCLES).
  // One 32-byte descriptor per item (p0 = its first slot in the document's query list): a block reads it instead of
  // searching offsets.
  for (long i = threadIdx.x; i < n_docs; i += 256) {
    const int v = dcnt[i];
    const int it = (v + kMsQ - 1) / kMsQ;
    if (!it) continue;
    const long long t_lo = doc_ptr[i];
    const int len = (int)(doc_ptr[i + 1] - t_lo);
    const int tiles = (len + 31) >> 5;
    const int at = atomicAdd(&bpos[15 - (tiles < 15 ? tiles : 15)], it);
    for (int c = 0; c < it; ++c)
      items[at + c] = MsItem{(int)i, c * kMsQ, v - c * kMsQ < kMsQ ? v - c * kMsQ : kMsQ, len, t_lo, 0};
  }
}

template <int NBUF>
__global__ __launch_bounds__(kMsQ * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void maxsim_rescore_ring_kernel(
    const unsigned char* __restrict__ img, long n_docs, const unsigned char* __restrict__ img_q,
    const float* __restrict__ unscale_q, int q_len, float unscale_d, const MsItem* __restrict__ item_tab,
    const int* __restrict__ n_items, const int* __restrict__ dlist /*[n_docs][nq]: a document's queries*/, int nq,
    float* __restrict__ exact /*[nq, n_docs]*/) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ring[];  // [NBUF][32 * 512]
  constexpr int kStage = 32 * 512;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, h = lane >> 5;
  long poff[2];  // DMA role of this wave: pieces 2 wave, 2 wave + 1 of a tile (maxsim_scores_ring_kernel)
  piece_offs<2, 512>(2 * wave, lane, poff);
  int foff[8];
#pragma unroll
  for (int st = 0; st < 8; ++st) foff[st] = tile_off<512>(r32, 2 * st + h);
  const int items = *n_items;
  const int stride = (int)gridDim.x;
  auto desc_of = [&](int it) { return it < items ? item_tab[it] : MsItem{0, 0, 0, 0, 0, 0}; };
  // The block's items (blockIdx.x, + gridDim.x, ...) are ONE stream of tiles through the ring: the producer cursor runs up
  // to NBUF - 1 tiles ahead of the consumer ACROSS item boundaries (a document has ~5 tiles: restarting the ring per item
  // exposed a memory latency per item and left the ring mostly empty).  Consumer look-ahead: the descriptor of the item
  // after next and this wave's query of the next item are requested while the current item is multiplied.
  MsItem c_cur = desc_of(blockIdx.x), c_nxt = desc_of(blockIdx.x + stride);
  int qi_c = wave < c_cur.cnt ? dlist[(size_t)c_cur.doc * nq + c_cur.p0 + wave] : 0;
  MsItem p_cur = c_cur, p_nxt = c_nxt;
  int p_item = blockIdx.x, p_tile = 0;
  int issued = 0, done = 0;
  auto produce = [&]() {
    while (p_item < items && p_tile >= ((p_cur.len + 31) >> 5)) {  // the producer moves on to its next item
      p_item += stride;
      p_cur = p_nxt;
      p_nxt = desc_of(p_item + stride);
      p_tile = 0;
    }
    if (p_item >= items) return;
    ring_issue_tile<2>(img + (size_t)(p_cur.t_lo + 32 * p_tile) * 512, poff, ring + (issued % NBUF) * kStage + 2 * wave * 1024);
    ++issued;
    ++p_tile;
  };
#pragma unroll
  for (int i = 0; i < NBUF - 1; ++i) produce();
  for (int item = blockIdx.x; item < items; item += stride) {
    const bool live = wave < c_cur.cnt;
    const int qi = qi_c, len = c_cur.len, ntiles = (c_cur.len + 31) >> 5;
    h8 qh[8], ql[8];
    ms_load_query_img(img_q, qi, r32, h, qh, ql);  // (a dead wave reads query 0's: its result is never stored)
    const float unscale = unscale_q[qi] * unscale_d;
    // vmcnt counts in issue order: with the fragments (the youngest requests) in, every DMA issued so far has landed
    wait_vm0();
    asm volatile("" ::: "memory");
    const int safe = issued;  // tiles below this index need no further wait by this wave
    const MsItem nn = desc_of(item + 2 * stride);
    const int qi_n = wave < c_nxt.cnt ? dlist[(size_t)c_nxt.doc * nq + c_nxt.p0 + wave] : 0;
    float best = -FLT_MAX;
    for (int t = 0; t < ntiles; ++t) {
      wait_lgkm0();  // the fragment reads of the previous tile
      if (done >= safe) wait_vm<2, 3>(issued - done - 1);  // this wave's pieces of tile `done`
      __builtin_amdgcn_s_barrier();  // everybody's pieces of tile `done` are in; tile done - 1 has been read by all
      asm volatile("" ::: "memory");
      produce();                     // into the stage of tile done - 1
      if (live) {  // wave-uniform: a wave without a query of this item (a document's last, partly filled item) only moves tiles
        const unsigned char* tile = ring + (done % NBUF) * kStage;
        h8 ah[8], al[8];
#pragma unroll
        for (int st = 0; st < 8; ++st) {
          const unsigned char* fp = tile + foff[st];
          ah[st] = *reinterpret_cast<const h8*>(fp);
          al[st] = *reinterpret_cast<const h8*>(fp + 256);
        }
        ms_tile_h(ah, al, qh, ql, h, len - 32 * t, best);
      }
      ++done;
    }
    const float total = ms_finish_h(best, r32, h, q_len, unscale);
    if (live && lane == 0) exact[(size_t)qi * n_docs + c_cur.doc] = total;
    c_cur = c_nxt;
    c_nxt = nn;
    qi_c = qi_n;
  }
}

// a query whose candidate list overflowed: every document, full form (rare: mass near-ties at the cut)
__global__ __launch_bounds__(256) void maxsim_overflow_kernel(const unsigned char* __restrict__ img,
                                                              const long long* __restrict__ doc_ptr, long n_docs,
                                                              const float* __restrict__ Q, int q_len, float unscale_d,
                                                              const int* __restrict__ overflow, float* __restrict__ exact) {
  extern __shared__ __attribute__((aligned(16))) unsigned char stages[];
  const int q = blockIdx.x;
  if (!overflow[q]) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  h8 qh[8], ql[8];
  float unscale;
  ms_load_query_h(Q + (size_t)q * q_len * kDim, q_len, true, lane & 31, lane >> 5, qh, ql, unscale);
  for (long doc = wave; doc < n_docs; doc += kMsWaves) {
    const float total = ms_exact_doc_lds(img, doc_ptr, doc, qh, ql, lane, q_len, unscale * unscale_d, stages + wave * 16384);
    if (lane == 0) exact[(size_t)q * n_docs + doc] = total;
  }
}

// Per-query top-k over a dense fp32 score row (one block per query).
__global__ __launch_bounds__(256) void rowscores_topk_kernel(const float* __restrict__ scores, long n, int k, int cap,
                                                              float* __restrict__ out_scores,
                                                              long long* __restrict__ out_ids) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const TopkLds<C32> L(smem, kMsWaves, cap);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qi = blockIdx.x;
  const float* row = scores + (size_t)qi * n;
  WaveTopK<C32> tk;
  tk.init(L.list(wave), cap, k);
  for (long base = (long)wave * 64; base < n; base += (long)kMsWaves * 64) {
    long i = base + lane;
    bool v = i < n;
    C32 c = v ? C32::make(row[i], (u32)i) : C32::pad();
    tk.push_lanes(c, v, lane);
  }
  tk.finalize(lane);
  block_combine_topk(tk, L, kMsWaves, wave, lane);
  if (wave == 0) topk_store(tk.buf, tk.cnt, k, lane, out_scores + (size_t)qi * k, out_ids + (size_t)qi * k);
}

// The two-pass top-k's last step, one wave per query: only a query's candidates (<= cap, 64 for k <= 32) carry a
// re-scored value, so the k best are found among THEM — one register sort — instead of scanning the n_docs-long row that
// the select kernel had to fill with -FLT_MAX first (rowscores_topk_kernel: 18 us per 1 168 UCC-en queries, + 591 stores per
// query in the select kernel).  A query whose candidate list overflowed was re-scored in full (maxsim_overflow_kernel):
// its whole row is ranked.  Same keys (score, lower id first), same result.
__global__ __launch_bounds__(256) void maxsim_final_topk_kernel(const float* __restrict__ exact, long n_docs, int nq,
                                                                 const int* __restrict__ cand, const int* __restrict__ cnt,
                                                                 const int* __restrict__ overflow, int cap, int k,
                                                                 int cap_sel, float* __restrict__ out_scores,
                                                                 long long* __restrict__ out_ids) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * 4 + wave;
  if (q >= nq) return;
  const float* row = exact + (size_t)q * n_docs;
  const bool whole = overflow[q] != 0;
  const int n = whole ? 0 : cnt[q];
  if (!whole && cap <= 64 && k <= 64) {
    C32 c = C32::pad();
    if (lane < n) {
      const int d = cand[(size_t)q * cap + lane];
      c = C32::make(row[d], (u32)d);
    }
    c = wave_sort64_desc(c, lane);
    if (lane < k) topk_store(c, lane < n, lane, out_scores + (size_t)q * k, out_ids + (size_t)q * k);
    return;
  }
  WaveTopK<C32> tk;
  tk.init(reinterpret_cast<C32*>(smem) + (size_t)wave * cap_sel, cap_sel, k);
  const long total = whole ? n_docs : (long)n;
  for (long base = 0; base < total; base += 64) {
    const long i = base + lane;
    const bool v = i < total;
    long d = 0;
    if (v) d = whole ? i : (long)cand[(size_t)q * cap + i];
    tk.push_lanes(v ? C32::make(row[d], (u32)d) : C32::pad(), v, lane);
  }
  tk.finalize(lane);
  topk_store(tk.buf, tk.cnt, k, lane, out_scores + (size_t)q * k, out_ids + (size_t)q * k);
}

}  // namespace amdr

using namespace amdr;

namespace amdr {
int maxsim_raw(amdr_maxsim_t* h, MaxsimRaw* out) {
  out->img = h->img;
  out->doc_ptr = h->doc_ptr;
  out->n_docs = (long)h->n_docs;
  out->unscale_d = 1.f / h->d_scale;
  out->device = h->device;
  return AMDR_OK;
}
}  // namespace amdr
namespace {

// What the workspace arithmetic depends on: the corpus size and whether the store has its split-fp16 images (a store
// holding a NaN / infinity has none).  amdr_maxsim_workspace_plan builds one from the shape alone.
struct MsShape {
  int64_t n_docs;
  bool img, img_hi;
};
MsShape ms_shape(const amdr_maxsim* h) { return MsShape{h->n_docs, h->img != nullptr, h->img_hi != nullptr}; }

// ---- the route: which form a call takes, decided once ---------------------------------------------------------------------
// Everything about a call that is fixed before its first launch.  The three pins are read here, once per call (tests set
// them between calls of one process: nothing is kept from one call to the next): AMDR_MAXSIM_F16X3=0 the fp32-input
// forms, AMDR_MAXSIM_TWOPASS=0 one pass, AMDR_MAXSIM_DOCS the documents per block of the ring kernels.
enum class MsForm {
  TwoPass,   // top-k only: hi-only pass 1 over every document, candidates re-scored in full, top-k over the candidates
  Ring,      // maxsim_scores_ring_kernel: split-fp16 tiles shared by 8 queries through the LDS ring
  Blocked,   // maxsim_scores_blocked_kernel: fp32-input tiles shared by 8 queries
  PairHalf,  // maxsim_scores_h_kernel: one wave per (query, document), split-fp16
  PairF32,   // maxsim_scores_kernel: one wave per (query, document), fp32-input
};
struct MsRoute {
  MsForm form;
  int docs;  // documents per block of the pass that walks them (TwoPass: pass 1; the pair forms: one per wave), with
             // the grid limit of 65 535 blocks in y applied
};
// Ring depths and blocks per CU: constants of the route (template arguments of the kernels; amdr_maxsim_create sizes
// the kernels' dynamic LDS from them).
constexpr int kRing = 4;   // one-pass ring: LDS stages (2 / 3 / 4 / 6 measured; best: 4)
constexpr int kRing1 = 3;  // pass 1: three blocks per CU
// Pass 2 (same process, interleaved, 1 168 UCC-en queries, whole channel):
// 4 stages x 2 blocks per CU (64 KB of LDS each: 4 waves per SIMD) 0.8916 ms; 3 x 3: 0.8903; 2 x 4 (8 waves per SIMD):
// 0.8837; 2 stages with 6 / 8 blocks per CU in the grid (the items then outnumber the blocks by little: the hardware
// deals them) 0.8815 / 0.8793.  What the deeper ring bought inside a block, twice the resident waves buy across
// blocks: the per-item latencies (descriptor -> query list -> query fragments -> first tile) overlap another
// block's products.  Civil-Code-zh: 1.1017 -> 1.0947.
constexpr int kRing2 = 2, kBlocks2 = 8;
constexpr int kPairLds = kMsWaves * 16384;  // maxsim_overflow_kernel: a 16-KiB stage per wave
// Documents per block.  One-pass ring: 16 (measured best).  Pass 1 (round 4, scripts/ab_maxsim_env.py — variants
// interleaved in one process, channel ms): UCC-en 16 / 24 / 29 / 32: 0.891 / 0.884 / 0.897 / 0.903, Civil-Code-zh 16 / 24 /
// 32 / 48 / 64: 1.161 / 1.161 / 1.163 / 1.101* / 1.095* (*another box: 32 = 1.090).  Whole rounds of the chip's block slots
// (29 documents: 3 066 blocks = 3.99 rounds of 768, against 3.6 at 32) bought nothing, nor did 2 or 4 ring stages (5 or
// 2 blocks per CU instead of 3: -0.5 % / +2 %): the pass sits on a plateau that scheduling does not move.
constexpr int kDocsRing = 16, kDocsPass1 = 24;

MsRoute ms_route(const MsShape& s, int nq, int k, bool want_topk) {
  auto off = [](const char* name) { const char* e = getenv(name); return e && e[0] == '0'; };
  const bool half = s.img && !off("AMDR_MAXSIM_F16X3");  // split-fp16 MFMA form (default) / fp32-input form
  const bool batch = nq >= kMsQ;                         // batches: document tiles shared by 8 queries through LDS
  const char* dpb = getenv("AMDR_MAXSIM_DOCS");
  auto docs = [&](long d) {
    if (dpb && atoi(dpb) > 0) d = atoi(dpb);
    while (ceil_div(s.n_docs, d) > 65535) d *= 2;
    return (int)d;
  };
  // the two-pass top-k: batches on the split-fp16 form, k small against the corpus
  if (want_topk && half && batch && s.img_hi && (int64_t)4 * k <= s.n_docs && !off("AMDR_MAXSIM_TWOPASS"))
    return MsRoute{MsForm::TwoPass, docs(kDocsPass1)};
  if (batch && half) return MsRoute{MsForm::Ring, docs(kDocsRing)};
  if (batch && ceil_div(s.n_docs, kMsDocs) <= 65535) return MsRoute{MsForm::Blocked, kMsDocs};
  return MsRoute{half ? MsForm::PairHalf : MsForm::PairF32, kMsWaves};
}

int ms_cand_cap(int k) {
  const int c = next_pow2(2 * k);
  return c < 64 ? 64 : c;
}

// ---- the workspace ---------------------------------------------------------------------------------------------------------
constexpr size_t kMsAlign = 256;  // of the row blocks and of the total
size_t ms_rows_bytes(int64_t n_docs, int nq) {  // the score rows [nq, n_docs]: all a one-pass call uses
  return ((size_t)nq * n_docs * sizeof(float) + kMsAlign - 1) / kMsAlign * kMsAlign;
}
// The two-pass workspace: the byte offset of every region, in the order ms_run's kernels meet them, and the end.  ms_run
// takes its pointers from here, amdr_maxsim_reserve / amdr_maxsim_workspace_plan their sizes: there is no second sum.
struct MsLayout {
  size_t approx, exact, dlist, cand, cnt, ovf, dcnt, n_items, items, img_q, unscale_q, nsum_q, bytes;
};
MsLayout ms_layout(int64_t n_docs, int nq, int k) {
  MsLayout L;
  size_t at = 0;
  auto take = [&](size_t bytes, size_t align) { const size_t o = (at + align - 1) / align * align; at = o + bytes; return o; };
  const size_t n = (size_t)n_docs, q = (size_t)nq, cap = (size_t)ms_cand_cap(k), row = q * n * sizeof(float);
  L.approx = take(row, kMsAlign);                  // float [nq, n_docs]: first-pass scores
  L.exact = take(row, kMsAlign);                   // float [nq, n_docs]: re-scored scores
  L.dlist = take(row, kMsAlign);                   // int [n_docs][nq]: the queries a document is a candidate of
  L.cand = take(q * cap * sizeof(int), kMsAlign);  // int [nq, cap]: a query's candidates
  L.cnt = take(q * sizeof(int), sizeof(int));      // int [nq]: their number (0: the list overflowed)
  L.ovf = take(q * sizeof(int), sizeof(int));      // int [nq]: the list overflowed
  L.dcnt = take(n * sizeof(int), sizeof(int));     // int [n_docs]: candidates per document
  L.n_items = take(sizeof(int), sizeof(int));      // items of the re-scoring pass
  // 32-byte descriptors: a document that c queries take has ceil(c / 8) <= c / 8 + 1 items, nq * cap pairs at most
  L.items = take((n + q * cap / kMsQ) * sizeof(MsItem), sizeof(MsItem));
  L.img_q = take(q * 32 * 512, kMsAlign);  // the queries' split images (16-byte fragment loads)
  L.unscale_q = take(q * sizeof(float), sizeof(float));  // float [nq]: their power-of-two scales
  L.nsum_q = take(q * sizeof(float), sizeof(float));     // float [nq]: the sums of their token norms
  L.bytes = take(0, kMsAlign);
  return L;
}
size_t ms_workspace_bytes(const MsShape& s, const MsRoute& r, int nq, int k) {
  return r.form == MsForm::TwoPass ? ms_layout(s.n_docs, nq, k).bytes : ms_rows_bytes(s.n_docs, nq);
}
// what amdr_maxsim_reserve(nq_max, k_max) sizes: the maximum over every call within it.  The form depends on k (a call
// with 4 k <= n_docs takes the two-pass layout, three row blocks + the query images, a deeper one the one-pass rows), so
// every depth <= k_max is visited; every term grows with nq and a batch of >= kMsQ queries is two-pass whenever a
// smaller one is, so nq_max covers every smaller batch.
size_t ms_reserve_bytes(const MsShape& s, int nq_max, int k_max) {
  size_t need = 0;
  for (int k = 1; k <= k_max; ++k) {
    const size_t b = ms_workspace_bytes(s, ms_route(s, nq_max, k, true), nq_max, k);
    need = b > need ? b : need;
  }
  return need;
}

#define AMDR_MS_LAUNCH(...) do { hipLaunchKernelGGL(__VA_ARGS__); AMDR_HIP(hipGetLastError()); } while (0)

int ms_run_two_pass(amdr_maxsim* h, const MsRoute& r, const float* Q_dev, int nq, int q_len, int k, const DevBuf& ws,
                    float* scores_dev, int64_t* ids_dev, hipStream_t st) {
  const float unscale_d = 1.f / h->d_scale;
  const long n = (long)h->n_docs;
  const MsLayout L = ms_layout(h->n_docs, nq, k);
  unsigned char *w = ws.as<unsigned char>(), *img_q = w + L.img_q;
  float *approx = (float*)(w + L.approx), *exact = (float*)(w + L.exact), *unscale_q = (float*)(w + L.unscale_q);
  float* nsum_q = (float*)(w + L.nsum_q);
  int *dlist = (int*)(w + L.dlist), *cand = (int*)(w + L.cand), *cnt = (int*)(w + L.cnt), *ovf = (int*)(w + L.ovf);
  int *dcnt = (int*)(w + L.dcnt), *n_items = (int*)(w + L.n_items);
  MsItem* items = (MsItem*)(w + L.items);
  const int cap = ms_cand_cap(k), cap_sel = topk_cap(k);
  AMDR_MS_LAUNCH(maxsim_split_queries_kernel, dim3(ceil_div(nq, 4)), dim3(256), 0, st, Q_dev, nq, q_len, img_q, unscale_q,
                 nsum_q);
  AMDR_MS_LAUNCH((maxsim_hi2_ring_kernel<kRing1>), dim3(ceil_div(nq, 2 * kMsQ2), ceil_div(n, r.docs)), dim3(kMsQ2 * 64),
                 kRing1 * 16384, st, h->img_hi, h->doc_ptr, n, r.docs, nq, q_len, approx, unscale_d, img_q, unscale_q);
  AMDR_HIP(hipMemsetAsync(dcnt, 0, (size_t)n * sizeof(int), st));
  AMDR_MS_LAUNCH(maxsim_select_kernel, dim3(nq), dim3(64), (size_t)cap_sel * sizeof(C32), st, approx, n, q_len, k, cap_sel,
                 h->d_norm_max, unscale_d, cap, cand, cnt, ovf, dcnt, dlist, nq, nsum_q, unscale_q);
  AMDR_MS_LAUNCH(maxsim_items_kernel, dim3(1), dim3(256), 0, st, dcnt, n, h->doc_ptr, n_items, items);
  AMDR_MS_LAUNCH((maxsim_rescore_ring_kernel<kRing2>), dim3(kBlocks2 * h->cus), dim3(kMsQ * 64), kRing2 * 16384, st, h->img,
                 n, img_q, unscale_q, q_len, unscale_d, items, n_items, dlist, nq, exact);
  AMDR_MS_LAUNCH(maxsim_overflow_kernel, dim3(nq), dim3(256), kPairLds, st, h->img, h->doc_ptr, n, Q_dev, q_len, unscale_d,
                 ovf, exact);
  AMDR_MS_LAUNCH(maxsim_final_topk_kernel, dim3(ceil_div(nq, 4)), dim3(256), (size_t)4 * cap_sel * sizeof(C32), st, exact, n,
                 nq, cand, cnt, ovf, cap, k, cap_sel, scores_dev, (long long*)ids_dev);
  return AMDR_OK;
}

// The launches of one call on route r, in workspace ws (sized by ms_workspace_bytes for the same route).
int ms_run(amdr_maxsim* h, const MsRoute& r, const float* Q_dev, int nq, int q_len, int k, const DevBuf& ws,
           float* scores_dev, int64_t* ids_dev, hipStream_t st) {
  const size_t need = ms_workspace_bytes(ms_shape(h), r, nq, k);
  AMDR_REQUIRE(need <= ws.cap, "maxsim: a call of %zu bytes in a workspace of %zu", need, ws.cap);
  const float unscale_d = 1.f / h->d_scale;
  const long n = (long)h->n_docs;
  float* full_dev = ws.as<float>();
  switch (r.form) {  // (ring, blocked and two-pass forms: the batch in the grid's x, <= 65 535 document blocks in y by ms_route)
    case MsForm::Ring:
      AMDR_MS_LAUNCH((maxsim_scores_ring_kernel<kRing>), dim3(ceil_div(nq, kMsQ), ceil_div(n, r.docs)), dim3(kMsQ * 64),
                     kRing * 16384, st, h->img, h->doc_ptr, n, r.docs, Q_dev, nq, q_len, full_dev, unscale_d);
      break;
    case MsForm::Blocked:
      AMDR_MS_LAUNCH(maxsim_scores_blocked_kernel, dim3(ceil_div(nq, kMsQ), ceil_div(n, r.docs)), dim3(kMsQ * 64), 0, st, h->D,
                     h->doc_ptr, n, Q_dev, nq, q_len, full_dev);
      break;
    case MsForm::PairHalf:  // the pair forms carry the batch in the grid's y: pieces (grid_y_pieces)
    case MsForm::PairF32: {
      const int rc = grid_y_pieces(nq, [&](int q0, int m) -> int {
        const float* Qp = Q_dev + (size_t)q0 * q_len * kDim;
        float* out = full_dev + (size_t)q0 * n;
        if (r.form == MsForm::PairHalf)
          AMDR_MS_LAUNCH(maxsim_scores_h_kernel, dim3(ceil_div(n, r.docs), m), dim3(256), 0, st, h->img, h->doc_ptr, n, Qp,
                         q_len, out, unscale_d);
        else
          AMDR_MS_LAUNCH(maxsim_scores_kernel, dim3(ceil_div(n, r.docs), m), dim3(256), 0, st, h->D, h->doc_ptr, n, Qp, q_len,
                         out);
        return AMDR_OK;
      });
      if (rc) return rc;
      break;
    }
    case MsForm::TwoPass:
      return ms_run_two_pass(h, r, Q_dev, nq, q_len, k, ws, scores_dev, ids_dev, st);
  }
  if (scores_dev) {
    const int cap = topk_cap(k);
    AMDR_MS_LAUNCH(rowscores_topk_kernel, dim3(nq), dim3(256), TopkLds<C32>::bytes(kMsWaves, cap),
                   st, full_dev, n, k, cap, scores_dev, (long long*)ids_dev);
  }
  return AMDR_OK;
}

int ms_check(const amdr_maxsim* h, const void* Q, int nq, int q_len, int k) {
  AMDR_REQUIRE(h != nullptr, "maxsim: null handle");
  AMDR_REQUIRE(nq >= 0, "maxsim: nq=%d", nq);
  AMDR_REQUIRE(q_len >= 1 && q_len <= AMDR_MAXSIM_QLEN, "maxsim: q_len=%d outside [1,%d]", q_len, AMDR_MAXSIM_QLEN);
  AMDR_REQUIRE(k >= 1 && k <= AMDR_MAX_K, "maxsim: k=%d outside [1,%d]", k, AMDR_MAX_K);
  AMDR_REQUIRE(nq == 0 || Q, "maxsim: null Q");
  return AMDR_OK;
}

}  // namespace

extern "C" {

int amdr_maxsim_create(const float* D_host, const int64_t* doc_ptr, int64_t n_docs, int32_t dim, int32_t device,
                       amdr_maxsim_t** out) {
  AMDR_REQUIRE(out != nullptr, "maxsim_create: out is null");
  *out = nullptr;
  AMDR_REQUIRE(dim == AMDR_MAXSIM_DIM, "maxsim_create: dim=%d, kernel is built for %d", dim, AMDR_MAXSIM_DIM);
  AMDR_REQUIRE(doc_ptr && n_docs >= 1 && n_docs < (1ll << 32), "maxsim_create: bad doc_ptr / n_docs");
  AMDR_REQUIRE(doc_ptr[0] == 0, "maxsim_create: doc_ptr[0] != 0");
  for (int64_t i = 0; i < n_docs; ++i)
    AMDR_REQUIRE(doc_ptr[i + 1] > doc_ptr[i], "maxsim_create: document %lld has no tokens", (long long)i);
  const int64_t nt = doc_ptr[n_docs];
  AMDR_REQUIRE(D_host != nullptr, "maxsim_create: D is null");
  int rc = check_device(device);
  if (rc) return rc;
  amdr_maxsim* h = new (std::nothrow) amdr_maxsim();
  if (!h) return fail(AMDR_ENOMEM, "maxsim_create: host alloc");
  h->device = device;
  h->n_docs = h->cap_docs = n_docs;
  h->n_tokens = h->cap_tokens = nt;
  hipError_t e = hipMalloc((void**)&h->D, (size_t)nt * dim * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(h->D, D_host, (size_t)nt * dim * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void**)&h->doc_ptr, (size_t)(n_docs + 1) * sizeof(long long));
  if (e == hipSuccess)
    e = hipMemcpy(h->doc_ptr, doc_ptr, (size_t)(n_docs + 1) * sizeof(long long), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  // once per handle (it is bound to this device): the CU count, the dynamic-LDS limits of the ring and overflow kernels
  if (e == hipSuccess) e = hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, device);
  auto lds = [&](const void* f, int b) { if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, b); };
  lds((const void*)maxsim_scores_ring_kernel<kRing>, kRing * 16384);
  lds((const void*)maxsim_hi2_ring_kernel<kRing1>, kRing1 * 16384);
  lds((const void*)maxsim_rescore_ring_kernel<kRing2>, kRing2 * 16384);
  lds((const void*)maxsim_overflow_kernel, kPairLds);
  if (e != hipSuccess) {
    amdr_maxsim_destroy(h);
    return fail(e == hipErrorOutOfMemory ? AMDR_ENOMEM : AMDR_EHIP, "maxsim_create: %s", hipGetErrorString(e));
  }
  if ((rc = ms_finish_store(*h))) {  // the statistics and the images (maxsim_store.hip), as every rebuild takes them
    amdr_maxsim_destroy(h);
    return rc;
  }
  *out = h;
  return AMDR_OK;
}

int amdr_maxsim_ndocs(const amdr_maxsim_t* h, int64_t* n) {
  AMDR_REQUIRE(h && n, "maxsim_ndocs: null");
  *n = h->n_docs;
  return AMDR_OK;
}

int amdr_maxsim_plan_info(const amdr_maxsim_t* h, int32_t nq, char* buf, int32_t buf_len) {
  AMDR_REQUIRE(h && buf && buf_len > 0, "maxsim_plan_info: null");
  AMDR_REQUIRE(nq >= 1, "maxsim_plan_info: nq=%d", nq);
  static const char* const half = "%s split-fp16 (hi + lo/2048, 3 x v_mfma_f32_32x32x16_f16 per block) + rowscores_topk_kernel";
  static const char* const f32 = "%s fp32-input (v_mfma_f32_16x16x4_f32) + rowscores_topk_kernel";
  switch (ms_route(ms_shape(h), nq, 1, true).form) {  // the ABI has no k: the route at the shallowest depth
    case MsForm::TwoPass:
      snprintf(buf, buf_len,
               "maxsim_hi2_ring_kernel split-fp16 two-pass top-k (k <= n_docs / 4): maxsim_split_queries_kernel + pass 1 hi "
               "parts only (1 x v_mfma_f32_32x32x16_f16 per block, two queries per wave) + maxsim_select_kernel + "
               "maxsim_rescore_ring_kernel<%d> (pairs grouped by document: a block = one document x %d of its queries; %d "
               "blocks per CU) (hi + lo/2048, 3 MFMAs per block, candidates only) + maxsim_final_topk_kernel (the candidates "
               "only); full score rows: maxsim_scores_ring_kernel",
               kRing2, kMsQ, kBlocks2);
      break;
    case MsForm::Ring: snprintf(buf, buf_len, half, "maxsim_scores_ring_kernel"); break;
    case MsForm::PairHalf: snprintf(buf, buf_len, half, "maxsim_scores_h_kernel"); break;
    case MsForm::Blocked: snprintf(buf, buf_len, f32, "maxsim_scores_blocked_kernel"); break;
    case MsForm::PairF32: snprintf(buf, buf_len, f32, "maxsim_scores_kernel"); break;
  }
  return AMDR_OK;
}

int amdr_maxsim_reserve(amdr_maxsim_t* h, int32_t nq_max, int32_t k_max) {
  AMDR_REQUIRE(h != nullptr, "maxsim_reserve: null handle");
  AMDR_REQUIRE(nq_max >= 1 && k_max >= 1 && k_max <= AMDR_MAX_K, "maxsim_reserve: bad sizes");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  const size_t need = ms_reserve_bytes(ms_shape(h), nq_max, k_max);
  int rc = h->full[0].ensure(need);
  if (!rc) rc = h->qbuf.ensure((size_t)nq_max * AMDR_MAXSIM_QLEN * kDim * sizeof(float));
  if (!rc) rc = h->sbuf.ensure((size_t)nq_max * k_max * sizeof(float));
  if (!rc) rc = h->ibuf.ensure((size_t)nq_max * k_max * sizeof(int64_t));
  return rc;
}

int amdr_maxsim_workspace_plan(int64_t n_docs, int32_t split_image, int32_t nq_max, int32_t k_max, int32_t nq, int32_t k,
                               int64_t* out2) {
  AMDR_REQUIRE(out2 != nullptr, "maxsim_workspace_plan: null");
  AMDR_REQUIRE(n_docs >= 1 && n_docs < (1ll << 32), "maxsim_workspace_plan: bad n_docs");
  AMDR_REQUIRE(nq_max >= 1 && k_max >= 1 && k_max <= AMDR_MAX_K && nq >= 1 && k >= 1 && k <= AMDR_MAX_K,
               "maxsim_workspace_plan: bad sizes");
  const MsShape s{n_docs, split_image != 0, split_image != 0};  // create() makes both images or neither
  out2[0] = (int64_t)ms_reserve_bytes(s, nq_max, k_max);
  out2[1] = (int64_t)ms_workspace_bytes(s, ms_route(s, nq, k, true), nq, k);
  return AMDR_OK;
}

int amdr_maxsim_search_device(amdr_maxsim_t* h, const float* Q_dev, int32_t nq, int32_t q_len, int32_t k,
                              float* scores_dev, int64_t* ids_dev, void* stream) {
  int rc = ms_check(h, Q_dev, nq, q_len, k);
  if (rc) return rc;
  AMDR_REQUIRE(nq == 0 || (scores_dev && ids_dev), "maxsim: null output");
  if (nq == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  const MsRoute r = ms_route(ms_shape(h), nq, k, true);
  if ((rc = h->full[0].ensure(ms_workspace_bytes(ms_shape(h), r, nq, k)))) return rc;
  return ms_run(h, r, Q_dev, nq, q_len, k, h->full[0], scores_dev, ids_dev, (hipStream_t)stream);
}

int amdr_maxsim_search(amdr_maxsim_t* h, const float* Q_host, int32_t nq, int32_t q_len, int32_t k,
                       float* scores_host, int64_t* ids_host) {
  int rc = ms_check(h, Q_host, nq, q_len, k);
  if (rc) return rc;
  AMDR_REQUIRE(nq == 0 || (scores_host && ids_host), "maxsim: null output");
  if (nq == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  size_t qbytes = (size_t)nq * q_len * kDim * sizeof(float);
  if ((rc = h->qbuf.ensure(qbytes))) return rc;
  const MsRoute r = ms_route(ms_shape(h), nq, k, true);
  if ((rc = h->full[1].ensure(ms_workspace_bytes(ms_shape(h), r, nq, k)))) return rc;
  if ((rc = h->sbuf.ensure((size_t)nq * k * sizeof(float)))) return rc;
  if ((rc = h->ibuf.ensure((size_t)nq * k * sizeof(int64_t)))) return rc;
  AMDR_HIP(hipMemcpyAsync(h->qbuf.p, Q_host, qbytes, hipMemcpyHostToDevice, h->stream));
  rc = ms_run(h, r, h->qbuf.as<float>(), nq, q_len, k, h->full[1], h->sbuf.as<float>(), h->ibuf.as<int64_t>(), h->stream);
  if (rc) return rc;
  AMDR_HIP(hipMemcpyAsync(scores_host, h->sbuf.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipMemcpyAsync(ids_host, h->ibuf.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipStreamSynchronize(h->stream));
  return AMDR_OK;
}

int amdr_maxsim_scores(amdr_maxsim_t* h, const float* Q_host, int32_t nq, int32_t q_len, float* scores_host) {
  int rc = ms_check(h, Q_host, nq, q_len, 1);
  if (rc) return rc;
  AMDR_REQUIRE(nq == 0 || scores_host, "maxsim_scores: null output");
  if (nq == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  size_t qbytes = (size_t)nq * q_len * kDim * sizeof(float);
  if ((rc = h->qbuf.ensure(qbytes))) return rc;
  const MsRoute r = ms_route(ms_shape(h), nq, 1, false);  // every score: one pass
  if ((rc = h->full[1].ensure(ms_workspace_bytes(ms_shape(h), r, nq, 1)))) return rc;
  AMDR_HIP(hipMemcpyAsync(h->qbuf.p, Q_host, qbytes, hipMemcpyHostToDevice, h->stream));
  rc = ms_run(h, r, h->qbuf.as<float>(), nq, q_len, 1, h->full[1], nullptr, nullptr, h->stream);
  if (rc) return rc;
  AMDR_HIP(hipMemcpyAsync(scores_host, h->full[1].p, (size_t)nq * h->n_docs * sizeof(float), hipMemcpyDeviceToHost,
                          h->stream));
  AMDR_HIP(hipStreamSynchronize(h->stream));
  return AMDR_OK;
}

int amdr_maxsim_destroy(amdr_maxsim_t* h) {
  if (!h) return AMDR_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamDestroy(h->stream);
  }
  if (h->D) (void)hipFree(h->D);
  if (h->img) (void)hipFree(h->img);
  if (h->img_hi) (void)hipFree(h->img_hi);
  if (h->doc_ptr) (void)hipFree(h->doc_ptr);
  h->full[0].release();
  h->full[1].release();
  h->qbuf.release();
  h->sbuf.release();
  h->ibuf.release();
  delete h;
  return AMDR_OK;
}

}  // extern "C"

// Dense channel, batched form: 32 queries share one pass over the chunk matrix (5-95 queries per
// call, and the 32-queries-per-pass scan of a large matrix; batches of >= 96 queries take
// dense_panel.hip).
//
// Same contract as dense.hip (exact inner-product top-k behind faiss
// `index.search`, legalrag/retrieval/dense_retriever.py:42) for query batches.
// With B queries per pass the scan is a [n x d] . [d x B] product; beyond ~8
// queries the per-(row, query) cross-lane reductions of the GEMV form saturate
// the vector ALU before HBM, so the batch is tiled 32 queries x 32 rows per wave on the
// fp32-input matrix instruction v_mfma_f32_16x16x4_f32 (four 16x16 accumulator blocks): exact
// fp32 products and accumulation (no TF32/bf16 shortcut exists or is wanted), the same peak
// rate as the vector ALU, but the accumulate needs no cross-lane traffic.  (The tile was first
// built on v_mfma_f32_32x32x2_f32 — same flops per cycle on paper; the 16x16 form measured
// 7.5 % faster on the UCC-en launch in a same-box A/B: the chip holds a higher clock on it.)
//   A (16 x 4): lane (i16 = l&15, kq = l>>4) <- streamed row 16b + i16    (HBM -> registers -> LDS -> registers)
//   B (4 x 16): lane (i16, kq)              <- LDS tile (query) row 16b + i16   (staged once per block)
// The streamed operand is fetched with fully coalesced 16-B/lane loads (8 rows x 128 B per wave
// instruction, each byte read from HBM exactly once), parked in a wave-private, XOR-swizzled
// 4-KiB LDS stage and read back as fragments; four 32-float chunks per wave (128 KiB per CU
// with 8 waves) are always in flight in registers.  The k order inside a chunk is permuted
// (lane group kq takes 16-B slots kq and 4 + kq); both operands use the same permutation,
// which a dot product cannot see.  The finished 32x32 tile leaves as 16-byte stores
// S[query][4 consecutive rows] straight from the accumulators (epilogue).  Top-k is a
// second, slab-parallel pass over S (+8 % traffic at d = 768: 128 B written and read per
// 3072-B row per 32 queries).
#include "common.hpp"
#include "tile_swizzle.hpp"
#include "topk.hpp"

#include <cfloat>
#include <cstdlib>

namespace amdr {

constexpr int kBW = 4;          // waves per block
constexpr int kKC = 32;         // floats of every row per staged chunk (128 B = 8 slots of 16 B)
constexpr int kStageBytes = 32 * kKC * 4;  // 4 KiB: one 32-row x 32-float chunk
#ifndef AMDR_STAGE_BUFS
#define AMDR_STAGE_BUFS 1
#endif
// LDS stages per wave.  One is enough: the LDS unit serves a wave's operations in order, so the
// ds_writes of chunk c+2 cannot overtake the fragment reads of chunk c+1 issued before them, and
// those reads land in registers (FX/FQ) a whole chunk of MFMAs before they are used.
constexpr int kStageBufs = AMDR_STAGE_BUFS;
constexpr int kPieces = kStageBytes / 1024;  // 1-KiB wave loads per chunk (4): 8 rows x 128 B each
constexpr int kDepth = 4;                      // chunks in flight from HBM per wave (16 KiB)

// LDS image of a staged chunk: 32 rows of 128 B in the byte order of stage_off (tile_swizzle.hpp).

// The three pipeline steps are macros, not functions: passing the register arrays by
// reference made hipcc (ROCm 7.2) keep them in scratch memory.
#define AMDR_STAGE_CHUNK(ST, G)                                                                   \
  _Pragma("unroll") for (int p_ = 0; p_ < kPieces; ++p_)                                          \
      *reinterpret_cast<f32x4*>((ST) + stage_off(8 * p_ + lrow, lslot)) = G[p_];
// Fragments of one 32-float chunk.  v_mfma_f32_16x16x4_f32 takes A[row l&15][k = l>>4] and
// B[k = l>>4][col l&15], one float per lane, so a lane (i16 = l & 15, kq = l >> 4) owns, for each
// of the two 16-row blocks b of the tile, the 16-B slots 4u + kq (u = 0, 1) of row 16b + i16: the
// chunk's eight k-steps take component (u, x..w) of those slots from the four kq groups — a
// permutation of k that both operands share.  Slot choice 4u + kq keeps both images
// conflict-free: a ds_read_b128 lane group {0-3, 12-15, 20-27} (and its three siblings) holds 16
// distinct rows, eight at slot 4u + kq and eight at 4u + (kq ^ 1), and the row swizzles map
// exactly those two sets onto disjoint bank quads.
#define AMDR_READ_FRAGS(ST, C, FX, FQ)                                                            \
  _Pragma("unroll") for (int b_ = 0; b_ < 2; ++b_) {                                              \
    _Pragma("unroll") for (int u_ = 0; u_ < 2; ++u_) {                                            \
      FX[b_][u_] = *reinterpret_cast<const f32x4*>((ST) + b_ * 2048 + xoff[u_]);                    \
      FQ[b_][u_] = qrow[b_ * 16 * (d / 4) + ((C) >> 1) * 16 + qlow[(C) & 1][u_]];                 \
    }                                                                                             \
  }
#if defined(AMDR_ABLATE) && AMDR_ABLATE == 1  // timing-only build: matrix pipe removed, operands kept live
#define AMDR_MFMA_STEP(A_, B_, BI, BJ) acc[BI][BJ].x += (A_) * (B_);
#else
#define AMDR_MFMA_STEP(A_, B_, BI, BJ) acc[BI][BJ] = __builtin_amdgcn_mfma_f32_16x16x4f32(A_, B_, acc[BI][BJ], 0, 0, 0);
#endif
// 8 k-steps x 4 accumulator blocks = 32 MFMAs of 32 cycles per chunk; an accumulator is touched
// every fourth instruction, well past the 40-cycle dependent latency.
// A operand = streamed chunk rows, B operand = queries: a 16x16 result block then has the QUERY on the lane and four
// consecutive chunk rows in the lane's registers (acc[bi][bj][r] = <row 16 bj + 4 kq + r, query 16 bi + i16>), so
// S[query][row .. row+3] is one 16-byte store (see the epilogue).
#define AMDR_MFMA_KSTEP(FX, FQ, U, COMP)                                                          \
  AMDR_MFMA_STEP(FX[0][U].COMP, FQ[0][U].COMP, 0, 0)                                              \
  AMDR_MFMA_STEP(FX[1][U].COMP, FQ[0][U].COMP, 0, 1)                                              \
  AMDR_MFMA_STEP(FX[0][U].COMP, FQ[1][U].COMP, 1, 0)                                              \
  AMDR_MFMA_STEP(FX[1][U].COMP, FQ[1][U].COMP, 1, 1)
#define AMDR_MFMA_CHUNK(FX, FQ)                                                                   \
  AMDR_MFMA_KSTEP(FX, FQ, 0, x) AMDR_MFMA_KSTEP(FX, FQ, 0, y) AMDR_MFMA_KSTEP(FX, FQ, 0, z)       \
  AMDR_MFMA_KSTEP(FX, FQ, 0, w) AMDR_MFMA_KSTEP(FX, FQ, 1, x) AMDR_MFMA_KSTEP(FX, FQ, 1, y)       \
  AMDR_MFMA_KSTEP(FX, FQ, 1, z) AMDR_MFMA_KSTEP(FX, FQ, 1, w)
// (Pinning an MFMA / ds_write / global_load / ds_read interleave with sched_group_barrier was
// measured 2-7 % SLOWER than hipcc's own schedule of this region and is not kept.)
#define AMDR_INTERLEAVE()

#if defined(AMDR_ABLATE) && AMDR_ABLATE == 2  // timing-only build: no X traffic (registers filled from an address hash)
#define AMDR_LDX(PTR) ([&] { f32x4 z_; z_.x = z_.y = z_.z = z_.w = (float)(((size_t)(PTR)) & 1023) * 1e-3f; return z_; }())
#else
// NTL (template constant): non-temporal policy for a matrix beyond the Infinity Cache (common.hpp)
#define AMDR_LDX(PTR) (NTL ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(PTR)) : *reinterpret_cast<const f32x4*>(PTR))
#endif

// grid: (x = row slabs, y = 32-query tiles).
// LDS: Q tile row-major [32][d/4] float4, slots XOR-swizzled per row (d*128 B) + per wave one private 4-KiB chunk stage.
// (Round 1 also ran this kernel with the roles swapped — chunk tiles in LDS, queries streamed — for
// short corpora under long batches; dense_panel.hip replaced that orientation and it was removed.)
template <int D8, int WAVES, bool NTL>  // NTL: non-temporal loads of the streamed operand; D8 = d / 8; WAVES = 8 when the Q tile leaves room for 8 stages (d <= 768)
__global__ __launch_bounds__(WAVES * 64) void dense_mfma_scores_kernel(const float* __restrict__ X, long n,
                                                                 const float* __restrict__ Q, int nq,
                                                                 long rows_per_block, int gx, int gy, long ldS,
                                                                 float* __restrict__ S /*[queries][ldS]*/, int tile_max,
                                                                 const int* __restrict__ gate) {
  if (gate != nullptr && *gate == 0) return;  // a gated launch (dense.hip hi2_pass): decided on the device, block-uniform
  // tile_max == 0: S[query][row] for every row.
  // tile_max != 0: S[query][tile] = MAXIMUM of the query's scores over the 32-row tile (first pass of the two-level
  //                top-k of a large scan: dense.hip exact_tail).
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int d = D8 * 8;
  constexpr int NCH = d / kKC;  // chunks per row: 12 / 24 / 32 (always even: d % 64 == 0)
  static_assert(d % kKC == 0, "dim must be a multiple of 64");
  const f32x4* qsv = reinterpret_cast<const f32x4*>(smem);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned char* stage = smem + (size_t)d * 128 + (size_t)wave * kStageBufs * kStageBytes;
  const int i16 = lane & 15, kq = lane >> 4;  // MFMA fragment roles
  // Lane-dependent parts of the fragment addresses, computed once: every other term is a
  // compile-time constant of the unrolled chunk loop and folds into the ds_read offset field.
  //   stage: row 16 b + i16, slot 4 u + kq -> b * 2048 + i16 * 128 + ((4u + kq) ^ (i16 >> 1)) * 16
  //   LDS tile: row 16 b + i16, slot 8 C + 4 u + kq, XOR i16 touches the low four bits only
  int xoff[2], qlow[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    xoff[u] = stage_off(i16, 4 * u + kq);
    qlow[0][u] = (4 * u + kq) ^ i16;
    qlow[1][u] = (8 + 4 * u + kq) ^ i16;
  }
  const f32x4* qrow = qsv + i16 * (d / 4);
  // Block id -> (slab bx of the streamed operand, tile by of the LDS operand).  The grid is 1-D and
  // remapped so that each XCD (blocks with equal id % 8 share one; 8 XCDs, each with its own L2)
  // owns a CONTIGUOUS range of the slab-major order: the `gy` blocks that stream the same slab
  // then sit on one XCD and the slab crosses the fabric once, not once per XCD.  (UCC-en step,
  // PMC: L2-miss reads of this launch 268 MB -> see profiles/; the bijective form of the remap
  // handles grids that are not a multiple of 8.)
  int bx, by;
  {
    const int nwg = gx * gy, bid = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    // with a single LDS tile (gy == 1) nothing is shared between blocks: plain order (a 10 M-row
    // scan measured 1 % slower remapped, the UCC-en launch 1.3 % faster and 3.7x less fabric traffic)
    const int logical = gy == 1 ? bid : (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    bx = logical / gy;
    by = logical - bx * gy;
  }
  const int q0 = by * 32;

  // ---- stage the query tile, row-major with a per-row XOR swizzle of the 16-byte slots:
  //   qs[i * d/4 + (k4 ^ (i & 15))] = Q[q0+i][4*k4 .. 4*k4+3]
  // Global reads are fully coalesced (a wave reads 1 KiB of one query row per instruction);
  // both the staging writes (8 consecutive slots of one row per ds_write_b128 lane group) and
  // the fragment reads (same logical slot of 16 different rows per ds_read_b128 lane group;
  // row stride d*4 is a multiple of the 256-B bank row) are conflict-free.
  // Loads are issued in batches of 16 per thread BEFORE any of them is consumed: one load per
  // loop trip serialises 24+ L2 round trips (measured: ~14 us of a 25-us block at UCC-en size).
  {
    constexpr int NT = WAVES * 64, TOTAL = 32 * (d / 4), PER = (TOTAL + NT - 1) / NT, BATCH = 16;
#pragma unroll
    for (int j0 = 0; j0 < PER; j0 += BATCH) {
      f32x4 tmp[BATCH];
#pragma unroll
      for (int j = 0; j < BATCH; ++j) {
        if (j0 + j < PER) {
          const int idx = threadIdx.x + (j0 + j) * NT;
          const int qi_ = idx / (d / 4), k4 = idx - qi_ * (d / 4);
          f32x4 z = {0.f, 0.f, 0.f, 0.f};
          tmp[j] = (idx < TOTAL && q0 + qi_ < nq) ? *reinterpret_cast<const f32x4*>(Q + (size_t)(q0 + qi_) * d + 4 * k4)
                                                  : z;
        }
      }
#pragma unroll
      for (int j = 0; j < BATCH; ++j) {
        if (j0 + j < PER) {
          const int idx = threadIdx.x + (j0 + j) * NT;
          const int qi_ = idx / (d / 4), k4 = idx - qi_ * (d / 4);
          if (idx < TOTAL) reinterpret_cast<f32x4*>(smem)[qi_ * (d / 4) + (k4 ^ (qi_ & 15))] = tmp[j];
        }
      }
    }
  }
  __syncthreads();

  const long row_lo = (long)bx * rows_per_block;
  long row_hi = row_lo + rows_per_block;
  if (row_hi > n) row_hi = n;
  // loader role of this lane inside a 1-KiB piece: 8 rows x 8 slots
  const int lrow = lane >> 3, lslot = lane & 7;

  for (long r0 = row_lo + (long)wave * 32; r0 < row_hi; r0 += (long)WAVES * 32) {
    // global pointers of the 8 pieces (rows 4p + lrow), clamped at the slab end
    const float* gp[kPieces];
#pragma unroll
    for (int p = 0; p < kPieces; ++p) {
      long r = r0 + 8 * p + lrow;
      if (r >= row_hi) r = row_hi - 1;
      gp[p] = X + (size_t)r * d + lslot * 4;
    }
    // Software pipeline; every index below is a compile-time constant once the chunk loop is
    // unrolled, so the arrays live in registers:
    //   G[c % kDepth]  chunk c as it arrives from HBM (kDepth chunks = 16 KiB per wave in flight)
    //   stage[c & 1]   this wave's LDS image of chunk c (swizzled, double-buffered)
    //   FX/FQ[c & 1]   MFMA fragments of chunk c, read from LDS one chunk AHEAD of their use so
    //                  the dependent MFMA chain never waits on an LDS round trip.
    f32x4 G[kDepth][kPieces], FX[2][2][2], FQ[2][2][2];
#pragma unroll
    for (int j = 0; j < kDepth; ++j) {
      if (j < NCH) {
#pragma unroll
        for (int p = 0; p < kPieces; ++p) G[j][p] = AMDR_LDX(gp[p] + j * kKC);
      }
    }
    AMDR_STAGE_CHUNK(stage, G[0])
    if (kDepth < NCH) {
#pragma unroll
      for (int p = 0; p < kPieces; ++p) G[0][p] = AMDR_LDX(gp[p] + kDepth * kKC);
    }
    wave_lds_fence();
    AMDR_READ_FRAGS(stage, 0, FX[0], FQ[0])
    f32x4 acc[2][2];  // acc[bi][bj][r] = <streamed row 16 bj + 4 kq + r, query (LDS-tile row) 16 bi + i16>
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      // One scheduling region per chunk: the 32 MFMAs of chunk c and, in their shadow,
      // the staging of chunk c+1 (4 ds_write), the refill of its registers with chunk
      // c+1+kDepth (4 loads) and its fragment reads (8 ds_read).  The LDS unit serves a wave's
      // operations in order and the compiler keeps the may-alias write->read order on `stage`.
      if (c + 1 < NCH) {
        unsigned char* st_n = stage + ((c + 1) % kStageBufs) * kStageBytes;
        AMDR_STAGE_CHUNK(st_n, G[(c + 1) % kDepth])
        if (c + 1 + kDepth < NCH) {
#pragma unroll
          for (int p = 0; p < kPieces; ++p) G[(c + 1) % kDepth][p] = AMDR_LDX(gp[p] + (c + 1 + kDepth) * kKC);
        }
        AMDR_READ_FRAGS(st_n, c + 1, FX[(c + 1) & 1], FQ[(c + 1) & 1])
      }
      AMDR_MFMA_CHUNK(FX[c & 1], FQ[c & 1])
      AMDR_INTERLEAVE()
      wave_lds_fence();
    }
    // Epilogue: four 16-byte stores per lane, S[query 16 bi + i16][rows 16 bj + 4 kq .. + 3] — a store instruction
    // covers 64 contiguous bytes of each of 16 query rows.  (Round 1 had the operands the other way round — query
    // on the registers — and turned the 32x32 tile through the wave's LDS stage to store whole 128-byte rows:
    // 16 ds_write + 16 ds_read + 16 four-byte stores per tile; with the matrix pipe taken out that kernel ran no
    // faster on the 10 M-row scan, i.e. the non-MFMA stream bound it, and 8 / 16 / 32 queries per scan cost
    // 4.9 / 5.4 / 5.8 ms.  With these stores: 4.9 / 5.1 / 5.8-5.9 ms, the UCC-en launch of this kernel 351 -> 344 us.
    // Timing-only builds on the 10 M-row, 32-query scan: without the score stores 5.80 -> 5.10 ms (1.28 GB of writes
    // = 4 % of the bytes cost 12 % of the time: they interleave with the read stream at the HBM), non-temporal
    // stores 6.01 -> 6.10 ms.)  Rows past n inside the last 32-row tile repeat row n - 1 and land in the
    // padding of S (ldS is a multiple of 32); slab boundaries are multiples of 32 rows.
    if (tile_max) {
      // tile maxima: 7 v_max per query block in the lane, two exchanges over the four kq groups (rows past the end
      // of the matrix repeat its last row: no effect on a maximum)
#pragma unroll
      for (int bi = 0; bi < 2; ++bi) {
        float m = fmaxf(fmaxf(fmaxf(acc[bi][0][0], acc[bi][0][1]), fmaxf(acc[bi][0][2], acc[bi][0][3])),
                        fmaxf(fmaxf(acc[bi][1][0], acc[bi][1][1]), fmaxf(acc[bi][1][2], acc[bi][1][3])));
        m = fmaxf(m, __uint_as_float(lane_xor<16>(__float_as_uint(m))));
        m = fmaxf(m, __uint_as_float(lane_xor<32>(__float_as_uint(m))));
        const int q = q0 + 16 * bi + i16;
        if (kq == 0 && q < nq) S[(size_t)q * ldS + (r0 >> 5)] = m;
      }
      continue;
    }
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
      const int q = q0 + 16 * bi + i16;
      if (q < nq) {
        float* srow = S + (size_t)q * ldS + r0 + 4 * kq;
#if defined(AMDR_ABLATE) && AMDR_ABLATE == 3  // timing-only build: no score stores
        if (acc[bi][0][0] == 12345.f) srow[0] = acc[bi][1][1];
#else
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) *reinterpret_cast<f32x4*>(srow + 16 * bj) = acc[bi][bj];
#endif
      }
    }
  }
}


// grid: (x = row slabs, y = queries): top-k of S[q][slab] -> part[slab][q][k], or, when there
// is a single slab, straight to the final (scores, ids).  WAVES = 1 for short rows.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void scores_slab_topk_kernel(const float* __restrict__ S, long ldS, long n, int nq, int k,
                                                                       int cap, long rows_per_slab,
                                                                       C32* __restrict__ part,
                                                                       float* __restrict__ fin_scores,
                                                                       long long* __restrict__ fin_ids) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const TopkLds<C32> L(smem, WAVES, cap);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qi = blockIdx.y;
  const long lo = (long)blockIdx.x * rows_per_slab;
  long hi = lo + rows_per_slab;
  if (hi > n) hi = n;
  const float* row = S + (size_t)qi * ldS;
  WaveTopK<C32> tk;
  tk.init(L.list(wave), cap, k);
  bool done = false;
  if (WAVES == 1 && k <= 64 && hi - lo <= kSelectRowsMax) {
    // short row: register selector (topk.hpp); scratch = the upper half of the staging buffer
    const int got = select_row_any(row, lo, hi, k, lane, tk.buf);
    if (got >= 0) {
      tk.cnt = got;
      done = true;
    }
  }
  // S is read exactly once: non-temporal (slabs start on multiples of 64 rows and S rows on 128-byte lines)
  if (!done) wave_topk_sweep4<true>(tk, row, lo, hi, wave, WAVES, lane);
  if (WAVES > 1) block_combine_topk(tk, L, WAVES, wave, lane);
  if (wave == 0) topk_emit(tk.buf, tk.cnt, k, lane, fin_scores, fin_ids, (size_t)qi, part, (size_t)blockIdx.x * nq + qi);
}

__global__ __launch_bounds__(64) void scores_pair_topk_kernel(const float* __restrict__ S, long ldS, long n, int nq,
                                                              int k, int cap, float* __restrict__ fin_scores,
                                                              long long* __restrict__ fin_ids) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  C32* buf = reinterpret_cast<C32*>(smem);  // cap entries (>= 128): staged-selector list; the pair selector uses 64
  const int lane = threadIdx.x;
  const int q = 2 * blockIdx.x + (lane >> 5);
  const bool has_q = q < nq;
  C32 out = C32::pad();
  int got = select_row_pair_any(S, ldS, n, q, has_q, k, lane, buf, out);
  if (got < 0) pair_rows_staged(S, ldS, n, 2 * blockIdx.x, nq, k, cap, buf, lane, true, out, got);  // mass ties at the cut
  const int j = lane & 31;
  if (has_q && j < k) topk_store(out, j < got, j, fin_scores + (size_t)q * k, fin_ids + (size_t)q * k);
}

// ---------------------------------------------------------------------------------------------------------------------
// The exact tail of a large scan behind the tile maxima M[q][tile] (tile_max above): each query's k best tiles, the exact
// scores of their rows, the final top-k.  The exact two-level form runs it for every query of a pass; the fp16 first
// pass (dense_hi.hip) behind its device flag, for the queries its rounding bound did not resolve (dense.hip exact_tail).

// Step 2: the k tiles with the largest maxima, ascending by tile id, into the query's list; lower tile ids win among
// equal maxima.  `gate` (nullable): nothing runs unless *gate != 0.  `unres` (nullable): only queries with unres[q] != 0.
// One block sweeps its query's whole row of M: right for the few unresolved queries behind the fp16 pass.  For every
// query of a pass on a 10 M-row matrix (312 500 maxima per query, a handful of blocks) the sweep is bound by the
// latency of its own loads, so the ungated call picks the tiles with the slab top-k (+ merge) that spreads a row over
// many blocks and passes them in `chosen` ([queries][k] tile ids, best first, -1 behind the last; one wave per
// query): only the ordering is left to do here.
__global__ __launch_bounds__(256) void dense_hi_exact_select_kernel(const float* __restrict__ M, long ldM, long n_tiles, int k,
                                                                    int tcap, int list_stride, int* __restrict__ list,
                                                                    int* __restrict__ count, const int* __restrict__ unres,
                                                                    const int* __restrict__ gate,
                                                                    const long long* __restrict__ chosen) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (gate != nullptr && *gate == 0) return;
  const int q = blockIdx.x;
  if (unres != nullptr && unres[q] == 0) return;
  const TopkLds<C32> L(smem, 4, tcap);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  WaveTopK<C32> tk;
  tk.init(L.list(wave), tcap, k);
  if (chosen != nullptr) {
    int got = 0;
    for (int j0 = 0; j0 < k; j0 += 64) {
      const int j = j0 + lane;
      const long long t = j < k ? chosen[(size_t)q * k + j] : -1ll;
      if (t >= 0) tk.buf[j] = C32::make(0.f, (u32)t);
      got += __popcll(__ballot(t >= 0));
    }
    tk.cnt = got;
    wave_lds_fence();
  } else {
    wave_topk_sweep4<false>(tk, M + (size_t)q * ldM, 0, n_tiles, wave, 4, lane);  // ldM is a multiple of 32 floats: whole float4s
    block_combine_topk(tk, L, 4, wave, lane);
    if (wave != 0) return;
  }
  const int keep = tk.cnt;
  for (int j = lane; j < keep; j += 64) {
    const long long t = tk.buf[j].id();
    int rank = 0;
    for (int i = 0; i < keep; ++i) rank += tk.buf[i].id() < t ? 1 : 0;
    list[(size_t)q * list_stride + rank] = (int)t;
  }
  if (lane == 0) count[q] = keep;
}

// Step 3: exact scores of every query's OWN candidate tiles, lean form.  A retired mode 3 of
// the tile kernel above did this with a whole 32-query LDS tile per block (96 KiB staged, 31 of 32 MFMA columns idle, one block
// per CU: 38 us per 64 queries).  Here a wave scores ONE (query, tile): the tile's rows stream through the wave's 4-KiB
// stage exactly as above (same loads, same fragments), the B operand is the query's own components broadcast to all 16
// columns, and only the two row blocks are multiplied: 16 MFMAs per chunk instead of 32, the k-steps in the SAME order —
// acc[bj] sees the sequence the tile kernel's acc[bi][bj] sees, hence the same bits (tested against the full score matrix).
// 20 KiB of LDS per 4-wave block: the candidate tiles of a batch spread over every CU.
// grid: (queries, ceil(max tiles per query / WPB)).
template <int D8, int WPB>
__global__ __launch_bounds__(WPB * 64) void dense_rescore_tiles_kernel(const float* __restrict__ X, long n_real,
                                                                       const float* __restrict__ Q,
                                                                       const int* __restrict__ list,
                                                                       const int* __restrict__ count, int list_stride,
                                                                       long ldS, float* __restrict__ S) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int d = D8 * 8;
  constexpr int NCH = d / kKC;
  // 8 chunks (32 KiB) in flight per wave: a wave walks ONE tile, 24-32 dependent chunk steps, and with 4 in flight the kernel
  // was bound by the latency of its own loads (64 queries: 27 us for 86 MB)
  constexpr int kRsDepth = 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // grid (queries, tile groups): the blocks that hold the HEADS of the lists — the live ones — are dispatched first and
  // land one per CU; with the tile group as the fast index the 4 live blocks of a query sat next to 5 dead ones and the
  // live blocks clumped on the CUs the dead ones had just freed (27 us for 86 MB)
  const int q = blockIdx.x;
  const int cnt = count[q];
  if ((int)blockIdx.y * WPB >= cnt) return;  // block-uniform: nothing of this query's list falls to the block
  f32x4* qv = reinterpret_cast<f32x4*>(smem);
  for (int i = threadIdx.x; i < d / 4; i += WPB * 64) qv[i] = *reinterpret_cast<const f32x4*>(Q + (size_t)q * d + 4 * i);
  __syncthreads();
  const int t = blockIdx.y * WPB + wave;
  if (t >= cnt) return;
  unsigned char* stage = smem + (size_t)d * 4 + (size_t)wave * kStageBytes;
  const int i16 = lane & 15, kq = lane >> 4;
  const int lrow = lane >> 3, lslot = lane & 7;
  int xoff[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) xoff[u] = stage_off(i16, 4 * u + kq);
  const long src0 = (long)list[(size_t)q * list_stride + t] * 32;
  const float* gp[kPieces];
#pragma unroll
  for (int p = 0; p < kPieces; ++p) {
    long r = src0 + 8 * p + lrow;
    if (r >= n_real) r = n_real - 1;
    gp[p] = X + (size_t)r * d + lslot * 4;
  }
  f32x4 G[kRsDepth][kPieces], FX[2][2][2], FQ[2][2];
#pragma unroll
  for (int j = 0; j < kRsDepth; ++j) {
    if (j < NCH) {
#pragma unroll
      for (int p = 0; p < kPieces; ++p) G[j][p] = *reinterpret_cast<const f32x4*>(gp[p] + j * kKC);
    }
  }
#define AMDR_RS_FRAGS(ST, C, FX_, FQ_)                                                     \
  _Pragma("unroll") for (int u_ = 0; u_ < 2; ++u_) {                                       \
    FX_[0][u_] = *reinterpret_cast<const f32x4*>((ST) + xoff[u_]);                           \
    FX_[1][u_] = *reinterpret_cast<const f32x4*>((ST) + 2048 + xoff[u_]);                    \
    FQ_[u_] = qv[8 * (C) + 4 * u_ + kq];                                                   \
  }
#define AMDR_RS_KSTEP(FX_, FQ_, U, COMP)                                                              \
  acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(FX_[0][U].COMP, FQ_[U].COMP, acc[0], 0, 0, 0);        \
  acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(FX_[1][U].COMP, FQ_[U].COMP, acc[1], 0, 0, 0);
  AMDR_STAGE_CHUNK(stage, G[0])
  if (kRsDepth < NCH) {
#pragma unroll
    for (int p = 0; p < kPieces; ++p) G[0][p] = *reinterpret_cast<const f32x4*>(gp[p] + kRsDepth * kKC);
  }
  wave_lds_fence();
  AMDR_RS_FRAGS(stage, 0, FX[0], FQ[0])
  f32x4 acc[2];  // acc[bj][r] = <row 16 bj + 4 kq + r of the tile, the query>, the same in every column i16
  acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
  acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (c + 1 < NCH) {
      AMDR_STAGE_CHUNK(stage, G[(c + 1) % kRsDepth])
      if (c + 1 + kRsDepth < NCH) {
#pragma unroll
        for (int p = 0; p < kPieces; ++p) G[(c + 1) % kRsDepth][p] = *reinterpret_cast<const f32x4*>(gp[p] + (c + 1 + kRsDepth) * kKC);
      }
      AMDR_RS_FRAGS(stage, c + 1, FX[(c + 1) & 1], FQ[(c + 1) & 1])
    }
    AMDR_RS_KSTEP(FX[c & 1], FQ[c & 1], 0, x) AMDR_RS_KSTEP(FX[c & 1], FQ[c & 1], 0, y)
    AMDR_RS_KSTEP(FX[c & 1], FQ[c & 1], 0, z) AMDR_RS_KSTEP(FX[c & 1], FQ[c & 1], 0, w)
    AMDR_RS_KSTEP(FX[c & 1], FQ[c & 1], 1, x) AMDR_RS_KSTEP(FX[c & 1], FQ[c & 1], 1, y)
    AMDR_RS_KSTEP(FX[c & 1], FQ[c & 1], 1, z) AMDR_RS_KSTEP(FX[c & 1], FQ[c & 1], 1, w)
    wave_lds_fence();
  }
#undef AMDR_RS_FRAGS
#undef AMDR_RS_KSTEP
  if (i16 == 0) {
    float* srow = S + (size_t)q * ldS + (size_t)t * 32 + 4 * kq;
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      f32x4 v = acc[bj];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (src0 + 16 * bj + 4 * kq + r >= n_real) v[r] = -FLT_MAX;  // rows past the end inside the last tile
      *reinterpret_cast<f32x4*>(srow + 16 * bj) = v;
    }
  }
}

// The final top-k of every query over the re-scored columns of ITS tiles (32 per list entry, count[q] entries), with the
// column -> row id map in the epilogue (columns ascend with the rows: ties already went to the lower id).  A column
// past the end of the matrix (score -FLT_MAX) can only surface when fewer than k rows are real: id -1.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void dense_final_topk_kernel(const float* __restrict__ S, long ldS,
                                                                      const int* __restrict__ list,
                                                                      const int* __restrict__ count, int list_stride,
                                                                      long n_real, int k, int cap,
                                                                      float* __restrict__ fin_scores,
                                                                      long long* __restrict__ fin_ids) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const TopkLds<C32> L(smem, WAVES, cap);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qi = blockIdx.x;
  const long hi = (long)count[qi] * 32;
  const float* row = S + (size_t)qi * ldS;
  WaveTopK<C32> tk;
  tk.init(L.list(wave), cap, k);
  bool done = false;
  if (WAVES == 1 && k <= 64 && hi <= kSelectRowsMax) {
    int got;
    if (hi <= 512)
      got = select_row<8>(row, 0, hi, k, lane, tk.buf);
    else if (hi <= 1024)
      got = select_row<16>(row, 0, hi, k, lane, tk.buf);
    else
      got = select_row<32>(row, 0, hi, k, lane, tk.buf);
    if (got >= 0) {
      tk.cnt = got;
      done = true;
    }
  }
  if (!done) wave_topk_sweep4<false>(tk, row, 0, hi, wave, WAVES, lane);
  if (WAVES > 1) block_combine_topk(tk, L, WAVES, wave, lane);
  if (wave == 0) {
    for (int j = lane; j < k; j += 64) {
      // A NaN score (key 1: it sorts behind every real score) is no hit: a query or rows that score NaN come back as
      // padding (id -1, -FLT_MAX), whichever other queries share the pass (tests/test_kernels_gpu.py, test_dense_hi_gpu.py).
      const bool v = j < tk.cnt && (u32)(tk.buf[j].c >> 32) != 1u;
      const C32 c = v ? tk.buf[j] : C32::pad();
      long long id = -1ll;
      if (v) {
        const long long col = c.id();
        const long long r = (long long)list[(size_t)qi * list_stride + (col >> 5)] * 32 + (col & 31);
        id = r < n_real ? r : -1ll;
      }
      fin_scores[(size_t)qi * k + j] = v ? c.score() : -FLT_MAX;
      fin_ids[(size_t)qi * k + j] = id;
    }
  }
}

bool dense_mfma_supported(int d) { return d >= 64 && d <= 1024 && d % 64 == 0; }

// Plan shared by reserve and launch.
// waves per block: each needs kStageBufs x 4 KiB of stage beside the d*128-byte LDS tile in 160 KiB of LDS
static constexpr int scores_waves(int d) {
  int w = (int)((160 * 1024 - (long)d * 128) / (kStageBufs * kStageBytes));
  return w > 8 ? 8 : w;  // two waves per SIMD wherever the LDS tile leaves room (every d <= 1024 with one stage)
}

// `tiles` 32-row tiles of the chunk matrix are cut into gx slabs per query tile held in LDS
// (`q_tiles` of them).  One block per CU is resident (the LDS tile fills most of the LDS), a block
// costs (tiles per wave) tile-times plus ~1/4 tile-time to stage its LDS tile, and blocks run in
// rounds of 256.  Returns the slab count with the smallest estimate.
static long plan_slabs(long tiles, long q_tiles, int waves) {
  long gx_max = (tiles + waves - 1) / waves;  // at least one tile per wave
  if (gx_max < 1) gx_max = 1;
  long gx = 1;
  double best = 1e300;
  for (long g = 1; g <= gx_max && g <= 4096; ++g) {
    long tpb = (tiles + g - 1) / g;
    long per_wave = (tpb + waves - 1) / waves;
    long rounds = (q_tiles * g + 255) / 256;
    double est = (double)rounds * ((double)per_wave + 0.25);
    if (est < best - 1e-9) {
      best = est;
      gx = g;
    }
  }
  return gx;
}

void dense_mfma_plan(long n, int d, int nq, int k, DenseMfmaPlan* p, bool grid) {
  const int kBW = scores_waves(d);
  p->q_tiles = ceil_div(nq, 32);
  const long tiles = (n + 31) / 32;
  const long gx = grid ? plan_slabs(tiles, p->q_tiles, kBW) : 1;
  long tiles_per_block = (tiles + gx - 1) / gx;
  tiles_per_block = ((tiles_per_block + kBW - 1) / kBW) * kBW;
  p->rows_per_block = tiles_per_block * 32;
  p->grid_x = (int)((n + p->rows_per_block - 1) / p->rows_per_block);
  p->grid_y = p->q_tiles;
  if (p->grid_x < 1) p->grid_x = 1;
  p->lds_scores = (size_t)d * 32 * sizeof(float) + (size_t)kBW * kStageBufs * kStageBytes;
  p->waves = kBW;
  // top-k pass: slabs of >= 16 Ki rows, enough blocks to fill the chip
  long sl = (256L * 8 + nq - 1) / nq;
  long sl_max = (n + 16383) / 16384;
  if (sl > sl_max) sl = sl_max;
  if (sl < 1) sl = 1;
  p->rows_per_slab = ((n + sl - 1) / sl + 63) / 64 * 64;
  p->slabs = (int)((n + p->rows_per_slab - 1) / p->rows_per_slab);
  if (p->slabs < 1) p->slabs = 1;
  p->cap = topk_cap(k);
  // rows of S start on 128-byte lines: the 32-column store segments are then whole lines
  p->ld = (n + 31) / 32 * 32;
  p->s_bytes = (size_t)nq * (size_t)p->ld * sizeof(float);
  p->part_bytes = (size_t)p->slabs * nq * k * sizeof(C32);
}

template <int D8, int WAVES, bool NTL>
static int launch_scores(const DenseMfmaPlan& p, const float* X, long n, const float* Q, int nq, float* S,
                         hipStream_t st, bool tile_max, const int* gate) {
  // 128-160 KiB of dynamic LDS needs the opt-in.  The attribute belongs to the (function, device)
  // pair, the C ABI takes a device ordinal, and setting it is cheap: set on every launch for the
  // current device rather than remembering "done" per process.
  AMDR_HIP(hipFuncSetAttribute((const void*)dense_mfma_scores_kernel<D8, WAVES, NTL>,
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               D8 * 8 * 32 * (int)sizeof(float) + WAVES * kStageBufs * kStageBytes));
  hipLaunchKernelGGL((dense_mfma_scores_kernel<D8, WAVES, NTL>), dim3(p.grid_x * p.grid_y), dim3(WAVES * 64),
                     p.lds_scores, st, X, n, Q, nq, p.rows_per_block, p.grid_x, p.grid_y, p.ld, S, (int)tile_max, gate);
  return AMDR_OK;
}

int dense_mfma_launch_scores(const DenseMfmaPlan& p, const float* X, long n, int d, const float* Q, int nq, float* S,
                             hipStream_t st, bool tile_max, const int* gate) {
  int rc = AMDR_OK;
  const bool nt = dense_stream_nontemporal(n, d);
  switch (d) {
#define AMDR_CASE(D)                                                          \
  case D:                                                                     \
    rc = nt ? launch_scores<D / 8, scores_waves(D), true>(p, X, n, Q, nq, S, st, tile_max, gate)   \
            : launch_scores<D / 8, scores_waves(D), false>(p, X, n, Q, nq, S, st, tile_max, gate); \
    break;
    AMDR_CASE(64) AMDR_CASE(128) AMDR_CASE(192) AMDR_CASE(256) AMDR_CASE(320) AMDR_CASE(384)
    AMDR_CASE(448) AMDR_CASE(512) AMDR_CASE(576) AMDR_CASE(640) AMDR_CASE(704) AMDR_CASE(768)
    AMDR_CASE(832) AMDR_CASE(896) AMDR_CASE(960) AMDR_CASE(1024)
#undef AMDR_CASE
    default: return fail(AMDR_EINVAL, "dense (batched): unsupported dim %d", d);
  }
  if (rc) return rc;
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

// The top-k pass of nq queries over n columns ranks two queries per wave (scores_pair_topk_kernel): a single slab — its
// list is the answer —, a row the pair selector holds in registers, a list of one half-wave, a pair to share the wave.
bool dense_topk_pair_applies(const DenseMfmaPlan& p, long n, int nq, int k) {
  const char* pair_env = getenv("AMDR_TOPK_PAIR");  // "0" pins one query per wave (A/B, tests)
  if (pair_env && pair_env[0] == '0') return false;
  return p.slabs == 1 && n <= 1024 && k <= 32 && nq >= 2;
}

int dense_mfma_launch_topk(const DenseMfmaPlan& p, const float* S, long n, int nq, int k, void* part,
                           float* fin_scores, int64_t* fin_ids, hipStream_t st) {
  const int waves = p.rows_per_slab <= kSelectRowsMax ? 1 : kBW;
  const size_t lds = TopkLds<C32>::bytes(waves, p.cap);
  if (fin_ids && dense_topk_pair_applies(p, n, nq, k)) {
    hipLaunchKernelGGL(scores_pair_topk_kernel, dim3((nq + 1) / 2), dim3(64), (size_t)p.cap * sizeof(C32), st, S, p.ld,
                       n, nq, k, p.cap, fin_scores, (long long*)fin_ids);
    AMDR_HIP(hipGetLastError());
    return AMDR_OK;
  }
  // The batch is the grid's y: pieces (grid_y_pieces).  A piece is handed the pass's nq and its own rows of S, of the result
  // and of every slab's list ([slab][nq][k] + q0 * k), so the pieces fill the one set of lists that the caller's merge reads.
  return grid_y_pieces(nq, [&](int q0, int m) -> int {
    const float* Sp = S + (size_t)q0 * p.ld;
    C32* pp = part ? (C32*)part + (size_t)q0 * k : nullptr;
    float* fs = fin_scores ? fin_scores + (size_t)q0 * k : nullptr;
    long long* fi = fin_ids ? (long long*)fin_ids + (size_t)q0 * k : nullptr;
    if (waves == 1)
      hipLaunchKernelGGL(scores_slab_topk_kernel<1>, dim3(p.slabs, m), dim3(64), lds, st, Sp, p.ld, n, nq, k, p.cap,
                         p.rows_per_slab, pp, fs, fi);
    else
      hipLaunchKernelGGL(scores_slab_topk_kernel<kBW>, dim3(p.slabs, m), dim3(256), lds, st, Sp, p.ld, n, nq, k, p.cap,
                         p.rows_per_slab, pp, fs, fi);
    AMDR_HIP(hipGetLastError());
    return AMDR_OK;
  });
}


// list[q][0 .. count[q]) = the k tiles of query q with the largest M[q][tile], ascending (gate, unres, chosen: see the
// kernel)
int dense_exact_select_launch(const float* M, long ldM, long n_tiles, int m, int k, int list_stride, int* list, int* count,
                              const int* unres, const int* gate, const int64_t* chosen, hipStream_t st) {
  const int tcap = topk_cap(k);
  const size_t lds = TopkLds<C32>::bytes(4, tcap);
  hipLaunchKernelGGL(dense_hi_exact_select_kernel, dim3(m), dim3(chosen ? 64 : 256), lds, st, M, ldM, n_tiles, k, tcap,
                     list_stride, list, count, unres, gate, (const long long*)chosen);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

template <int D8>
static int launch_rescore(const float* X, long n_real, const float* Q, int m, const int* list, const int* count,
                          int list_stride, int max_tiles, long ldS, float* S, hipStream_t st) {
  constexpr int WPB = 4;
  const size_t lds = (size_t)D8 * 8 * sizeof(float) + (size_t)WPB * kStageBytes;
  // grid y: tiles of one query's list, <= AMDR_MAX_K / WPB
  hipLaunchKernelGGL((dense_rescore_tiles_kernel<D8, WPB>), dim3(m, (max_tiles + WPB - 1) / WPB), dim3(WPB * 64), lds, st, X,
                     n_real, Q, list, count, list_stride, ldS, S);
  return AMDR_OK;
}
// S[q][32 t ..] = exact scores of the rows of tile list[q * list_stride + t], t < count[q] (<= max_tiles)
int dense_rescore_tiles_launch(const float* X, long n_real, int d, const float* Q, int m, const int* list, const int* count,
                               int list_stride, int max_tiles, long ldS, float* S, hipStream_t st) {
  int rc = AMDR_OK;
  switch (d) {
#define AMDR_CASE(D) \
  case D: rc = launch_rescore<D / 8>(X, n_real, Q, m, list, count, list_stride, max_tiles, ldS, S, st); break;
    AMDR_CASE(64) AMDR_CASE(128) AMDR_CASE(192) AMDR_CASE(256) AMDR_CASE(320) AMDR_CASE(384)
    AMDR_CASE(448) AMDR_CASE(512) AMDR_CASE(576) AMDR_CASE(640) AMDR_CASE(704) AMDR_CASE(768)
    AMDR_CASE(832) AMDR_CASE(896) AMDR_CASE(960) AMDR_CASE(1024)
#undef AMDR_CASE
    default: return fail(AMDR_EINVAL, "dense (re-scoring): unsupported dim %d", d);
  }
  if (rc) return rc;
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}
// final (scores, row ids) of every query from S (dense_rescore_tiles_launch's layout)
int dense_final_topk_launch(const float* S, long ldS, const int* list, const int* count, int list_stride, int max_tiles,
                            long n_real, int m, int k, float* fin_scores, int64_t* fin_ids, hipStream_t st) {
  const int cap = topk_cap(k);
  const bool one = (long)max_tiles * 32 <= kSelectRowsMax && k <= 64;
  const int waves = one ? 1 : kBW;
  const size_t lds = TopkLds<C32>::bytes(waves, cap);
  if (one)
    hipLaunchKernelGGL(dense_final_topk_kernel<1>, dim3(m), dim3(64), lds, st, S, ldS, list, count, list_stride, n_real, k, cap,
                       fin_scores, (long long*)fin_ids);
  else
    hipLaunchKernelGGL(dense_final_topk_kernel<kBW>, dim3(m), dim3(kBW * 64), lds, st, S, ldS, list, count, list_stride, n_real,
                       k, cap, fin_scores, (long long*)fin_ids);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

}  // namespace amdr

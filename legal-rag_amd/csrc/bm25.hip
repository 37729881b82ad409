// BM25 channel: Okapi scoring over term-major CSR postings + fused top-k.
//
// Replaces `BM25Okapi.get_scores(tokens)` and the full Python sort at
// legalrag/retrieval/bm25_retriever.py:74-75.  One block owns (query, slab of
// documents): the slab's fp64 score vector lives in LDS, the query's tokens are
// walked IN QUERY ORDER (duplicates included) and each token's posting list is
// scattered into it by all threads — a posting list holds a document at most
// once, so there are no write conflicts and every document receives its
// contributions in exactly the order rank_bm25's `score += ...` loop applies
// them.  fp64, compiled with -ffp-contract=off: bit-identical scores.  The
// slab is then ranked in place (score desc, ties -> lower doc id, zero-score
// docs included) with the wave-level selector of topk.hpp.
// Algorithmic bytes per query: sum_t df(t)*12 (posting doc id + precomputed fp64 factor).
//
// amdr_bm25_add appends documents.  N and avgdl are corpus-global, so every factor changes: the add is ONE pass over the
// resident postings (bm25_merge_kernel) that interleaves each term's old list with the added documents' list behind it
// and recomputes post_w with the new avgdl, next to the data.  post_tf and doc_len stay resident for that (16 B per
// posting instead of 12, + 4 B per document).  The new arrays are built beside the old ones and swapped in after the
// stream has finished: a failed add leaves the handle as it was.
//
// amdr_bm25_remove takes documents out, with the same contract (the handle is what create makes of the survivors' index)
// and the same build-beside-and-swap.  It is a stream compaction of the postings in two passes over them, divided by
// tiles of kBmAddTile OLD postings, with no atomics (compact.hpp, bm25_remove_rule.hpp):
//   bm25_rm_docmap_kernel   doc_new[d] = -1 or d minus the remove ids below d; doc_len compacted through it
//   bm25_rm_count_kernel    per tile: the keep flags scanned in LDS -> each posting's rank inside its tile (2 B) + the
//                           tile's count                                         reads 4 B + a 4 B gather, writes 2 B
//   compact_scan_i64_kernel tile counts -> tile bases (the last one is nnz_new)
//   bm25_rm_terms_kernel    per old term: rank of its first posting (rank_at), surviving count -> df_new[term_map[t]];
//                           a term mapped to -1 with a surviving posting raises the error flag
//   compact_scan_i64_kernel df_new -> the new term_ptr
//   (the host reads nnz_new and the flag here, and allocates the new posting arrays at their exact size)
//   bm25_rm_scatter_kernel  per tile: a kept posting of term t goes to new_ptr[term_map[t]] + rank - rank_at[t] with its
//                           mapped document, its tf and the recomputed factor    reads 10 B + two 4 B gathers, writes 16 B
#include "common.hpp"
#include "topk.hpp"
#include "topk_merge.hpp"

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>


#include "bm25_add_rule.hpp"
#include "bm25_core.hpp"
#include "bm25_remove_rule.hpp"
#include "compact.hpp"

using namespace amdr;

struct amdr_bm25 {
  int device = 0;
  int64_t n_terms = 0, n_docs = 0, nnz = 0, adds = 0, removes = 0;
  double avgdl = 0, k1 = 1.5, b = 0.75;
  double add_kernel_ms = -1;     // event time of the last add's merge kernel (amdr_bm25_add_kernel_ms)
  double remove_kernel_ms = -1;  // summed event time of the last remove's passes (amdr_bm25_remove_kernel_ms)
  long long* term_ptr = nullptr;
  int* post_doc = nullptr;
  double* post_w = nullptr;  // tf*(k1+1) / (tf + k1*(1 - b + b*len/avgdl)) per posting, fp64
  double* idf = nullptr;
  int* post_tf = nullptr;  // resident for amdr_bm25_add: the factors are recomputed from (tf, doc_len, avgdl)
  int* doc_len = nullptr;
  hipStream_t stream = nullptr;
  std::mutex mu;
  DevBuf part[2], qterms, qptr, sbuf, ibuf, full;  // part[0]: "_device" calls, part[1]: host-pointer calls (see dense.hip)
  DevBuf ticket;  // 64 zeroed ints: arrival counters of the one-launch serving step (dense_tail.hip), self-resetting
};

namespace {

constexpr int kSlabMax = 4096;  // docs per block: 32 KiB of fp64 scores in LDS

struct BmPlan {
  int slab, nslabs, cap, cap_merge, waves;
  size_t lds, part_bytes;
};

void bm_plan(int64_t n_docs, int nq, int k, BmPlan* p) {
  // One wave per (query, slab) in every shape (measured on 1 260 ... 9 000 documents, 8 192
  // queries: the 4-wave block with its per-token block barriers and list combine lost to one
  // wave at every size — e.g. 1 260 docs, k = 10: 237 -> 74 us).  Shallow k (bm_use_argmax):
  // slabs of <= 2 048 documents ranked by the register arg-max (<= 32 scores per lane), its k
  // winners parked in a short list; otherwise slabs of <= 4 096 ranked by the staged selector.
  // Slabs are balanced (3 000 documents = 2 x 1 536, not 2 048 + 952) and merged by
  // merge_parts_kernel (topk_merge.hip).
  const int64_t n = n_docs > 0 ? n_docs : 1;
  auto balanced = [&](int slab_max) {
    p->nslabs = (int)((n + slab_max - 1) / slab_max);
    p->slab = (int)(((n + p->nslabs - 1) / p->nslabs + 15) / 16 * 16);
    if (p->slab > slab_max) p->slab = slab_max;
    p->nslabs = (int)((n + p->slab - 1) / p->slab);
  };
  balanced(kBmOneWaveDocs);
  const bool argmax = bm_use_argmax(k, p->slab);
  if (!argmax) balanced(kSlabMax);
  p->waves = 1;
  p->cap_merge = topk_cap(k);
  p->cap = argmax ? (k <= 16 ? 16 : kBmArgmaxK) : p->cap_merge;
  p->lds = (size_t)p->slab * sizeof(double) + TopkLds<C64>::bytes(p->waves, p->cap, kBmCnts) +
           128 * sizeof(long) + 8;  // token table (3 x kBmTok x 8 B) / ranking scratch (2 x 64 x 8 B)
  p->part_bytes = (size_t)p->nslabs * nq * k * sizeof(C64);
}

// Slab-list bytes a "_device" call of nq queries at depth k uses (bm_run), and what amdr_bm25_reserve(nq_max, k_max)
// sizes for every call within it: the maximum over every depth <= k_max — the slab size depends on k (bm_use_argmax:
// slabs of <= 2 048 documents for a shallow k, <= 4 096 otherwise), so a SMALLER k can need more list space (100 000 documents:
// k = 17 takes 25 slabs, k = 16 49).  Linear in nq: nq_max covers every smaller batch.
size_t bm_part_bytes(int64_t n_docs, int nq, int k) {
  BmPlan p;
  bm_plan(n_docs, nq, k, &p);
  return p.part_bytes;
}
size_t bm_reserve_bytes(int64_t n_docs, int nq_max, int k_max) {
  size_t need = 0;
  for (int k = 1; k <= k_max; ++k) {
    const size_t b = bm_part_bytes(n_docs, nq_max, k);
    need = b > need ? b : need;
  }
  return need;
}

// AMDR_BM25_SELECT=0 pins the exact arg-max rounds (A/B and tests of the fallback path)
static bool bm_select_enabled() {
  const char* e = getenv("AMDR_BM25_SELECT");
  return !(e && e[0] == '0');
}

int bm_run(amdr_bm25* h, int ws, const int* q_terms_dev, const long long* q_ptr_dev, int nq, int k, double* scores_dev,
           int64_t* ids_dev, double* full_dev, hipStream_t st) {
  BmPlan p;
  bm_plan(h->n_docs, nq, k, &p);
  C64* part = nullptr;
  if (scores_dev) {
    int rc = h->part[ws].ensure(bm_part_bytes(h->n_docs, nq, k));
    if (rc) return rc;
    part = h->part[ws].as<C64>();
  }
  const bool direct = scores_dev && p.nslabs == 1;  // single slab: the block's list is the answer
  double* fs = direct ? scores_dev : nullptr;
  long long* fi = direct ? (long long*)ids_dev : nullptr;
  if (direct) part = nullptr;
  if (p.lds > 48 * 1024) {  // never with the slab limits of bm_plan (4 096 x 8 B + lists < 48 KiB); guard for edits
    return fail(AMDR_EINVAL, "bm25: slab needs %zu B of LDS", p.lds);
  }
#define AMDR_BM_LAUNCH(NVT)                                                                                          \
  hipLaunchKernelGGL((bm25_score_topk_kernel<1, NVT>), dim3(p.nslabs, nq), dim3(64), p.lds, st, h->term_ptr,         \
                     h->post_doc, h->post_w, h->idf, (long)h->n_terms, (long)h->n_docs, q_terms_dev, q_ptr_dev, nq, k, \
                     p.cap, p.slab, bm_select_enabled() ? 1 : 0, full_dev, part, fs, fi)
  const int nv = bm_use_argmax(k, p.slab) ? (p.slab + 63) / 64 : 1;  // the staged selector needs no register bucket
  if (nv <= 4) AMDR_BM_LAUNCH(4);
  else if (nv <= 8) AMDR_BM_LAUNCH(8);
  else if (nv <= 10) AMDR_BM_LAUNCH(10);
  else if (nv <= 16) AMDR_BM_LAUNCH(16);
  else if (nv <= 20) AMDR_BM_LAUNCH(20);
  else AMDR_BM_LAUNCH(32);
#undef AMDR_BM_LAUNCH
  AMDR_HIP(hipGetLastError());
  if (scores_dev && !direct) return launch_merge_packed(part, p.nslabs, nq, k, p.cap_merge, scores_dev, ids_dev, st);
  return AMDR_OK;
}

}  // namespace
namespace amdr {
int bm25_small_raw(amdr_bm25_t* h, int nq, int k, Bm25Raw* out) {
  if (!h->ticket.p) return fail(AMDR_EINVAL, "bm25: handle without arrival counters");
  BmPlan p;
  bm_plan(h->n_docs, nq, k, &p);
  out->term_ptr = h->term_ptr;
  out->post_doc = h->post_doc;
  out->post_w = h->post_w;
  out->idf = h->idf;
  out->n_terms = (long)h->n_terms;
  out->n_docs = (long)h->n_docs;
  out->ticket = h->ticket.as<int>();
  out->slab = p.slab;
  out->nslabs = p.nslabs;
  out->cap = p.cap;
  out->lds = p.lds;
  out->argmax = bm_use_argmax(k, p.slab);
  out->nvt = out->argmax ? (p.slab + 63) / 64 : 1;
  out->select_on = bm_select_enabled();
  return AMDR_OK;
}
std::mutex& bm25_mutex(amdr_bm25_t* h) { return h->mu; }
int bm25_device_of(const amdr_bm25_t* h) { return h->device; }
}  // namespace amdr
namespace {

template <class T>
int upload(T** dst, const T* src, size_t count) {
  *dst = nullptr;
  size_t bytes = (count + 1) * sizeof(T);  // one padding element: clamped prefetch reads may touch [count]
  AMDR_HIP(hipMalloc((void**)dst, bytes));
  if (count) AMDR_HIP(hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
  return AMDR_OK;
}

// ---- amdr_bm25_add: term table and merge ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bm25_term_ptr_sum_kernel(const long long* __restrict__ old_ptr, long n_terms_old,
                                                                const long long* __restrict__ add_ptr, long n_terms_new,
                                                                long long* __restrict__ new_ptr) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t <= n_terms_new) new_ptr[t] = bm_add_term_ptr(old_ptr, n_terms_old, add_ptr, t);
}

// One block = kBmAddTile consecutive OUTPUT postings (work is divided by postings, not by terms: a Zipfian head term holds
// every document and a wave per term would serialise on it).  Thread 0 finds the terms of the tile's first and last
// posting by binary search in the new term table; the table entries between them go to LDS (a tile holds at most
// kBmAddTile terms that have postings; a window widened by terms WITHOUT postings beyond the LDS room is searched in
// global memory instead), and every posting finds its term there.  A posting reads 8 B (doc, tf) from the old list or
// the add's, gathers 4 B of doc_len, and writes 16 B (doc, tf, factor).  No atomics: the result is deterministic.
__global__ __launch_bounds__(kBmAddThreads) void bm25_merge_kernel(
    const long long* __restrict__ new_ptr, long n_terms_new, const long long* __restrict__ old_ptr, long n_terms_old,
    const int* __restrict__ old_doc, const int* __restrict__ old_tf, const long long* __restrict__ add_ptr,
    const int* __restrict__ add_doc, const int* __restrict__ add_tf, const int* __restrict__ doc_len /* new */,
    int n_docs_old, long long nnz_new, double avgdl, double k1, double b, int* __restrict__ out_doc,
    int* __restrict__ out_tf, double* __restrict__ out_w) {
  __shared__ long long win[kBmAddTile + 2];
  __shared__ long t_first, t_last;
  const int tid = threadIdx.x;
  const long long p0 = (long long)blockIdx.x * kBmAddTile;
  long long p1 = p0 + kBmAddTile;  // exclusive
  if (p1 > nnz_new) p1 = nnz_new;
  if (p0 >= p1) return;
  if (tid == 0) {
    long a, z;
    bm_add_tile_terms(new_ptr, n_terms_new, p0, p1, &a, &z);
    t_first = a;
    t_last = z;
  }
  __syncthreads();
  const long t0 = t_first, t1 = t_last;
  const bool in_lds = bm_add_window_fits(t0, t1);
  if (in_lds) {
    for (long i = tid; i <= t1 - t0 + 1; i += kBmAddThreads) win[i] = new_ptr[t0 + i];
    __syncthreads();
  }
  const long long* tab = in_lds ? win : new_ptr;
  const long base = in_lds ? t0 : 0;
#pragma unroll
  for (int u = 0; u < kBmAddPerThread; ++u) {
    const long long p = p0 + (long long)u * kBmAddThreads + tid;
    if (p < p1) {
      const long t = bm_add_term_of(tab, base, t0, t1, p);
      bool from_add;
      const long long src = bm_add_source(p, tab[t - base], t, old_ptr, n_terms_old, add_ptr, &from_add);
      const int doc = from_add ? add_doc[src] + n_docs_old : old_doc[src];
      const int tf = from_add ? add_tf[src] : old_tf[src];
      out_doc[p] = doc;
      out_tf[p] = tf;
      out_w[p] = bm25_factor(tf, doc_len[doc], avgdl, k1, b);
    }
  }
}

// ---- amdr_bm25_remove: document map, tile ranks, term table, scatter -------------------------------------------------
__global__ __launch_bounds__(256) void bm25_rm_docmap_kernel(const long long* __restrict__ remove_ids, long n_remove,
                                                             const int* __restrict__ doc_len_old, long n_docs_old,
                                                             int* __restrict__ doc_new, int* __restrict__ doc_len_new) {
  const long d = (long)blockIdx.x * 256 + threadIdx.x;
  if (d >= n_docs_old) return;
  const int nd = bm_rm_doc_new(remove_ids, n_remove, d);
  doc_new[d] = nd;
  if (nd >= 0) doc_len_new[nd] = doc_len_old[d];
}

// One block = one tile of kBmAddTile consecutive OLD postings (thread tid owns postings tid, tid + 256, ...): which of
// them survive, each one's rank among the tile's survivors (compact_tile_scan) and the tile's count.
__global__ __launch_bounds__(kBmAddThreads) void bm25_rm_count_kernel(const int* __restrict__ old_doc, long long nnz_old,
                                                                      const int* __restrict__ doc_new,
                                                                      unsigned short* __restrict__ tile_rank,
                                                                      long long* __restrict__ tile_cnt) {
  __shared__ int lds[kBmAddTile + kBmAddThreads / 64 + 1];
  const int tid = threadIdx.x;
  const long long p0 = (long long)blockIdx.x * kBmAddTile;
  unsigned keep = 0;
#pragma unroll
  for (int u = 0; u < kBmAddPerThread; ++u) {
    const long long p = p0 + (long long)u * kBmAddThreads + tid;
    if (p < nnz_old && doc_new[old_doc[p]] >= 0) keep |= 1u << u;
  }
  int rank[kBmAddPerThread];
  const int total = compact_tile_scan<kBmAddThreads, kBmAddPerThread>(keep, lds, rank);
#pragma unroll
  for (int u = 0; u < kBmAddPerThread; ++u) {
    const long long p = p0 + (long long)u * kBmAddThreads + tid;
    if (p < nnz_old) tile_rank[p] = (unsigned short)rank[u];
  }
  if (tid == 0) tile_cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void bm25_rm_terms_kernel(const long long* __restrict__ old_ptr, long n_terms_old,
                                                            long long nnz_old, const long long* __restrict__ tile_base,
                                                            const unsigned short* __restrict__ tile_rank,
                                                            const int* __restrict__ term_map, long long* __restrict__ rank_at,
                                                            long long* __restrict__ df_new, int* __restrict__ bad) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t <= n_terms_old) bm_rm_term_entry(t, n_terms_old, old_ptr, nnz_old, tile_base, tile_rank, term_map, rank_at, df_new, bad);
}

// One block = one tile of OLD postings again.  The tile's terms are found as in bm25_merge_kernel, in the OLD term table
// (a window of it in LDS; a window widened beyond the LDS room by terms without postings is searched in global memory).
// A surviving posting reads 8 B (doc, tf) + 2 B of rank, gathers doc_new and doc_len (4 B each) and the few table entries
// of its term, and writes 16 B (doc, tf, factor) at bm_rm_dest.  Every destination is a sum of counts: no atomics.
__global__ __launch_bounds__(kBmAddThreads) void bm25_rm_scatter_kernel(
    const long long* __restrict__ old_ptr, long n_terms_old, const int* __restrict__ old_doc, const int* __restrict__ old_tf,
    long long nnz_old, const int* __restrict__ doc_new, const int* __restrict__ doc_len /* new */,
    const long long* __restrict__ tile_base, const unsigned short* __restrict__ tile_rank,
    const long long* __restrict__ rank_at, const long long* __restrict__ new_ptr, const int* __restrict__ term_map,
    long long nnz_new, double avgdl, double k1, double b, int* __restrict__ out_doc, int* __restrict__ out_tf,
    double* __restrict__ out_w) {
  __shared__ long long win[kBmAddTile + 2];
  __shared__ long t_first, t_last;
  const int tid = threadIdx.x;
  const long long p0 = (long long)blockIdx.x * kBmAddTile;
  long long p1 = p0 + kBmAddTile;  // exclusive
  if (p1 > nnz_old) p1 = nnz_old;
  if (p0 >= p1) return;
  if (tid == 0) {
    long a, z;
    bm_add_tile_terms(old_ptr, n_terms_old, p0, p1, &a, &z);
    t_first = a;
    t_last = z;
  }
  __syncthreads();
  const long t0 = t_first, t1 = t_last;
  const bool in_lds = bm_add_window_fits(t0, t1);
  if (in_lds) {
    for (long i = tid; i <= t1 - t0 + 1; i += kBmAddThreads) win[i] = old_ptr[t0 + i];
    __syncthreads();
  }
  const long long* tab = in_lds ? win : old_ptr;
  const long base = in_lds ? t0 : 0;
#pragma unroll
  for (int u = 0; u < kBmAddPerThread; ++u) {
    const long long p = p0 + (long long)u * kBmAddThreads + tid;
    if (p < p1) {
      const int doc = doc_new[old_doc[p]];
      if (doc >= 0) {
        const long t = bm_add_term_of(tab, base, t0, t1, p);
        const long long dst = bm_rm_dest(p, t, nnz_old, tile_base, tile_rank, rank_at, new_ptr, term_map);
        if (dst >= 0 && dst < nnz_new) {  // (always, after the host's checks and the terms kernel's flag)
          const int tf = old_tf[p];
          out_doc[dst] = doc;
          out_tf[dst] = tf;
          out_w[dst] = bm25_factor(tf, doc_len[doc], avgdl, k1, b);
        }
      }
    }
  }
}

// device arrays of an add or a remove in the making: freed unless they were handed to the handle
struct BmAddBufs {
  void* p[16] = {};
  ~BmAddBufs() {
    for (void* q : p)
      if (q) (void)hipFree(q);
  }
  int alloc(int i, size_t bytes) {
    if (hipMalloc(&p[i], bytes) != hipSuccess) {
      (void)hipGetLastError();
      p[i] = nullptr;
      return fail(AMDR_ENOMEM, "bm25_add: device allocation of %zu B failed", bytes);
    }
    return AMDR_OK;
  }
};

}  // namespace

extern "C" {

int amdr_bm25_create(const int64_t* term_ptr, const int32_t* post_doc, const int32_t* post_tf, const double* idf,
                     const int32_t* doc_len, int64_t n_terms, int64_t n_docs, double avgdl, double k1, double b,
                     int32_t device, amdr_bm25_t** out) {
  AMDR_REQUIRE(out != nullptr, "bm25_create: out is null");
  *out = nullptr;
  AMDR_REQUIRE(term_ptr && idf && doc_len, "bm25_create: null array");
  AMDR_REQUIRE(n_terms >= 0 && n_docs >= 1 && n_docs < (1ll << 31), "bm25_create: bad sizes");
  AMDR_REQUIRE(n_terms < (1ll << 31), "bm25_create: too many terms");
  AMDR_REQUIRE(term_ptr[0] == 0, "bm25_create: term_ptr[0] != 0");
  for (int64_t t = 0; t < n_terms; ++t)
    AMDR_REQUIRE(term_ptr[t + 1] >= term_ptr[t], "bm25_create: term_ptr not monotone at %lld", (long long)t);
  // rank_bm25 never produces a non-finite idf; the rankings use -inf as "no document" and order NaN by convention
  for (int64_t t = 0; t < n_terms; ++t)
    AMDR_REQUIRE(std::isfinite(idf[t]), "bm25_create: idf of term %lld is not finite", (long long)t);
  const int64_t nnz = term_ptr[n_terms];
  AMDR_REQUIRE(nnz == 0 || (post_doc && post_tf), "bm25_create: null postings");
  for (int64_t t = 0; t < n_terms; ++t)
    for (int64_t p = term_ptr[t]; p < term_ptr[t + 1]; ++p) {
      AMDR_REQUIRE(post_doc[p] >= 0 && post_doc[p] < n_docs, "bm25_create: posting %lld doc out of range", (long long)p);
      AMDR_REQUIRE(p == term_ptr[t] || post_doc[p] > post_doc[p - 1],
                   "bm25_create: postings of term %lld not strictly ascending", (long long)t);
    }
  int rc = check_device(device);
  if (rc) return rc;
  amdr_bm25* h = new (std::nothrow) amdr_bm25();
  if (!h) return fail(AMDR_ENOMEM, "bm25_create: host alloc");
  h->device = device;
  h->n_terms = n_terms;
  h->n_docs = n_docs;
  h->nnz = nnz;
  h->avgdl = avgdl;
  h->k1 = k1;
  h->b = b;
  // Per-posting factor of rank_bm25's expression, operand for operand in numpy's order
  // (this translation unit is built with -ffp-contract=off; IEEE fp64 mul/add/div are
  // correctly rounded on the host as on the device, so the value is the one numpy computes).
  std::vector<double> pw((size_t)nnz);
  for (int64_t p = 0; p < nnz; ++p) pw[(size_t)p] = bm25_factor(post_tf[p], doc_len[post_doc[p]], avgdl, k1, b);
  rc = upload(&h->term_ptr, (const long long*)term_ptr, (size_t)n_terms + 1);
  if (!rc) rc = upload(&h->post_doc, post_doc, (size_t)nnz);
  if (!rc) rc = upload(&h->post_w, pw.data(), (size_t)nnz);
  if (!rc) rc = upload(&h->idf, idf, (size_t)n_terms);
  if (!rc) rc = upload(&h->post_tf, post_tf, (size_t)nnz);
  if (!rc) rc = upload(&h->doc_len, doc_len, (size_t)n_docs);
  if (!rc && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
    rc = fail(AMDR_EHIP, "bm25_create: stream");
  if (!rc) rc = h->ticket.ensure(64 * sizeof(int));  // arrival counters of the one-launch serving step: zero between launches
  if (!rc && hipMemset(h->ticket.p, 0, 64 * sizeof(int)) != hipSuccess) rc = fail(AMDR_EHIP, "bm25_create: memset");
  if (rc) {
    amdr_bm25_destroy(h);
    return rc;
  }
  *out = h;
  return AMDR_OK;
}

int amdr_bm25_ndocs(const amdr_bm25_t* h, int64_t* n) {
  AMDR_REQUIRE(h && n, "bm25_ndocs: null");
  *n = h->n_docs;
  return AMDR_OK;
}

int amdr_bm25_reserve(amdr_bm25_t* h, int32_t nq_max, int32_t k_max, int64_t total_terms_max) {
  AMDR_REQUIRE(h != nullptr, "bm25_reserve: null handle");
  AMDR_REQUIRE(nq_max >= 1 && k_max >= 1 && k_max <= AMDR_MAX_K && total_terms_max >= 0, "bm25_reserve: bad sizes");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  int rc = h->part[0].ensure(bm_reserve_bytes(h->n_docs, nq_max, k_max));
  if (!rc) rc = h->qterms.ensure((size_t)(total_terms_max + 1) * sizeof(int));
  if (!rc) rc = h->qptr.ensure((size_t)(nq_max + 1) * sizeof(long long));
  if (!rc) rc = h->sbuf.ensure((size_t)nq_max * k_max * sizeof(double));
  if (!rc) rc = h->ibuf.ensure((size_t)nq_max * k_max * sizeof(int64_t));
  return rc;
}

int amdr_bm25_workspace_plan(int64_t n_docs, int32_t nq_max, int32_t k_max, int32_t nq, int32_t k, int64_t* out2) {
  AMDR_REQUIRE(out2 != nullptr, "bm25_workspace_plan: null");
  AMDR_REQUIRE(n_docs >= 1 && n_docs < (1ll << 31), "bm25_workspace_plan: bad n_docs");
  AMDR_REQUIRE(nq_max >= 1 && k_max >= 1 && k_max <= AMDR_MAX_K && nq >= 1 && k >= 1 && k <= AMDR_MAX_K,
               "bm25_workspace_plan: bad sizes");
  out2[0] = (int64_t)bm_reserve_bytes(n_docs, nq_max, k_max);
  out2[1] = (int64_t)bm_part_bytes(n_docs, nq, k);
  return AMDR_OK;
}

int amdr_bm25_plan_info(const amdr_bm25_t* h, int32_t nq, int32_t k, char* buf, int32_t buf_len) {
  AMDR_REQUIRE(h && buf && buf_len > 0, "bm25_plan_info: null");
  AMDR_REQUIRE(nq >= 1 && k >= 1 && k <= AMDR_MAX_K, "bm25_plan_info: bad sizes");
  BmPlan p;
  bm_plan(h->n_docs, nq, k, &p);
  snprintf(buf, buf_len, "bm25_score_topk_kernel slabs=%d of <= %d documents, ranked by %s%s", p.nslabs, p.slab,
           bm_use_argmax(k, p.slab) ? "the register arg-max rounds" : "the staged selector",
           p.nslabs == 1 ? " (one slab: direct)" : " + merge_parts_kernel");
  return AMDR_OK;
}

static int bm_check(const amdr_bm25* h, const void* qt, const void* qp, int nq, int k) {
  AMDR_REQUIRE(h != nullptr, "bm25: null handle");
  AMDR_REQUIRE(nq >= 0, "bm25: nq=%d", nq);
  AMDR_REQUIRE(k >= 1 && k <= AMDR_MAX_K, "bm25: k=%d outside [1,%d]", k, AMDR_MAX_K);
  AMDR_REQUIRE(nq == 0 || qp, "bm25: null q_ptr");
  (void)qt;
  return AMDR_OK;
}

int amdr_bm25_search_device(amdr_bm25_t* h, const int32_t* q_terms_dev, const int64_t* q_ptr_dev, int32_t nq,
                            int32_t k, double* scores_dev, int64_t* ids_dev, void* stream) {
  int rc = bm_check(h, q_terms_dev, q_ptr_dev, nq, k);
  if (rc) return rc;
  AMDR_REQUIRE(nq == 0 || (scores_dev && ids_dev), "bm25: null output");
  if (nq == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  return bm_run(h, 0, q_terms_dev, (const long long*)q_ptr_dev, nq, k, scores_dev, ids_dev, nullptr, (hipStream_t)stream);
}

static int bm_stage_queries(amdr_bm25* h, const int32_t* q_terms, const int64_t* q_ptr, int nq) {
  AMDR_REQUIRE(q_ptr[0] == 0, "bm25: q_ptr[0] != 0");
  for (int i = 0; i < nq; ++i) AMDR_REQUIRE(q_ptr[i + 1] >= q_ptr[i], "bm25: q_ptr not monotone");
  const int64_t tot = q_ptr[nq];
  AMDR_REQUIRE(tot == 0 || q_terms, "bm25: null q_terms");
  int rc = h->qterms.ensure((size_t)(tot + 1) * sizeof(int));
  if (!rc) rc = h->qptr.ensure((size_t)(nq + 1) * sizeof(long long));
  if (rc) return rc;
  if (tot) AMDR_HIP(hipMemcpyAsync(h->qterms.p, q_terms, (size_t)tot * sizeof(int), hipMemcpyHostToDevice, h->stream));
  AMDR_HIP(hipMemcpyAsync(h->qptr.p, q_ptr, (size_t)(nq + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  return AMDR_OK;
}

int amdr_bm25_search(amdr_bm25_t* h, const int32_t* q_terms, const int64_t* q_ptr, int32_t nq, int32_t k,
                     double* scores_host, int64_t* ids_host) {
  int rc = bm_check(h, q_terms, q_ptr, nq, k);
  if (rc) return rc;
  AMDR_REQUIRE(nq == 0 || (scores_host && ids_host), "bm25: null output");
  if (nq == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  if ((rc = bm_stage_queries(h, q_terms, q_ptr, nq))) return rc;
  if ((rc = h->sbuf.ensure((size_t)nq * k * sizeof(double)))) return rc;
  if ((rc = h->ibuf.ensure((size_t)nq * k * sizeof(int64_t)))) return rc;
  rc = bm_run(h, 1, h->qterms.as<int>(), h->qptr.as<long long>(), nq, k, h->sbuf.as<double>(), h->ibuf.as<int64_t>(),
              nullptr, h->stream);
  if (rc) return rc;
  AMDR_HIP(hipMemcpyAsync(scores_host, h->sbuf.p, (size_t)nq * k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipMemcpyAsync(ids_host, h->ibuf.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipStreamSynchronize(h->stream));
  return AMDR_OK;
}

int amdr_bm25_scores(amdr_bm25_t* h, const int32_t* q_terms, const int64_t* q_ptr, int32_t nq, double* scores_host) {
  int rc = bm_check(h, q_terms, q_ptr, nq, 1);
  if (rc) return rc;
  AMDR_REQUIRE(nq == 0 || scores_host, "bm25_scores: null output");
  if (nq == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  if ((rc = bm_stage_queries(h, q_terms, q_ptr, nq))) return rc;
  if ((rc = h->full.ensure((size_t)nq * h->n_docs * sizeof(double)))) return rc;
  rc = bm_run(h, 1, h->qterms.as<int>(), h->qptr.as<long long>(), nq, 1, nullptr, nullptr, h->full.as<double>(),
              h->stream);
  if (rc) return rc;
  AMDR_HIP(hipMemcpyAsync(scores_host, h->full.p, (size_t)nq * h->n_docs * sizeof(double), hipMemcpyDeviceToHost,
                          h->stream));
  AMDR_HIP(hipStreamSynchronize(h->stream));
  return AMDR_OK;
}

int amdr_bm25_add(amdr_bm25_t* h, const int64_t* term_ptr_add, const int32_t* post_doc_add, const int32_t* post_tf_add,
                  const double* idf, const int32_t* doc_len_add, int64_t n_terms, int64_t n_add, double avgdl) {
  AMDR_REQUIRE(h != nullptr, "bm25_add: null handle");
  AMDR_REQUIRE(n_add >= 0, "bm25_add: n_add=%lld", (long long)n_add);
  if (n_add == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  const int bad = bm_add_validate(term_ptr_add, post_doc_add, post_tf_add, idf, doc_len_add, n_terms, n_add, avgdl,
                                  h->n_terms, h->n_docs);
  AMDR_REQUIRE(bad == kBmAddOk, "bm25_add: %s", bm_add_error_text(bad));
  AMDR_HIP(hipSetDevice(h->device));
  const int64_t nnz_add = term_ptr_add[n_terms], nnz_new = h->nnz + nnz_add, n_docs_new = h->n_docs + n_add;
  // The new arrays beside the old ones (one padding element each, as upload() leaves: the scoring kernel's clamped
  // prefetch may touch [count]); 6..8: the add's own CSR on the device, freed when the call returns.
  enum { TP, PD, PT, PW, IDF, DL, ATP, APD, APT };
  BmAddBufs nb;
  int rc = nb.alloc(TP, (size_t)(n_terms + 2) * sizeof(long long));
  if (!rc) rc = nb.alloc(PD, (size_t)(nnz_new + 1) * sizeof(int));
  if (!rc) rc = nb.alloc(PT, (size_t)(nnz_new + 1) * sizeof(int));
  if (!rc) rc = nb.alloc(PW, (size_t)(nnz_new + 1) * sizeof(double));
  if (!rc) rc = nb.alloc(IDF, (size_t)(n_terms + 1) * sizeof(double));
  if (!rc) rc = nb.alloc(DL, (size_t)(n_docs_new + 1) * sizeof(int));
  if (!rc) rc = nb.alloc(ATP, (size_t)(n_terms + 1) * sizeof(long long));
  if (!rc) rc = nb.alloc(APD, (size_t)(nnz_add + 1) * sizeof(int));
  if (!rc) rc = nb.alloc(APT, (size_t)(nnz_add + 1) * sizeof(int));
  if (rc) return rc;
  hipStream_t st = h->stream;
  AMDR_HIP(hipMemcpyAsync(nb.p[ATP], term_ptr_add, (size_t)(n_terms + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
  if (nnz_add) {
    AMDR_HIP(hipMemcpyAsync(nb.p[APD], post_doc_add, (size_t)nnz_add * sizeof(int), hipMemcpyHostToDevice, st));
    AMDR_HIP(hipMemcpyAsync(nb.p[APT], post_tf_add, (size_t)nnz_add * sizeof(int), hipMemcpyHostToDevice, st));
  }
  if (n_terms) AMDR_HIP(hipMemcpyAsync(nb.p[IDF], idf, (size_t)n_terms * sizeof(double), hipMemcpyHostToDevice, st));
  AMDR_HIP(hipMemcpyAsync(nb.p[DL], h->doc_len, (size_t)h->n_docs * sizeof(int), hipMemcpyDeviceToDevice, st));
  AMDR_HIP(hipMemcpyAsync((int*)nb.p[DL] + h->n_docs, doc_len_add, (size_t)n_add * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(bm25_term_ptr_sum_kernel, dim3((unsigned)((n_terms + 1 + 255) / 256)), dim3(256), 0, st, h->term_ptr,
                     (long)h->n_terms, (const long long*)nb.p[ATP], (long)n_terms, (long long*)nb.p[TP]);
  AMDR_HIP(hipGetLastError());
  // the merge kernel between two events (amdr_bm25_add_kernel_ms); an event that cannot be made only loses the time
  hipEvent_t ev[2] = {nullptr, nullptr};
  struct EvGuard {
    hipEvent_t* e;
    ~EvGuard() {
      for (int i = 0; i < 2; ++i)
        if (e[i]) (void)hipEventDestroy(e[i]);
    }
  } ev_guard{ev};
  if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess) {
    (void)hipGetLastError();
    if (ev[0]) (void)hipEventDestroy(ev[0]);
    ev[0] = ev[1] = nullptr;
  }
  if (nnz_new > 0) {
    const long long blocks = (nnz_new + kBmAddTile - 1) / kBmAddTile;
    AMDR_REQUIRE(blocks < (1ll << 31), "bm25_add: %lld postings exceed the merge grid", (long long)nnz_new);
    if (ev[0]) AMDR_HIP(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(bm25_merge_kernel, dim3((unsigned)blocks), dim3(kBmAddThreads), 0, st, (const long long*)nb.p[TP],
                       (long)n_terms, h->term_ptr, (long)h->n_terms, h->post_doc, h->post_tf, (const long long*)nb.p[ATP],
                       (const int*)nb.p[APD], (const int*)nb.p[APT], (const int*)nb.p[DL], (int)h->n_docs,
                       (long long)nnz_new, avgdl, h->k1, h->b, (int*)nb.p[PD], (int*)nb.p[PT], (double*)nb.p[PW]);
    AMDR_HIP(hipGetLastError());
    if (ev[0]) AMDR_HIP(hipEventRecord(ev[1], st));
  }
  AMDR_HIP(hipStreamSynchronize(st));
  float ms = -1.f;
  if (!(nnz_new > 0 && ev[0] && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)) ms = -1.f;
  h->add_kernel_ms = (double)ms;
  // the swap: from here on nothing can fail (the old arrays take the new ones' places in nb and are freed with it)
  auto swap_in = [&](auto*& held, int i) {
    void* old = (void*)held;
    held = reinterpret_cast<std::remove_reference_t<decltype(held)>>(nb.p[i]);
    nb.p[i] = old;
  };
  swap_in(h->term_ptr, TP);
  swap_in(h->post_doc, PD);
  swap_in(h->post_tf, PT);
  swap_in(h->post_w, PW);
  swap_in(h->idf, IDF);
  swap_in(h->doc_len, DL);
  h->n_terms = n_terms;
  h->n_docs = n_docs_new;
  h->nnz = nnz_new;
  h->avgdl = avgdl;
  ++h->adds;
  return AMDR_OK;
}

int amdr_bm25_remove(amdr_bm25_t* h, const int64_t* remove_ids, int64_t n_remove, const int32_t* term_map,
                     int64_t n_terms_new, const double* idf, double avgdl) {
  AMDR_REQUIRE(h != nullptr, "bm25_remove: null handle");
  AMDR_REQUIRE(n_remove >= 0, "bm25_remove: n_remove=%lld", (long long)n_remove);
  if (n_remove == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  const int bad = bm_rm_validate(remove_ids, n_remove, term_map, n_terms_new, idf, avgdl, h->n_terms, h->n_docs);
  if (bad == kBmRmNoMem) return fail(AMDR_ENOMEM, "bm25_remove: %s", bm_rm_error_text(bad));
  AMDR_REQUIRE(bad == kBmRmOk, "bm25_remove: %s", bm_rm_error_text(bad));
  AMDR_HIP(hipSetDevice(h->device));
  const int64_t V_old = h->n_terms, V_new = n_terms_new, nnz_old = h->nnz, n_old = h->n_docs, n_new = n_old - n_remove;
  const long long tiles = (nnz_old + kBmAddTile - 1) / kBmAddTile;
  AMDR_REQUIRE(tiles < (1ll << 31), "bm25_remove: %lld postings exceed the grid", (long long)nnz_old);
  // 0..5: the new arrays (one padding element each, as upload() leaves); the rest is freed when the call returns
  enum { TP, PD, PT, PW, IDF, DL, RID, DNEW, TRANK, TCNT, TBASE, RANKAT, DF, MAP, FLAG };
  BmAddBufs nb;
  int rc = nb.alloc(TP, (size_t)(V_new + 2) * sizeof(long long));
  if (!rc) rc = nb.alloc(IDF, (size_t)(V_new + 1) * sizeof(double));
  if (!rc) rc = nb.alloc(DL, (size_t)(n_new + 1) * sizeof(int));
  if (!rc) rc = nb.alloc(RID, (size_t)n_remove * sizeof(long long));
  if (!rc) rc = nb.alloc(DNEW, (size_t)n_old * sizeof(int));
  if (!rc) rc = nb.alloc(TRANK, (size_t)(nnz_old + 1) * sizeof(unsigned short));
  if (!rc) rc = nb.alloc(TCNT, (size_t)(tiles + 1) * sizeof(long long));
  if (!rc) rc = nb.alloc(TBASE, (size_t)(tiles + 1) * sizeof(long long));
  if (!rc) rc = nb.alloc(RANKAT, (size_t)(V_old + 1) * sizeof(long long));
  if (!rc) rc = nb.alloc(DF, (size_t)(V_new + 1) * sizeof(long long));
  if (!rc && term_map) rc = nb.alloc(MAP, (size_t)(V_old + 1) * sizeof(int));
  if (!rc) rc = nb.alloc(FLAG, sizeof(int));
  if (rc) return rc;
  hipStream_t st = h->stream;
  AMDR_HIP(hipMemcpyAsync(nb.p[RID], remove_ids, (size_t)n_remove * sizeof(long long), hipMemcpyHostToDevice, st));
  if (term_map && V_old) AMDR_HIP(hipMemcpyAsync(nb.p[MAP], term_map, (size_t)V_old * sizeof(int), hipMemcpyHostToDevice, st));
  if (V_new) AMDR_HIP(hipMemcpyAsync(nb.p[IDF], idf, (size_t)V_new * sizeof(double), hipMemcpyHostToDevice, st));
  AMDR_HIP(hipMemsetAsync(nb.p[FLAG], 0, sizeof(int), st));
  // the passes between events, in two stretches with the host's look at nnz_new between them
  // (amdr_bm25_remove_kernel_ms); an event that cannot be made only loses the time
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  struct EvGuard {
    hipEvent_t* e;
    ~EvGuard() {
      for (int i = 0; i < 4; ++i)
        if (e[i]) (void)hipEventDestroy(e[i]);
    }
  } ev_guard{ev};
  bool timed = true;
  for (int i = 0; i < 4 && timed; ++i)
    if (hipEventCreate(&ev[i]) != hipSuccess) {
      (void)hipGetLastError();
      ev[i] = nullptr;
      timed = false;
    }
  const int* map_dev = term_map ? (const int*)nb.p[MAP] : nullptr;
  if (timed) AMDR_HIP(hipEventRecord(ev[0], st));
  hipLaunchKernelGGL(bm25_rm_docmap_kernel, dim3((unsigned)((n_old + 255) / 256)), dim3(256), 0, st,
                     (const long long*)nb.p[RID], (long)n_remove, h->doc_len, (long)n_old, (int*)nb.p[DNEW], (int*)nb.p[DL]);
  AMDR_HIP(hipGetLastError());
  if (tiles > 0) {
    hipLaunchKernelGGL(bm25_rm_count_kernel, dim3((unsigned)tiles), dim3(kBmAddThreads), 0, st, h->post_doc,
                       (long long)nnz_old, (const int*)nb.p[DNEW], (unsigned short*)nb.p[TRANK], (long long*)nb.p[TCNT]);
    AMDR_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(compact_scan_i64_kernel, dim3(1), dim3(kCompactScanThreads), 0, st, (const long long*)nb.p[TCNT],
                     (long)tiles, (long long*)nb.p[TBASE]);
  AMDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(bm25_rm_terms_kernel, dim3((unsigned)((V_old + 1 + 255) / 256)), dim3(256), 0, st, h->term_ptr,
                     (long)V_old, (long long)nnz_old, (const long long*)nb.p[TBASE], (const unsigned short*)nb.p[TRANK],
                     map_dev, (long long*)nb.p[RANKAT], (long long*)nb.p[DF], (int*)nb.p[FLAG]);
  AMDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(compact_scan_i64_kernel, dim3(1), dim3(kCompactScanThreads), 0, st, (const long long*)nb.p[DF],
                     (long)V_new, (long long*)nb.p[TP]);
  AMDR_HIP(hipGetLastError());
  if (timed) AMDR_HIP(hipEventRecord(ev[1], st));
  long long nnz_new = 0;
  int flag = 0;
  AMDR_HIP(hipMemcpyAsync(&nnz_new, (const long long*)nb.p[TBASE] + tiles, sizeof(long long), hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipMemcpyAsync(&flag, nb.p[FLAG], sizeof(int), hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipStreamSynchronize(st));
  AMDR_REQUIRE(flag == 0, "bm25_remove: a term mapped to -1 still has a surviving posting");
  if (nnz_new < 0 || nnz_new > nnz_old) return fail(AMDR_EHIP, "bm25_remove: counted %lld of %lld postings", nnz_new, (long long)nnz_old);
  rc = nb.alloc(PD, (size_t)(nnz_new + 1) * sizeof(int));
  if (!rc) rc = nb.alloc(PT, (size_t)(nnz_new + 1) * sizeof(int));
  if (!rc) rc = nb.alloc(PW, (size_t)(nnz_new + 1) * sizeof(double));
  if (rc) return rc;
  if (timed) AMDR_HIP(hipEventRecord(ev[2], st));
  if (tiles > 0 && nnz_new > 0) {
    hipLaunchKernelGGL(bm25_rm_scatter_kernel, dim3((unsigned)tiles), dim3(kBmAddThreads), 0, st, h->term_ptr, (long)V_old,
                       h->post_doc, h->post_tf, (long long)nnz_old, (const int*)nb.p[DNEW], (const int*)nb.p[DL],
                       (const long long*)nb.p[TBASE], (const unsigned short*)nb.p[TRANK], (const long long*)nb.p[RANKAT],
                       (const long long*)nb.p[TP], map_dev, nnz_new, avgdl, h->k1, h->b, (int*)nb.p[PD], (int*)nb.p[PT],
                       (double*)nb.p[PW]);
    AMDR_HIP(hipGetLastError());
  }
  if (timed) AMDR_HIP(hipEventRecord(ev[3], st));
  AMDR_HIP(hipStreamSynchronize(st));
  float ms0 = -1.f, ms1 = -1.f;
  if (!(timed && hipEventElapsedTime(&ms0, ev[0], ev[1]) == hipSuccess && hipEventElapsedTime(&ms1, ev[2], ev[3]) == hipSuccess)) {
    (void)hipGetLastError();
    ms0 = -1.f;
    ms1 = 0.f;
  }
  h->remove_kernel_ms = (double)ms0 + (double)ms1;
  // the swap: from here on nothing can fail (the old arrays take the new ones' places in nb and are freed with it)
  auto swap_in = [&](auto*& held, int i) {
    void* old = (void*)held;
    held = reinterpret_cast<std::remove_reference_t<decltype(held)>>(nb.p[i]);
    nb.p[i] = old;
  };
  swap_in(h->term_ptr, TP);
  swap_in(h->post_doc, PD);
  swap_in(h->post_tf, PT);
  swap_in(h->post_w, PW);
  swap_in(h->idf, IDF);
  swap_in(h->doc_len, DL);
  h->n_terms = V_new;
  h->n_docs = n_new;
  h->nnz = nnz_new;
  h->avgdl = avgdl;
  ++h->removes;
  return AMDR_OK;
}

int amdr_bm25_remove_kernel_ms(amdr_bm25_t* h, double* ms) {
  AMDR_REQUIRE(h && ms, "bm25_remove_kernel_ms: null");
  std::lock_guard<std::mutex> g(h->mu);
  *ms = h->remove_kernel_ms;
  return AMDR_OK;
}

int amdr_bm25_info(amdr_bm25_t* h, int64_t* out6) {
  AMDR_REQUIRE(h && out6, "bm25_info: null");
  std::lock_guard<std::mutex> g(h->mu);
  out6[0] = h->n_docs;
  out6[1] = h->n_terms;
  out6[2] = h->nnz;
  out6[3] = h->adds;
  out6[4] = kBmAddTile;
  out6[5] = h->removes;
  return AMDR_OK;
}

int amdr_bm25_add_kernel_ms(amdr_bm25_t* h, double* ms) {
  AMDR_REQUIRE(h && ms, "bm25_add_kernel_ms: null");
  std::lock_guard<std::mutex> g(h->mu);
  *ms = h->add_kernel_ms;
  return AMDR_OK;
}

int amdr_bm25_read(amdr_bm25_t* h, int64_t* term_ptr, int32_t* post_doc, int32_t* post_tf, double* post_w, double* idf,
                   int32_t* doc_len) {
  AMDR_REQUIRE(h != nullptr, "bm25_read: null handle");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  const size_t V = (size_t)h->n_terms, nnz = (size_t)h->nnz, n = (size_t)h->n_docs;
  if (term_ptr) AMDR_HIP(hipMemcpy(term_ptr, h->term_ptr, (V + 1) * sizeof(long long), hipMemcpyDeviceToHost));
  if (post_doc && nnz) AMDR_HIP(hipMemcpy(post_doc, h->post_doc, nnz * sizeof(int), hipMemcpyDeviceToHost));
  if (post_tf && nnz) AMDR_HIP(hipMemcpy(post_tf, h->post_tf, nnz * sizeof(int), hipMemcpyDeviceToHost));
  if (post_w && nnz) AMDR_HIP(hipMemcpy(post_w, h->post_w, nnz * sizeof(double), hipMemcpyDeviceToHost));
  if (idf && V) AMDR_HIP(hipMemcpy(idf, h->idf, V * sizeof(double), hipMemcpyDeviceToHost));
  if (doc_len && n) AMDR_HIP(hipMemcpy(doc_len, h->doc_len, n * sizeof(int), hipMemcpyDeviceToHost));
  return AMDR_OK;
}

int amdr_bm25_destroy(amdr_bm25_t* h) {
  if (!h) return AMDR_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamDestroy(h->stream);
  }
  if (h->term_ptr) (void)hipFree(h->term_ptr);
  if (h->post_doc) (void)hipFree(h->post_doc);
  if (h->post_w) (void)hipFree(h->post_w);
  if (h->idf) (void)hipFree(h->idf);
  if (h->post_tf) (void)hipFree(h->post_tf);
  if (h->doc_len) (void)hipFree(h->doc_len);
  h->part[0].release();
  h->part[1].release();
  h->qterms.release();
  h->qptr.release();
  h->sbuf.release();
  h->ibuf.release();
  h->full.release();
  h->ticket.release();
  delete h;
  return AMDR_OK;
}

}  // extern "C"

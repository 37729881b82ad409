// BM25 channel: updates of the resident index (bm25_handle.hpp) — amdr_bm25_add, amdr_bm25_remove, amdr_bm25_replace — and
// what reads it back (amdr_bm25_info, amdr_bm25_read), and the token stream's own entry points (amdr_bm25_set_tokens,
// amdr_bm25_tokens_info, amdr_bm25_read_tokens: host-side copies and validation).  After any sequence of updates the
// handle is what amdr_bm25_create (bm25.hip) makes of the resulting index, byte for byte: built with -ffp-contract=off, as
// bm25.hip is, so that bm25_factor gives the bits of create's host loop.
//
// Every update builds a second BmIndex beside the live one and commits it by one swap after the stream has finished: a
// failed update leaves the handle as it was.  All divide the work by tiles of kBmTile postings, not by terms (a Zipfian
// head term holds every document and a wave per term would serialise on it); a block finds the terms of its tile with
// bm_tile_window.  No atomics anywhere: the result is deterministic.
//
// amdr_bm25_add appends documents.  N and avgdl are corpus-global, so every factor changes: the add is ONE pass over the
// resident postings (bm25_merge_kernel) that interleaves each term's old list with the added documents' list behind it
// and recomputes post_w with the new avgdl, next to the data.  post_tf and doc_len stay resident for that (16 B per
// posting instead of 12, + 4 B per document).
//
// amdr_bm25_remove takes documents out.  It is a stream compaction of the postings in two passes over them, divided by
// tiles of kBmTile OLD postings (compact.hpp, bm25_remove_rule.hpp):
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
//
// amdr_bm25_replace exchanges documents under their ids: the remove's document map, counting pass and scans, then two
// scatters that MERGE, per new term, the surviving old postings with the new documents' postings by document id
// (bm25_replace_rule.hpp) — one pass over the postings fewer than a remove followed by an add, and no id moves:
//   bm25_rp_docmap_kernel       doc_keep[d] = d or -1 (replaced); doc_len[d] = the old or the new length
//   bm25_rm_count_kernel        as in the remove, over doc_keep
//   bm25_rp_terms_kernel        rank_at per old term, the flag, and df_new[u] = survivors of the old term of u + add count
//   bm25_rp_scatter_old_kernel  per tile of old postings: a kept posting goes behind the kept ones before it and the add
//                               postings of its new list with a smaller document (one search in that list, mostly empty)
//   bm25_rp_scatter_add_kernel  per tile of the add's postings: behind the add postings before it and the kept old
//                               postings with a smaller document (one search in the old list + the tile rank tables)
//
// The carrying forms (amdr_bm25_add_carry, _remove_carry, _replace_carry) are the same three bodies with the carry of the
// resident token stream (bm25_handle.hpp: tok_ptr, tok) switched on: a second stream is built beside the live one and
// committed with the index, in the same place, after the stream has finished (tok_carry_rule.hpp):
//   bm25_rm_docmap_kernel       (remove) also writes kept_old[doc_new[d]] = d, the inverse of the document map
//   tok_len_i64_kernel          the new doc_len widened to 8 B, for
//   compact_scan_i64_kernel     the new tok_ptr = the exclusive scan of the new lengths (the last one is the token count)
//   tok_carry_kernel            per tile of kBmTile NEW tokens: the documents of the tile found in the new tok_ptr
//                               (bm_tile_window), each token read from the old stream or the add's and rewritten through
//                               the term map                       reads 4 B + a 4 B gather of the map, writes 4 B
// The plain forms drop the stream, as before.
#include "common.hpp"

#include <memory>
#include <mutex>
#include <new>

#include "bm25_add_rule.hpp"
#include "bm25_core.hpp"
#include "bm25_handle.hpp"
#include "bm25_remove_rule.hpp"
#include "bm25_replace_rule.hpp"
#include "compact.hpp"
#include "tok_carry_rule.hpp"

using namespace amdr;

namespace {

// ---- the tile walk of the update kernels -----------------------------------------------------------------------------
// Thread tid of a block owns postings p0 + u * kBmTileThreads + tid of its tile, u = 0 .. kBmTilePerThread - 1.  (That loop
// stays written out in the three kernels: with its body passed as a functor they compile to other code, 29 for 35 VGPRs
// in the merge kernel.)
// Where the postings of a tile find their terms: tab[t - base] is the table entry of term t, for t in [t0, t1 + 1].
struct BmTileWindow {
  const long long* tab;
  long base, t0, t1;
  __device__ long term_of(long long p) const { return bm_tile_term_of(tab, base, t0, t1, p); }
  __device__ long long start_of(long t) const { return tab[t - base]; }
};

// The terms of tile [p0, p1) (not empty) in the table `ptr` of n_terms terms; every thread of the block calls this.
// Thread 0 finds the terms of the tile's first and last posting by binary search in the table; the entries between them
// go to `win` (LDS, kBmTile + 2 entries: a tile holds at most kBmTile terms that have postings).  A window widened by
// terms WITHOUT postings beyond that room is searched in global memory instead.
__device__ __forceinline__ BmTileWindow bm_tile_window(const long long* __restrict__ ptr, long n_terms, long long p0,
                                                       long long p1, long long* win) {
  __shared__ long t_first, t_last;
  const int tid = threadIdx.x;
  if (tid == 0) {
    long a, z;
    bm_tile_terms(ptr, n_terms, p0, p1, &a, &z);
    t_first = a;
    t_last = z;
  }
  __syncthreads();
  const long t0 = t_first, t1 = t_last;
  const bool in_lds = bm_tile_window_fits(t0, t1);
  if (in_lds) {
    for (long i = tid; i <= t1 - t0 + 1; i += kBmTileThreads) win[i] = ptr[t0 + i];
    __syncthreads();
  }
  return {in_lds ? win : ptr, in_lds ? t0 : 0, t0, t1};
}

// ---- amdr_bm25_add: term table and merge ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bm25_term_ptr_sum_kernel(const long long* __restrict__ old_ptr, long n_terms_old,
                                                                const long long* __restrict__ add_ptr, long n_terms_new,
                                                                long long* __restrict__ new_ptr) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t <= n_terms_new) new_ptr[t] = bm_add_term_ptr(old_ptr, n_terms_old, add_ptr, t);
}

// One block = kBmTile consecutive OUTPUT postings, their terms found in the NEW term table.  A posting reads 8 B (doc, tf)
// from the old list or the add's, gathers 4 B of doc_len, and writes 16 B (doc, tf, factor).
__global__ __launch_bounds__(kBmTileThreads) void bm25_merge_kernel(
    const long long* __restrict__ new_ptr, long n_terms_new, const long long* __restrict__ old_ptr, long n_terms_old,
    const int* __restrict__ old_doc, const int* __restrict__ old_tf, const long long* __restrict__ add_ptr,
    const int* __restrict__ add_doc, const int* __restrict__ add_tf, const int* __restrict__ doc_len /* new */,
    int n_docs_old, long long nnz_new, double avgdl, double k1, double b, int* __restrict__ out_doc,
    int* __restrict__ out_tf, double* __restrict__ out_w) {
  __shared__ long long win[kBmTile + 2];
  const long long p0 = (long long)blockIdx.x * kBmTile;
  long long p1 = p0 + kBmTile;  // exclusive
  if (p1 > nnz_new) p1 = nnz_new;
  if (p0 >= p1) return;
  const BmTileWindow w = bm_tile_window(new_ptr, n_terms_new, p0, p1, win);
  const int tid = threadIdx.x;
#pragma unroll
  for (int u = 0; u < kBmTilePerThread; ++u) {
    const long long p = p0 + (long long)u * kBmTileThreads + tid;
    if (p < p1) {
      const long t = w.term_of(p);
      bool from_add;
      const long long src = bm_add_source(p, w.start_of(t), t, old_ptr, n_terms_old, add_ptr, &from_add);
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
                                                             int* __restrict__ doc_new, int* __restrict__ doc_len_new,
                                                             int* __restrict__ kept_old /* or null */) {
  const long d = (long)blockIdx.x * 256 + threadIdx.x;
  if (d >= n_docs_old) return;
  const int nd = bm_rm_doc_new(remove_ids, n_remove, d);
  doc_new[d] = nd;
  if (nd >= 0) {
    doc_len_new[nd] = doc_len_old[d];
    if (kept_old) kept_old[nd] = (int)d;  // the inverse map of the carry: one writer per slot
  }
}

// One block = one tile of kBmTile consecutive OLD postings: which of them survive, each one's rank among the tile's
// survivors (compact_tile_scan) and the tile's count.
__global__ __launch_bounds__(kBmTileThreads) void bm25_rm_count_kernel(const int* __restrict__ old_doc, long long nnz_old,
                                                                       const int* __restrict__ doc_new,
                                                                       unsigned short* __restrict__ tile_rank,
                                                                       long long* __restrict__ tile_cnt) {
  __shared__ int lds[kBmTile + kBmTileThreads / 64 + 1];
  const long long p0 = (long long)blockIdx.x * kBmTile;
  const int tid = threadIdx.x;
  unsigned keep = 0;
#pragma unroll
  for (int u = 0; u < kBmTilePerThread; ++u) {
    const long long p = p0 + (long long)u * kBmTileThreads + tid;
    if (p < nnz_old && doc_new[old_doc[p]] >= 0) keep |= 1u << u;
  }
  int rank[kBmTilePerThread];
  const int total = compact_tile_scan<kBmTileThreads, kBmTilePerThread>(keep, lds, rank);
#pragma unroll
  for (int u = 0; u < kBmTilePerThread; ++u) {
    const long long p = p0 + (long long)u * kBmTileThreads + tid;
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

// One block = one tile of OLD postings again, their terms found in the OLD term table.  A surviving posting reads 8 B
// (doc, tf) + 2 B of rank, gathers doc_new and doc_len (4 B each) and the few table entries of its term, and writes 16 B
// (doc, tf, factor) at bm_rm_dest.  Every destination is a sum of counts.
__global__ __launch_bounds__(kBmTileThreads) void bm25_rm_scatter_kernel(
    const long long* __restrict__ old_ptr, long n_terms_old, const int* __restrict__ old_doc, const int* __restrict__ old_tf,
    long long nnz_old, const int* __restrict__ doc_new, const int* __restrict__ doc_len /* new */,
    const long long* __restrict__ tile_base, const unsigned short* __restrict__ tile_rank,
    const long long* __restrict__ rank_at, const long long* __restrict__ new_ptr, const int* __restrict__ term_map,
    long long nnz_new, double avgdl, double k1, double b, int* __restrict__ out_doc, int* __restrict__ out_tf,
    double* __restrict__ out_w) {
  __shared__ long long win[kBmTile + 2];
  const long long p0 = (long long)blockIdx.x * kBmTile;
  long long p1 = p0 + kBmTile;  // exclusive
  if (p1 > nnz_old) p1 = nnz_old;
  if (p0 >= p1) return;
  const BmTileWindow w = bm_tile_window(old_ptr, n_terms_old, p0, p1, win);
  const int tid = threadIdx.x;
#pragma unroll
  for (int u = 0; u < kBmTilePerThread; ++u) {
    const long long p = p0 + (long long)u * kBmTileThreads + tid;
    if (p < p1) {
      const int doc = doc_new[old_doc[p]];
      if (doc >= 0) {
        const long long dst = bm_rm_dest(p, w.term_of(p), nnz_old, tile_base, tile_rank, rank_at, new_ptr, term_map);
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

// ---- amdr_bm25_replace: document map, the remove's tile ranks, term table, two scatters ---------------------------------
__global__ __launch_bounds__(256) void bm25_rp_docmap_kernel(const long long* __restrict__ replace_ids, long n_rep,
                                                             const int* __restrict__ doc_len_old,
                                                             const int* __restrict__ doc_len_add, long n_docs,
                                                             int* __restrict__ doc_keep, int* __restrict__ doc_len_new) {
  const long d = (long)blockIdx.x * 256 + threadIdx.x;
  if (d < n_docs) bm_rp_doc_entry(replace_ids, n_rep, doc_len_old, doc_len_add, d, doc_keep, doc_len_new);
}

__global__ __launch_bounds__(256) void bm25_rp_terms_kernel(const long long* __restrict__ old_ptr, long n_terms_old,
                                                            long n_terms_new, long long nnz_old,
                                                            const long long* __restrict__ tile_base,
                                                            const unsigned short* __restrict__ tile_rank,
                                                            const int* __restrict__ term_map, const int* __restrict__ inv,
                                                            const long long* __restrict__ add_ptr,
                                                            long long* __restrict__ rank_at, long long* __restrict__ df_new,
                                                            int* __restrict__ bad) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  bm_rp_term_entry(e, n_terms_old, n_terms_new, old_ptr, nnz_old, tile_base, tile_rank, term_map, inv, add_ptr, rank_at,
                   df_new, bad);
}

// One block = one tile of OLD postings, their terms found in the OLD term table: bm25_rm_scatter_kernel with the add
// postings of the term's new list counted in (one binary search in that list, skipped where it is empty).  A surviving
// posting reads 8 B (doc, tf) + 2 B of rank, gathers doc_keep and doc_len, and writes 16 B at bm_rp_dest_old.
__global__ __launch_bounds__(kBmTileThreads) void bm25_rp_scatter_old_kernel(
    const long long* __restrict__ old_ptr, long n_terms_old, const int* __restrict__ old_doc, const int* __restrict__ old_tf,
    long long nnz_old, const int* __restrict__ doc_keep, const int* __restrict__ doc_len /* new */,
    const long long* __restrict__ tile_base, const unsigned short* __restrict__ tile_rank,
    const long long* __restrict__ rank_at, const long long* __restrict__ new_ptr, const int* __restrict__ term_map,
    const long long* __restrict__ add_ptr, const int* __restrict__ add_doc, const long long* __restrict__ replace_ids,
    long long nnz_new, double avgdl, double k1, double b, int* __restrict__ out_doc, int* __restrict__ out_tf,
    double* __restrict__ out_w) {
  __shared__ long long win[kBmTile + 2];
  const long long p0 = (long long)blockIdx.x * kBmTile;
  long long p1 = p0 + kBmTile;  // exclusive
  if (p1 > nnz_old) p1 = nnz_old;
  if (p0 >= p1) return;
  const BmTileWindow w = bm_tile_window(old_ptr, n_terms_old, p0, p1, win);
  const int tid = threadIdx.x;
#pragma unroll
  for (int u = 0; u < kBmTilePerThread; ++u) {
    const long long p = p0 + (long long)u * kBmTileThreads + tid;
    if (p < p1) {
      const int doc = doc_keep[old_doc[p]];
      if (doc >= 0) {
        const long long dst = bm_rp_dest_old(p, doc, w.term_of(p), nnz_old, tile_base, tile_rank, rank_at, new_ptr, term_map,
                                             add_ptr, add_doc, replace_ids);
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

// One block = one tile of the ADD's postings, their terms found in the add's own term table (over the new ids).  A posting
// reads 8 B (local doc, tf) and its document id, searches its term's OLD list for that document (bm_rp_dest_add) and
// writes 16 B.
__global__ __launch_bounds__(kBmTileThreads) void bm25_rp_scatter_add_kernel(
    const long long* __restrict__ add_ptr, long n_terms_new, const int* __restrict__ add_doc, const int* __restrict__ add_tf,
    long long nnz_add, const long long* __restrict__ replace_ids, const int* __restrict__ inv,
    const long long* __restrict__ old_ptr, const int* __restrict__ old_doc, long long nnz_old,
    const long long* __restrict__ tile_base, const unsigned short* __restrict__ tile_rank,
    const long long* __restrict__ rank_at, const long long* __restrict__ new_ptr, const int* __restrict__ doc_len /* new */,
    long long nnz_new, double avgdl, double k1, double b, int* __restrict__ out_doc, int* __restrict__ out_tf,
    double* __restrict__ out_w) {
  __shared__ long long win[kBmTile + 2];
  const long long p0 = (long long)blockIdx.x * kBmTile;
  long long p1 = p0 + kBmTile;  // exclusive
  if (p1 > nnz_add) p1 = nnz_add;
  if (p0 >= p1) return;
  const BmTileWindow w = bm_tile_window(add_ptr, n_terms_new, p0, p1, win);
  const int tid = threadIdx.x;
#pragma unroll
  for (int u = 0; u < kBmTilePerThread; ++u) {
    const long long q = p0 + (long long)u * kBmTileThreads + tid;
    if (q < p1) {
      const long long doc = replace_ids[add_doc[q]];
      const long long dst = bm_rp_dest_add(q, doc, w.term_of(q), inv, old_ptr, old_doc, nnz_old, tile_base, tile_rank, rank_at,
                                           new_ptr, add_ptr);
      if (dst >= 0 && dst < nnz_new) {  // (always, after the host's checks)
        const int tf = add_tf[q];
        out_doc[dst] = (int)doc;
        out_tf[dst] = tf;
        out_w[dst] = bm25_factor(tf, doc_len[doc], avgdl, k1, b);
      }
    }
  }
}

// ---- the carry of the token stream: new tok_ptr, one pass over the new tokens ---------------------------------------------
__global__ __launch_bounds__(256) void tok_len_i64_kernel(const int* __restrict__ doc_len, long n_docs,
                                                          long long* __restrict__ len64) {
  const long d = (long)blockIdx.x * 256 + threadIdx.x;
  if (d < n_docs) len64[d] = (long long)doc_len[d];
}

// One block = kBmTile consecutive NEW tokens, their documents found in the NEW tok_ptr (a document is to the stream what a
// term is to the postings; a run of empty documents wider than the LDS window is searched in the table itself).  A token
// reads 4 B from the old stream or the add's, gathers 4 B of the term map and writes 4 B (tc_token_at: every index is
// compared with its array's count, a miss raises *bad instead of reading).
__global__ __launch_bounds__(kBmTileThreads) void tok_carry_kernel(const TcArgs a, const long long* __restrict__ new_ptr,
                                                                   long long n_tok_new, int* __restrict__ out,
                                                                   int* __restrict__ bad) {
  __shared__ long long win[kBmTile + 2];
  const long long p0 = (long long)blockIdx.x * kBmTile;
  long long p1 = p0 + kBmTile;  // exclusive
  if (p1 > n_tok_new) p1 = n_tok_new;
  if (p0 >= p1) return;
  const BmTileWindow w = bm_tile_window(new_ptr, a.n_docs_new, p0, p1, win);
  const int tid = threadIdx.x;
#pragma unroll
  for (int u = 0; u < kBmTilePerThread; ++u) {
    const long long q = p0 + (long long)u * kBmTileThreads + tid;
    if (q < p1) {
      const long d = w.term_of(q);
      const int t = tc_token_at(a, d, q - w.start_of(d), bad);
      if (t >= 0) out[q] = t;
    }
  }
}

// The carry of one update: the staged stream, its scratch and its timer (amdr_bm25_carry_kernel_ms).  With `on` false every
// step is skipped and the update ends in drop_tokens(), as the plain calls always have.
struct TokCarry {
  bool on;
  BmStagedTokens nx;
  CallScratch tmp;
  KernelSpans timer;
  long long *len64 = nullptr, *add_ptr = nullptr;
  int *add_tok = nullptr, *kept_old = nullptr, *flag_dev = nullptr;
  long long n_tok_new = -1;  // the device's count: new tok_ptr[n_docs_new], valid after the synchronisation behind scan()
  int flag = 0;              // the kernel's error flag, valid after the synchronisation behind run()
  explicit TokCarry(bool on_) : on(on_), timer(on_ ? 2 : 0) {}

  // the tables of n_new documents; kept_old for a remove (the document-map pass fills it)
  int begin(int64_t n_new, bool want_kept, const char* who) {
    if (!on) return AMDR_OK;
    AMDR_TRY(dev_alloc(&nx.tok_ptr, (size_t)n_new + 2, who));
    AMDR_TRY(tmp.alloc(&len64, (size_t)n_new + 1, who));
    if (want_kept) AMDR_TRY(tmp.alloc(&kept_old, (size_t)n_new + 1, who));
    AMDR_TRY(tmp.alloc(&flag_dev, 1, who));
    return AMDR_OK;
  }
  // the new tok_ptr from the new lengths (on the device, behind the pass that wrote them)
  int scan(const int* doc_len_new, int64_t n_new, hipStream_t st) {
    if (!on) return AMDR_OK;
    AMDR_TRY(timer.begin(0, st));
    hipLaunchKernelGGL(tok_len_i64_kernel, dim3((unsigned)((n_new + 255) / 256)), dim3(256), 0, st, doc_len_new, (long)n_new,
                       len64);
    AMDR_HIP(hipGetLastError());
    hipLaunchKernelGGL(compact_scan_i64_kernel, dim3(1), dim3(kCompactScanThreads), 0, st, len64, (long)n_new, nx.tok_ptr);
    AMDR_HIP(hipGetLastError());
    AMDR_TRY(timer.end(0, st));
    AMDR_HIP(hipMemcpyAsync(&n_tok_new, nx.tok_ptr + n_new, sizeof(long long), hipMemcpyDeviceToHost, st));
    return AMDR_OK;
  }
  // the new tokens: n_tok of them (the host's count in an add, the device's after a remove or a replace).  `a` comes
  // without the add's device arrays: they are uploaded here from tok_ptr_add[a.n_add + 1] / tok_add.
  int run(TcArgs a, int64_t n_tok, const int64_t* tok_ptr_add, const int32_t* tok_add, hipStream_t st, const char* who) {
    if (!on) return AMDR_OK;
    const long long tiles = (n_tok + kBmTile - 1) / kBmTile;
    if (n_tok < 0 || tiles >= (1ll << 31)) return fail(AMDR_EINVAL, "%s: %lld tokens exceed the carry grid", who, (long long)n_tok);
    nx.n_tokens = n_tok;
    AMDR_TRY(dev_alloc(&nx.tok, (size_t)n_tok + 1, who));  // (+ 1: never an empty allocation)
    a.n_tok_add = a.n_add ? (long long)tok_ptr_add[a.n_add] : 0;
    AMDR_TRY(tmp.alloc(&add_ptr, (size_t)a.n_add + 1, who));
    AMDR_TRY(tmp.alloc(&add_tok, (size_t)a.n_tok_add + 1, who));
    if (a.n_add) AMDR_HIP(hipMemcpyAsync(add_ptr, tok_ptr_add, (size_t)(a.n_add + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    if (a.n_tok_add) AMDR_HIP(hipMemcpyAsync(add_tok, tok_add, (size_t)a.n_tok_add * sizeof(int), hipMemcpyHostToDevice, st));
    a.add_ptr = add_ptr, a.add_tok = add_tok;
    AMDR_HIP(hipMemsetAsync(flag_dev, 0, sizeof(int), st));
    AMDR_TRY(timer.begin(1, st));
    if (tiles > 0) {
      hipLaunchKernelGGL(tok_carry_kernel, dim3((unsigned)tiles), dim3(kBmTileThreads), 0, st, a, nx.tok_ptr, (long long)n_tok,
                         nx.tok, flag_dev);
      AMDR_HIP(hipGetLastError());
    }
    AMDR_TRY(timer.end(1, st));
    AMDR_HIP(hipMemcpyAsync(&flag, flag_dev, sizeof(int), hipMemcpyDeviceToHost, st));
    return AMDR_OK;
  }
  // after the last synchronisation and the flag check: the stream changes places with the index, or goes as it always did
  void commit(amdr_bm25* h) {
    if (on) {
      h->carry_kernel_ms = timer.ms();
      nx.commit(*h);
    } else {
      h->drop_tokens();  // the stream described the index as it was (amdr_bm25_set_tokens)
    }
  }
};

// The old stream's part of a carry's arguments.
TcArgs tc_args(int mode, const amdr_bm25* h, int64_t n_docs_new, int64_t n_add, int64_t n_terms_new) {
  TcArgs a = {};
  a.mode = mode;
  a.n_docs_new = (long)n_docs_new, a.n_docs_old = (long)h->ix.n_docs, a.n_add = (long)n_add;
  a.old_ptr = h->tok_ptr, a.old_tok = h->tok, a.n_tok_old = h->n_tokens;
  a.n_terms_old = (long)h->ix.n_terms, a.n_terms_new = (long)n_terms_new;
  return a;
}

// ---- the three updates: each plain call is the carrying body with the carry off ------------------------------------------
int bm25_add_body(amdr_bm25_t* h, const int64_t* term_ptr_add, const int32_t* post_doc_add, const int32_t* post_tf_add,
                  const double* idf, const int32_t* doc_len_add, int64_t n_terms, int64_t n_add, double avgdl,
                  bool carry, const int64_t* tok_ptr_add, const int32_t* tok_add) {
  static const char* const who = "bm25_add";
  AMDR_REQUIRE(h != nullptr, "bm25_add: null handle");
  AMDR_REQUIRE(n_add >= 0, "bm25_add: n_add=%lld", (long long)n_add);
  if (n_add == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  const BmIndex& old = h->ix;
  const int bad = bm_add_validate(term_ptr_add, post_doc_add, post_tf_add, idf, doc_len_add, n_terms, n_add, avgdl,
                                  old.n_terms, old.n_docs);
  AMDR_REQUIRE(bad == kBmAddOk, "bm25_add: %s", bm_add_error_text(bad));
  if (carry) {
    const int tbad = tc_validate_add(tok_ptr_add, tok_add, doc_len_add, n_add, n_terms);
    AMDR_REQUIRE(tbad == kPhValid, "bm25_add_carry: the added token stream: %s", ph_error_text(tbad));
  }
  TokCarry tc(carry && h->has_tokens);  // without a resident stream the call is the plain call
  AMDR_HIP(hipSetDevice(h->device));
  const int64_t nnz_add = term_ptr_add[n_terms], nnz_new = old.nnz + nnz_add;
  BmStagedIndex nx;
  AMDR_TRY(nx.alloc_tables(n_terms, old.n_docs + n_add, avgdl, who));
  AMDR_TRY(nx.alloc_postings(nnz_new, who));
  AMDR_TRY(tc.begin(old.n_docs + n_add, false, who));
  // the add's own CSR on the device (never an empty allocation)
  CallScratch tmp;
  long long* add_ptr;
  int *add_doc, *add_tf;
  AMDR_TRY(tmp.alloc(&add_ptr, (size_t)n_terms + 1, who));
  AMDR_TRY(tmp.alloc(&add_doc, (size_t)nnz_add + 1, who));
  AMDR_TRY(tmp.alloc(&add_tf, (size_t)nnz_add + 1, who));
  hipStream_t st = h->stream;
  AMDR_HIP(hipMemcpyAsync(add_ptr, term_ptr_add, (size_t)(n_terms + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
  if (nnz_add) {
    AMDR_HIP(hipMemcpyAsync(add_doc, post_doc_add, (size_t)nnz_add * sizeof(int), hipMemcpyHostToDevice, st));
    AMDR_HIP(hipMemcpyAsync(add_tf, post_tf_add, (size_t)nnz_add * sizeof(int), hipMemcpyHostToDevice, st));
  }
  if (n_terms) AMDR_HIP(hipMemcpyAsync(nx.idf, idf, (size_t)n_terms * sizeof(double), hipMemcpyHostToDevice, st));
  AMDR_HIP(hipMemcpyAsync(nx.doc_len, old.doc_len, (size_t)old.n_docs * sizeof(int), hipMemcpyDeviceToDevice, st));
  AMDR_HIP(hipMemcpyAsync(nx.doc_len + old.n_docs, doc_len_add, (size_t)n_add * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(bm25_term_ptr_sum_kernel, dim3((unsigned)((n_terms + 1 + 255) / 256)), dim3(256), 0, st, old.term_ptr,
                     (long)old.n_terms, add_ptr, (long)n_terms, nx.term_ptr);
  AMDR_HIP(hipGetLastError());
  KernelSpans timer(1);  // the merge kernel (amdr_bm25_add_kernel_ms)
  if (nnz_new > 0) {
    const long long blocks = (nnz_new + kBmTile - 1) / kBmTile;
    AMDR_REQUIRE(blocks < (1ll << 31), "bm25_add: %lld postings exceed the merge grid", (long long)nnz_new);
    AMDR_TRY(timer.begin(0, st));
    hipLaunchKernelGGL(bm25_merge_kernel, dim3((unsigned)blocks), dim3(kBmTileThreads), 0, st, nx.term_ptr, (long)n_terms,
                       old.term_ptr, (long)old.n_terms, old.post_doc, old.post_tf, add_ptr, add_doc, add_tf, nx.doc_len,
                       (int)old.n_docs, (long long)nnz_new, avgdl, h->k1, h->b, nx.post_doc, nx.post_tf, nx.post_w);
    AMDR_HIP(hipGetLastError());
    AMDR_TRY(timer.end(0, st));
  }
  // the stream: the old one with the added documents behind it (the host knows the new token count)
  const int64_t n_tok_new = tc.on ? h->n_tokens + tok_ptr_add[n_add] : 0;
  AMDR_TRY(tc.scan(nx.doc_len, old.n_docs + n_add, st));
  AMDR_TRY(tc.run(tc_args(kTcAdd, h, old.n_docs + n_add, n_add, n_terms), n_tok_new, tok_ptr_add, tok_add, st, who));
  AMDR_HIP(hipStreamSynchronize(st));
  if (tc.on && tc.n_tok_new != n_tok_new)
    return fail(AMDR_EHIP, "bm25_add_carry: the new lengths sum to %lld tokens, not %lld", tc.n_tok_new, (long long)n_tok_new);
  AMDR_REQUIRE(tc.flag == 0, "bm25_add_carry: a token or a gather index of the carry is outside its array");
  h->add_kernel_ms = timer.ms();
  nx.commit(h->ix, h->adds);  // from here on nothing can fail
  tc.commit(h);
  return AMDR_OK;
}

int bm25_remove_body(amdr_bm25_t* h, const int64_t* remove_ids, int64_t n_remove, const int32_t* term_map,
                     int64_t n_terms_new, const double* idf, double avgdl, bool carry) {
  static const char* const who = "bm25_remove";
  AMDR_REQUIRE(h != nullptr, "bm25_remove: null handle");
  AMDR_REQUIRE(n_remove >= 0, "bm25_remove: n_remove=%lld", (long long)n_remove);
  if (n_remove == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  const BmIndex& old = h->ix;
  const int bad = bm_rm_validate(remove_ids, n_remove, term_map, n_terms_new, idf, avgdl, old.n_terms, old.n_docs);
  if (bad == kBmRmNoMem) return fail(AMDR_ENOMEM, "bm25_remove: %s", bm_rm_error_text(bad));
  AMDR_REQUIRE(bad == kBmRmOk, "bm25_remove: %s", bm_rm_error_text(bad));
  TokCarry tc(carry && h->has_tokens);  // without a resident stream the call is the plain call
  AMDR_HIP(hipSetDevice(h->device));
  const int64_t V_old = old.n_terms, V_new = n_terms_new, nnz_old = old.nnz, n_old = old.n_docs;
  const long long tiles = (nnz_old + kBmTile - 1) / kBmTile;
  AMDR_REQUIRE(tiles < (1ll << 31), "bm25_remove: %lld postings exceed the grid", (long long)nnz_old);
  BmStagedIndex nx;
  AMDR_TRY(nx.alloc_tables(V_new, n_old - n_remove, avgdl, who));
  AMDR_TRY(tc.begin(n_old - n_remove, true, who));
  CallScratch tmp;
  long long *rm_ids, *tile_cnt, *tile_base, *rank_at, *df_new;
  int *doc_new, *map_dev = nullptr, *flag_dev;
  unsigned short* tile_rank;
  AMDR_TRY(tmp.alloc(&rm_ids, (size_t)n_remove, who));
  AMDR_TRY(tmp.alloc(&doc_new, (size_t)n_old, who));
  AMDR_TRY(tmp.alloc(&tile_rank, (size_t)nnz_old + 1, who));  // (+ 1: never an empty allocation)
  AMDR_TRY(tmp.alloc(&tile_cnt, (size_t)tiles + 1, who));
  AMDR_TRY(tmp.alloc(&tile_base, (size_t)tiles + 1, who));
  AMDR_TRY(tmp.alloc(&rank_at, (size_t)V_old + 1, who));
  AMDR_TRY(tmp.alloc(&df_new, (size_t)V_new + 1, who));
  if (term_map) AMDR_TRY(tmp.alloc(&map_dev, (size_t)V_old + 1, who));
  AMDR_TRY(tmp.alloc(&flag_dev, 1, who));
  hipStream_t st = h->stream;
  AMDR_HIP(hipMemcpyAsync(rm_ids, remove_ids, (size_t)n_remove * sizeof(long long), hipMemcpyHostToDevice, st));
  if (term_map && V_old) AMDR_HIP(hipMemcpyAsync(map_dev, term_map, (size_t)V_old * sizeof(int), hipMemcpyHostToDevice, st));
  if (V_new) AMDR_HIP(hipMemcpyAsync(nx.idf, idf, (size_t)V_new * sizeof(double), hipMemcpyHostToDevice, st));
  AMDR_HIP(hipMemsetAsync(flag_dev, 0, sizeof(int), st));
  // the passes in two stretches, with the host's look at nnz_new between them (amdr_bm25_remove_kernel_ms)
  KernelSpans timer(2);
  AMDR_TRY(timer.begin(0, st));
  hipLaunchKernelGGL(bm25_rm_docmap_kernel, dim3((unsigned)((n_old + 255) / 256)), dim3(256), 0, st, rm_ids, (long)n_remove,
                     old.doc_len, (long)n_old, doc_new, nx.doc_len, tc.kept_old);
  AMDR_HIP(hipGetLastError());
  if (tiles > 0) {
    hipLaunchKernelGGL(bm25_rm_count_kernel, dim3((unsigned)tiles), dim3(kBmTileThreads), 0, st, old.post_doc,
                       (long long)nnz_old, doc_new, tile_rank, tile_cnt);
    AMDR_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(compact_scan_i64_kernel, dim3(1), dim3(kCompactScanThreads), 0, st, tile_cnt, (long)tiles, tile_base);
  AMDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(bm25_rm_terms_kernel, dim3((unsigned)((V_old + 1 + 255) / 256)), dim3(256), 0, st, old.term_ptr,
                     (long)V_old, (long long)nnz_old, tile_base, tile_rank, map_dev, rank_at, df_new, flag_dev);
  AMDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(compact_scan_i64_kernel, dim3(1), dim3(kCompactScanThreads), 0, st, df_new, (long)V_new, nx.term_ptr);
  AMDR_HIP(hipGetLastError());
  AMDR_TRY(timer.end(0, st));
  AMDR_TRY(tc.scan(nx.doc_len, n_old - n_remove, st));
  long long nnz_new = 0;
  int flag = 0;
  AMDR_HIP(hipMemcpyAsync(&nnz_new, tile_base + tiles, sizeof(long long), hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipMemcpyAsync(&flag, flag_dev, sizeof(int), hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipStreamSynchronize(st));
  AMDR_REQUIRE(flag == 0, "bm25_remove: a term mapped to -1 still has a surviving posting");
  if (nnz_new < 0 || nnz_new > nnz_old) return fail(AMDR_EHIP, "bm25_remove: counted %lld of %lld postings", nnz_new, (long long)nnz_old);
  AMDR_TRY(nx.alloc_postings(nnz_new, who));
  AMDR_TRY(timer.begin(1, st));
  if (tiles > 0 && nnz_new > 0) {
    hipLaunchKernelGGL(bm25_rm_scatter_kernel, dim3((unsigned)tiles), dim3(kBmTileThreads), 0, st, old.term_ptr, (long)V_old,
                       old.post_doc, old.post_tf, (long long)nnz_old, doc_new, nx.doc_len, tile_base, tile_rank, rank_at,
                       nx.term_ptr, map_dev, nnz_new, avgdl, h->k1, h->b, nx.post_doc, nx.post_tf, nx.post_w);
    AMDR_HIP(hipGetLastError());
  }
  AMDR_TRY(timer.end(1, st));
  // the stream: the survivors' documents in their old order, every token through the map
  TcArgs ta = tc_args(kTcRemove, h, n_old - n_remove, 0, V_new);
  ta.kept_old = tc.kept_old, ta.term_map = map_dev;
  AMDR_TRY(tc.run(ta, tc.n_tok_new, nullptr, nullptr, st, who));
  AMDR_HIP(hipStreamSynchronize(st));
  AMDR_REQUIRE(tc.flag == 0, "bm25_remove_carry: a token of a surviving document is mapped to -1, or a gather index of the "
                             "carry is outside its array");
  h->remove_kernel_ms = timer.ms();
  nx.commit(h->ix, h->removes);  // from here on nothing can fail
  tc.commit(h);
  return AMDR_OK;
}

int bm25_replace_body(amdr_bm25_t* h, const int64_t* replace_ids, int64_t n_rep, const int64_t* term_ptr_add,
                      const int32_t* post_doc_add, const int32_t* post_tf_add, const int32_t* doc_len_add,
                      const int32_t* term_map, int64_t n_terms_new, const double* idf, double avgdl, bool carry,
                      const int64_t* tok_ptr_add, const int32_t* tok_add) {
  static const char* const who = "bm25_replace";
  AMDR_REQUIRE(h != nullptr, "bm25_replace: null handle");
  AMDR_REQUIRE(n_rep >= 0, "bm25_replace: n_rep=%lld", (long long)n_rep);
  if (n_rep == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  const BmIndex& old = h->ix;
  AMDR_REQUIRE(n_terms_new >= 0 && n_terms_new < (1ll << 31), "bm25_replace: n_terms_new=%lld", (long long)n_terms_new);
  std::unique_ptr<int32_t[]> inv(new (std::nothrow) int32_t[(size_t)n_terms_new + 1]);
  if (!inv) return fail(AMDR_ENOMEM, "bm25_replace: no host memory for the inverse term map");
  const int bad = bm_rp_validate(replace_ids, n_rep, term_ptr_add, post_doc_add, post_tf_add, doc_len_add, term_map,
                                 n_terms_new, idf, avgdl, old.n_terms, old.n_docs, inv.get());
  AMDR_REQUIRE(bad == kBmRpOk, "bm25_replace: %s", bm_rp_error_text(bad));
  if (carry) {
    const int tbad = tc_validate_add(tok_ptr_add, tok_add, doc_len_add, n_rep, n_terms_new);
    AMDR_REQUIRE(tbad == kPhValid, "bm25_replace_carry: the new documents' token stream: %s", ph_error_text(tbad));
  }
  TokCarry tc(carry && h->has_tokens);  // without a resident stream the call is the plain call
  AMDR_HIP(hipSetDevice(h->device));
  const int64_t V_old = old.n_terms, V_new = n_terms_new, nnz_old = old.nnz, n = old.n_docs, nnz_add = term_ptr_add[V_new];
  const long long tiles = (nnz_old + kBmTile - 1) / kBmTile, add_tiles = (nnz_add + kBmTile - 1) / kBmTile;
  AMDR_REQUIRE(tiles < (1ll << 31) && add_tiles < (1ll << 31), "bm25_replace: %lld + %lld postings exceed the grid",
               (long long)nnz_old, (long long)nnz_add);
  BmStagedIndex nx;
  AMDR_TRY(nx.alloc_tables(V_new, n, avgdl, who));
  AMDR_TRY(tc.begin(n, false, who));
  CallScratch tmp;
  long long *rp_ids, *tile_cnt, *tile_base, *rank_at, *df_new, *add_ptr;
  int *doc_keep, *map_dev = nullptr, *inv_dev, *flag_dev, *add_doc, *add_tf, *add_len;
  unsigned short* tile_rank;
  AMDR_TRY(tmp.alloc(&rp_ids, (size_t)n_rep, who));
  AMDR_TRY(tmp.alloc(&doc_keep, (size_t)n, who));
  AMDR_TRY(tmp.alloc(&tile_rank, (size_t)nnz_old + 1, who));  // (+ 1: never an empty allocation)
  AMDR_TRY(tmp.alloc(&tile_cnt, (size_t)tiles + 1, who));
  AMDR_TRY(tmp.alloc(&tile_base, (size_t)tiles + 1, who));
  AMDR_TRY(tmp.alloc(&rank_at, (size_t)V_old + 1, who));
  AMDR_TRY(tmp.alloc(&df_new, (size_t)V_new + 1, who));
  if (term_map) AMDR_TRY(tmp.alloc(&map_dev, (size_t)V_old + 1, who));
  AMDR_TRY(tmp.alloc(&inv_dev, (size_t)V_new + 1, who));
  AMDR_TRY(tmp.alloc(&flag_dev, 1, who));
  AMDR_TRY(tmp.alloc(&add_ptr, (size_t)V_new + 1, who));
  AMDR_TRY(tmp.alloc(&add_doc, (size_t)nnz_add + 1, who));
  AMDR_TRY(tmp.alloc(&add_tf, (size_t)nnz_add + 1, who));
  AMDR_TRY(tmp.alloc(&add_len, (size_t)n_rep, who));
  hipStream_t st = h->stream;
  AMDR_HIP(hipMemcpyAsync(rp_ids, replace_ids, (size_t)n_rep * sizeof(long long), hipMemcpyHostToDevice, st));
  AMDR_HIP(hipMemcpyAsync(add_len, doc_len_add, (size_t)n_rep * sizeof(int), hipMemcpyHostToDevice, st));
  AMDR_HIP(hipMemcpyAsync(add_ptr, term_ptr_add, (size_t)(V_new + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
  if (nnz_add) {
    AMDR_HIP(hipMemcpyAsync(add_doc, post_doc_add, (size_t)nnz_add * sizeof(int), hipMemcpyHostToDevice, st));
    AMDR_HIP(hipMemcpyAsync(add_tf, post_tf_add, (size_t)nnz_add * sizeof(int), hipMemcpyHostToDevice, st));
  }
  if (term_map && V_old) AMDR_HIP(hipMemcpyAsync(map_dev, term_map, (size_t)V_old * sizeof(int), hipMemcpyHostToDevice, st));
  if (V_new) {
    AMDR_HIP(hipMemcpyAsync(inv_dev, inv.get(), (size_t)V_new * sizeof(int), hipMemcpyHostToDevice, st));
    AMDR_HIP(hipMemcpyAsync(nx.idf, idf, (size_t)V_new * sizeof(double), hipMemcpyHostToDevice, st));
  }
  AMDR_HIP(hipMemsetAsync(flag_dev, 0, sizeof(int), st));
  // the passes in two stretches, with the host's look at nnz_new between them (amdr_bm25_replace_kernel_ms)
  KernelSpans timer(2);
  AMDR_TRY(timer.begin(0, st));
  hipLaunchKernelGGL(bm25_rp_docmap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rp_ids, (long)n_rep,
                     old.doc_len, add_len, (long)n, doc_keep, nx.doc_len);
  AMDR_HIP(hipGetLastError());
  if (tiles > 0) {  // the remove's counting pass: doc_keep is its document map
    hipLaunchKernelGGL(bm25_rm_count_kernel, dim3((unsigned)tiles), dim3(kBmTileThreads), 0, st, old.post_doc,
                       (long long)nnz_old, doc_keep, tile_rank, tile_cnt);
    AMDR_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(compact_scan_i64_kernel, dim3(1), dim3(kCompactScanThreads), 0, st, tile_cnt, (long)tiles, tile_base);
  AMDR_HIP(hipGetLastError());
  const int64_t entries = V_old + 1 > V_new ? V_old + 1 : V_new;
  hipLaunchKernelGGL(bm25_rp_terms_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, old.term_ptr,
                     (long)V_old, (long)V_new, (long long)nnz_old, tile_base, tile_rank, map_dev, inv_dev, add_ptr, rank_at,
                     df_new, flag_dev);
  AMDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(compact_scan_i64_kernel, dim3(1), dim3(kCompactScanThreads), 0, st, df_new, (long)V_new, nx.term_ptr);
  AMDR_HIP(hipGetLastError());
  AMDR_TRY(timer.end(0, st));
  AMDR_TRY(tc.scan(nx.doc_len, n, st));
  long long kept = 0;
  int flag = 0;
  AMDR_HIP(hipMemcpyAsync(&kept, tile_base + tiles, sizeof(long long), hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipMemcpyAsync(&flag, flag_dev, sizeof(int), hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipStreamSynchronize(st));
  AMDR_REQUIRE(flag == 0, "bm25_replace: a term mapped to -1 still has a surviving posting");
  if (kept < 0 || kept > nnz_old) return fail(AMDR_EHIP, "bm25_replace: counted %lld of %lld postings", kept, (long long)nnz_old);
  const long long nnz_new = kept + nnz_add;
  AMDR_TRY(nx.alloc_postings(nnz_new, who));
  AMDR_TRY(timer.begin(1, st));
  if (tiles > 0 && kept > 0) {
    hipLaunchKernelGGL(bm25_rp_scatter_old_kernel, dim3((unsigned)tiles), dim3(kBmTileThreads), 0, st, old.term_ptr,
                       (long)V_old, old.post_doc, old.post_tf, (long long)nnz_old, doc_keep, nx.doc_len, tile_base, tile_rank,
                       rank_at, nx.term_ptr, map_dev, add_ptr, add_doc, rp_ids, nnz_new, avgdl, h->k1, h->b, nx.post_doc,
                       nx.post_tf, nx.post_w);
    AMDR_HIP(hipGetLastError());
  }
  if (add_tiles > 0) {
    hipLaunchKernelGGL(bm25_rp_scatter_add_kernel, dim3((unsigned)add_tiles), dim3(kBmTileThreads), 0, st, add_ptr,
                       (long)V_new, add_doc, add_tf, (long long)nnz_add, rp_ids, inv_dev, old.term_ptr, old.post_doc,
                       (long long)nnz_old, tile_base, tile_rank, rank_at, nx.term_ptr, nx.doc_len, nnz_new, avgdl, h->k1,
                       h->b, nx.post_doc, nx.post_tf, nx.post_w);
    AMDR_HIP(hipGetLastError());
  }
  AMDR_TRY(timer.end(1, st));
  // the stream: document replace_ids[i] takes local i's tokens, every other document its own through the map
  TcArgs ta = tc_args(kTcReplace, h, n, n_rep, V_new);
  ta.replace_ids = rp_ids, ta.term_map = map_dev;
  AMDR_TRY(tc.run(ta, tc.n_tok_new, tok_ptr_add, tok_add, st, who));
  AMDR_HIP(hipStreamSynchronize(st));
  AMDR_REQUIRE(tc.flag == 0, "bm25_replace_carry: a token of a surviving document is mapped to -1, or a gather index of the "
                             "carry is outside its array");
  h->replace_kernel_ms = timer.ms();
  nx.commit(h->ix, h->replaces);  // from here on nothing can fail
  tc.commit(h);
  return AMDR_OK;
}

}  // namespace

extern "C" {

int amdr_bm25_add(amdr_bm25_t* h, const int64_t* term_ptr_add, const int32_t* post_doc_add, const int32_t* post_tf_add,
                  const double* idf, const int32_t* doc_len_add, int64_t n_terms, int64_t n_add, double avgdl) {
  return bm25_add_body(h, term_ptr_add, post_doc_add, post_tf_add, idf, doc_len_add, n_terms, n_add, avgdl, false, nullptr,
                       nullptr);
}

int amdr_bm25_add_carry(amdr_bm25_t* h, const int64_t* term_ptr_add, const int32_t* post_doc_add, const int32_t* post_tf_add,
                        const double* idf, const int32_t* doc_len_add, int64_t n_terms, int64_t n_add, double avgdl,
                        const int64_t* tok_ptr_add, const int32_t* tok_add) {
  return bm25_add_body(h, term_ptr_add, post_doc_add, post_tf_add, idf, doc_len_add, n_terms, n_add, avgdl, true, tok_ptr_add,
                       tok_add);
}

int amdr_bm25_remove(amdr_bm25_t* h, const int64_t* remove_ids, int64_t n_remove, const int32_t* term_map,
                     int64_t n_terms_new, const double* idf, double avgdl) {
  return bm25_remove_body(h, remove_ids, n_remove, term_map, n_terms_new, idf, avgdl, false);
}

int amdr_bm25_remove_carry(amdr_bm25_t* h, const int64_t* remove_ids, int64_t n_remove, const int32_t* term_map,
                           int64_t n_terms_new, const double* idf, double avgdl) {
  return bm25_remove_body(h, remove_ids, n_remove, term_map, n_terms_new, idf, avgdl, true);
}

int amdr_bm25_replace(amdr_bm25_t* h, const int64_t* replace_ids, int64_t n_rep, const int64_t* term_ptr_add,
                      const int32_t* post_doc_add, const int32_t* post_tf_add, const int32_t* doc_len_add,
                      const int32_t* term_map, int64_t n_terms_new, const double* idf, double avgdl) {
  return bm25_replace_body(h, replace_ids, n_rep, term_ptr_add, post_doc_add, post_tf_add, doc_len_add, term_map, n_terms_new,
                           idf, avgdl, false, nullptr, nullptr);
}

int amdr_bm25_replace_carry(amdr_bm25_t* h, const int64_t* replace_ids, int64_t n_rep, const int64_t* term_ptr_add,
                            const int32_t* post_doc_add, const int32_t* post_tf_add, const int32_t* doc_len_add,
                            const int32_t* term_map, int64_t n_terms_new, const double* idf, double avgdl,
                            const int64_t* tok_ptr_add, const int32_t* tok_add) {
  return bm25_replace_body(h, replace_ids, n_rep, term_ptr_add, post_doc_add, post_tf_add, doc_len_add, term_map, n_terms_new,
                           idf, avgdl, true, tok_ptr_add, tok_add);
}

int amdr_bm25_set_tokens(amdr_bm25_t* h, const int64_t* doc_ptr, const int32_t* tokens) {
  static const char* const who = "bm25_set_tokens";
  AMDR_REQUIRE(h != nullptr, "bm25_set_tokens: null handle");
  AMDR_REQUIRE(doc_ptr != nullptr && tokens != nullptr, "bm25_set_tokens: null array");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  const BmIndex& ix = h->ix;
  const int64_t n = ix.n_docs;
  std::unique_ptr<int32_t[]> len(new (std::nothrow) int32_t[(size_t)n + 1]);
  if (!len) return fail(AMDR_ENOMEM, "bm25_set_tokens: no host memory for %lld document lengths", (long long)n);
  if (n) AMDR_HIP(hipMemcpy(len.get(), ix.doc_len, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  const int bad = ph_validate_stream(doc_ptr, tokens, len.get(), n, ix.n_terms);
  AMDR_REQUIRE(bad == kPhValid, "bm25_set_tokens: %s", ph_error_text(bad));
  const int64_t n_tok = doc_ptr[n];
  long long* np = nullptr;
  int* nt = nullptr;
  int rc = dev_alloc(&np, (size_t)n + 1, who);
  if (!rc) rc = dev_alloc(&nt, (size_t)n_tok + 1, who);  // (+ 1: never an empty allocation)
  if (!rc && hipMemcpy(np, doc_ptr, (size_t)(n + 1) * sizeof(long long), hipMemcpyHostToDevice) != hipSuccess) rc = AMDR_EHIP;
  if (!rc && n_tok && hipMemcpy(nt, tokens, (size_t)n_tok * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) rc = AMDR_EHIP;
  if (rc) {  // the handle keeps what it had
    if (rc == AMDR_EHIP) (void)fail(AMDR_EHIP, "bm25_set_tokens: the upload failed: %s", hipGetErrorString(hipGetLastError()));
    if (np) (void)hipFree(np);
    if (nt) (void)hipFree(nt);
    return rc;
  }
  h->drop_tokens();
  h->tok_ptr = np, h->tok = nt, h->n_tokens = n_tok, h->has_tokens = true;
  return AMDR_OK;
}

int amdr_bm25_tokens_info(amdr_bm25_t* h, int64_t* out2) {
  AMDR_REQUIRE(h && out2, "bm25_tokens_info: null");
  std::lock_guard<std::mutex> g(h->mu);
  out2[0] = h->has_tokens ? 1 : 0;
  out2[1] = h->has_tokens ? h->n_tokens : 0;
  return AMDR_OK;
}

int amdr_bm25_read_tokens(amdr_bm25_t* h, int64_t* doc_ptr, int32_t* tokens) {
  AMDR_REQUIRE(h != nullptr, "bm25_read_tokens: null handle");
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc = bm_require_tokens(h, "bm25_read_tokens")) return rc;
  AMDR_HIP(hipSetDevice(h->device));
  if (doc_ptr) AMDR_HIP(hipMemcpy(doc_ptr, h->tok_ptr, (size_t)(h->ix.n_docs + 1) * sizeof(long long), hipMemcpyDeviceToHost));
  if (tokens && h->n_tokens) AMDR_HIP(hipMemcpy(tokens, h->tok, (size_t)h->n_tokens * sizeof(int), hipMemcpyDeviceToHost));
  return AMDR_OK;
}

int amdr_bm25_carry_kernel_ms(amdr_bm25_t* h, double* ms) {
  AMDR_REQUIRE(h && ms, "bm25_carry_kernel_ms: null");
  std::lock_guard<std::mutex> g(h->mu);
  *ms = h->carry_kernel_ms;
  return AMDR_OK;
}

int amdr_bm25_replace_kernel_ms(amdr_bm25_t* h, double* ms) {
  AMDR_REQUIRE(h && ms, "bm25_replace_kernel_ms: null");
  std::lock_guard<std::mutex> g(h->mu);
  *ms = h->replace_kernel_ms;
  return AMDR_OK;
}

int amdr_bm25_replaces(amdr_bm25_t* h, int64_t* n) {
  AMDR_REQUIRE(h && n, "bm25_replaces: null");
  std::lock_guard<std::mutex> g(h->mu);
  *n = h->replaces;
  return AMDR_OK;
}

int amdr_bm25_add_kernel_ms(amdr_bm25_t* h, double* ms) {
  AMDR_REQUIRE(h && ms, "bm25_add_kernel_ms: null");
  std::lock_guard<std::mutex> g(h->mu);
  *ms = h->add_kernel_ms;
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
  out6[0] = h->ix.n_docs;
  out6[1] = h->ix.n_terms;
  out6[2] = h->ix.nnz;
  out6[3] = h->adds;
  out6[4] = kBmTile;
  out6[5] = h->removes;
  return AMDR_OK;
}

int amdr_bm25_read(amdr_bm25_t* h, int64_t* term_ptr, int32_t* post_doc, int32_t* post_tf, double* post_w, double* idf,
                   int32_t* doc_len) {
  AMDR_REQUIRE(h != nullptr, "bm25_read: null handle");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  const BmIndex& ix = h->ix;
  const size_t V = (size_t)ix.n_terms, nnz = (size_t)ix.nnz, n = (size_t)ix.n_docs;
  if (term_ptr) AMDR_HIP(hipMemcpy(term_ptr, ix.term_ptr, (V + 1) * sizeof(long long), hipMemcpyDeviceToHost));
  if (post_doc && nnz) AMDR_HIP(hipMemcpy(post_doc, ix.post_doc, nnz * sizeof(int), hipMemcpyDeviceToHost));
  if (post_tf && nnz) AMDR_HIP(hipMemcpy(post_tf, ix.post_tf, nnz * sizeof(int), hipMemcpyDeviceToHost));
  if (post_w && nnz) AMDR_HIP(hipMemcpy(post_w, ix.post_w, nnz * sizeof(double), hipMemcpyDeviceToHost));
  if (idf && V) AMDR_HIP(hipMemcpy(idf, ix.idf, V * sizeof(double), hipMemcpyDeviceToHost));
  if (doc_len && n) AMDR_HIP(hipMemcpy(doc_len, ix.doc_len, n * sizeof(int), hipMemcpyDeviceToHost));
  return AMDR_OK;
}

}  // extern "C"

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
// The resident arrays are one BmIndex (bm25_handle.hpp); amdr_bm25_add and amdr_bm25_remove replace it (bm25_update.hip).
#include "common.hpp"
#include "topk.hpp"
#include "topk_merge.hpp"

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <new>
#include <vector>

#include "bm25_core.hpp"
#include "bm25_handle.hpp"

using namespace amdr;

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
  bm_plan(h->ix.n_docs, nq, k, &p);
  C64* part = nullptr;
  if (scores_dev) {
    int rc = h->part[ws].ensure(bm_part_bytes(h->ix.n_docs, nq, k));
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
  const BmIndex& ix = h->ix;
  // The batch is the grid's y: pieces (grid_y_pieces).  A piece is handed the call's nq and its own rows of q_ptr, of the
  // outputs and of every slab's list ([slab][nq][k] + q0 * k), so the pieces fill one set of lists and one merge reads it.
#define AMDR_BM_LAUNCH(NVT)                                                                                            \
  hipLaunchKernelGGL((bm25_score_topk_kernel<1, NVT>), dim3(p.nslabs, m), dim3(64), p.lds, st, ix.term_ptr,            \
                     ix.post_doc, ix.post_w, ix.idf, (long)ix.n_terms, (long)ix.n_docs, q_terms_dev, q_ptr_dev + q0,   \
                     nq, k, p.cap, p.slab, bm_select_enabled() ? 1 : 0,                                                \
                     full_dev ? full_dev + (size_t)q0 * ix.n_docs : nullptr, part ? part + (size_t)q0 * k : nullptr,  \
                     fs ? fs + (size_t)q0 * k : nullptr, fi ? fi + (size_t)q0 * k : nullptr)
  const int nv = bm_use_argmax(k, p.slab) ? (p.slab + 63) / 64 : 1;  // the staged selector needs no register bucket
  const int rc = grid_y_pieces(nq, [&](int q0, int m) -> int {
    if (nv <= 4) AMDR_BM_LAUNCH(4);
    else if (nv <= 8) AMDR_BM_LAUNCH(8);
    else if (nv <= 10) AMDR_BM_LAUNCH(10);
    else if (nv <= 16) AMDR_BM_LAUNCH(16);
    else if (nv <= 20) AMDR_BM_LAUNCH(20);
    else AMDR_BM_LAUNCH(32);
    AMDR_HIP(hipGetLastError());
    return AMDR_OK;
  });
#undef AMDR_BM_LAUNCH
  if (rc) return rc;
  if (scores_dev && !direct) return launch_merge_packed(part, p.nslabs, nq, k, p.cap_merge, scores_dev, ids_dev, st);
  return AMDR_OK;
}

}  // namespace
namespace amdr {
int bm25_small_raw(amdr_bm25_t* h, int nq, int k, Bm25Raw* out) {
  if (!h->ticket.p) return fail(AMDR_EINVAL, "bm25: handle without arrival counters");
  BmPlan p;
  bm_plan(h->ix.n_docs, nq, k, &p);
  out->term_ptr = h->ix.term_ptr;
  out->post_doc = h->ix.post_doc;
  out->post_w = h->ix.post_w;
  out->idf = h->ix.idf;
  out->n_terms = (long)h->ix.n_terms;
  out->n_docs = (long)h->ix.n_docs;
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

// count values of src behind a padded allocation (BmIndex::alloc)
template <class T>
int upload(T** dst, const T* src, size_t count) {
  const int rc = BmIndex::alloc(dst, count, "bm25_create");
  if (rc) return rc;
  if (count) AMDR_HIP(hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
  return AMDR_OK;
}

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
  h->ix.n_terms = n_terms;
  h->ix.n_docs = n_docs;
  h->ix.nnz = nnz;
  h->ix.avgdl = avgdl;
  h->k1 = k1;
  h->b = b;
  // Per-posting factor of rank_bm25's expression, operand for operand in numpy's order
  // (this translation unit is built with -ffp-contract=off; IEEE fp64 mul/add/div are
  // correctly rounded on the host as on the device, so the value is the one numpy computes).
  std::vector<double> pw((size_t)nnz);
  for (int64_t p = 0; p < nnz; ++p) pw[(size_t)p] = bm25_factor(post_tf[p], doc_len[post_doc[p]], avgdl, k1, b);
  rc = upload(&h->ix.term_ptr, (const long long*)term_ptr, (size_t)n_terms + 1);
  if (!rc) rc = upload(&h->ix.post_doc, post_doc, (size_t)nnz);
  if (!rc) rc = upload(&h->ix.post_w, pw.data(), (size_t)nnz);
  if (!rc) rc = upload(&h->ix.idf, idf, (size_t)n_terms);
  if (!rc) rc = upload(&h->ix.post_tf, post_tf, (size_t)nnz);
  if (!rc) rc = upload(&h->ix.doc_len, doc_len, (size_t)n_docs);
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
  *n = h->ix.n_docs;
  return AMDR_OK;
}

int amdr_bm25_reserve(amdr_bm25_t* h, int32_t nq_max, int32_t k_max, int64_t total_terms_max) {
  AMDR_REQUIRE(h != nullptr, "bm25_reserve: null handle");
  AMDR_REQUIRE(nq_max >= 1 && k_max >= 1 && k_max <= AMDR_MAX_K && total_terms_max >= 0, "bm25_reserve: bad sizes");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  int rc = h->part[0].ensure(bm_reserve_bytes(h->ix.n_docs, nq_max, k_max));
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
  bm_plan(h->ix.n_docs, nq, k, &p);
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
  if ((rc = h->full.ensure((size_t)nq * h->ix.n_docs * sizeof(double)))) return rc;
  rc = bm_run(h, 1, h->qterms.as<int>(), h->qptr.as<long long>(), nq, 1, nullptr, nullptr, h->full.as<double>(),
              h->stream);
  if (rc) return rc;
  AMDR_HIP(hipMemcpyAsync(scores_host, h->full.p, (size_t)nq * h->ix.n_docs * sizeof(double), hipMemcpyDeviceToHost,
                          h->stream));
  AMDR_HIP(hipStreamSynchronize(h->stream));
  return AMDR_OK;
}

int amdr_bm25_destroy(amdr_bm25_t* h) {
  if (!h) return AMDR_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamDestroy(h->stream);
  }
  h->ix.free();
  h->part[0].release();
  h->part[1].release();
  h->qterms.release();
  h->qptr.release();
  h->sbuf.release();
  h->ibuf.release();
  h->full.release();
  h->tscope.release();
  h->ticket.release();
  h->drop_tokens();
  delete h;
  return AMDR_OK;
}

}  // extern "C"

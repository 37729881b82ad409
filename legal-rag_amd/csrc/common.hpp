// Shared host-side plumbing for libamdretrieval (error strings, HIP checks).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>

#include "../../include/amdretrieval.h"

namespace amdr {

std::string& last_error_ref();
int fail(int code, const char* fmt, ...);
// (re)allocations of every DevBuf in the process since the library was loaded (amdr_workspace_growths)
std::atomic<long long>& devbuf_growths();

#define AMDR_HIP(expr)                                                                          \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess)                                                                       \
      return ::amdr::fail(_e == hipErrorOutOfMemory ? AMDR_ENOMEM : AMDR_EHIP, "%s failed: %s (%s:%d)", \
                          #expr, hipGetErrorString(_e), __FILE__, __LINE__);                    \
  } while (0)

#define AMDR_REQUIRE(cond, ...) \
  do {                          \
    if (!(cond)) return ::amdr::fail(AMDR_EINVAL, __VA_ARGS__); \
  } while (0)

// Growable device buffer owned by a handle (never shrinks).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return AMDR_OK;
    if (p) {
      AMDR_HIP(hipFree(p));
      p = nullptr;
      cap = 0;
    }
    devbuf_growths().fetch_add(1, std::memory_order_relaxed);
    AMDR_HIP(hipMalloc(&p, bytes));
    cap = bytes;
    return AMDR_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
inline int next_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}
// top-k staging capacity: power of two, >= k + 64 (one wave of appends always fits)
inline int topk_cap(int k) { return next_pow2(k + 64) < 128 ? 128 : next_pow2(k + 64); }

int check_device(int device);

// A grid's y (and z) is sure to hold 65 535 blocks: hipDeviceProp_t::maxGridSize of the MI355X reports 65 536 for both.  (Its
// ROCm runtime took the unsplit launches of 65 541 queries as well, with the same results; nothing here relies on that.)  A
// launch that carries the batch in y goes in pieces of at most that many queries, one after the other on the caller's
// stream: piece(q0, m) enqueues queries [q0, q0 + m) and returns a status.  A batch of up to 65 535 queries is one piece,
// piece(0, nq): the launch it always was.
constexpr int kGridYMax = 65535;
template <class Piece>
int grid_y_pieces(int nq, Piece&& piece) {
  for (int q0 = 0; q0 < nq; q0 += kGridYMax) {
    const int rc = piece(q0, nq - q0 < kGridYMax ? nq - q0 : kGridYMax);
    if (rc) return rc;
  }
  return AMDR_OK;
}

// A chunk matrix larger than the 256 MiB Infinity Cache is streamed with the non-temporal policy
// (read once per scan; nothing to keep on-die).  AMDR_DENSE_NT=0|1 pins the choice.
inline bool dense_stream_nontemporal(long n, int d) {
  const char* e = getenv("AMDR_DENSE_NT");
  if (e && (e[0] == '0' || e[0] == '1')) return e[0] == '1';
  return (size_t)n * (size_t)d * sizeof(float) > ((size_t)256 << 20);
}

// ---- batched (32-query tile, fp32 MFMA) dense path: dense_mfma.hip -----------
struct DenseMfmaPlan {
  int q_tiles, grid_x, grid_y, slabs, cap, waves;
  long rows_per_block, rows_per_slab, ld;  // ld = leading dimension of S (n rounded up to 32 floats)
  size_t lds_scores, s_bytes, part_bytes;
};
bool dense_mfma_supported(int d);
// grid = false: the top-k half and the sizes only (the search for the scores grid costs ~10 us on a large matrix)
void dense_mfma_plan(long n, int d, int nq, int k, DenseMfmaPlan* p, bool grid = true);
// tile_max false: S[query][row], every row's score; true: S[query][tile], the maximum over each 32-row tile
// `gate` (nullable device int): the launch does nothing unless *gate != 0 — the exact first pass behind the fp16 one
// (dense_hi.hip) is enqueued unconditionally and decides on the device whether it runs
int dense_mfma_launch_scores(const DenseMfmaPlan& p, const float* X, long n, int d, const float* Q, int nq, float* S,
                             hipStream_t st, bool tile_max = false, const int* gate = nullptr);
int dense_mfma_launch_topk(const DenseMfmaPlan& p, const float* S, long n, int nq, int k, void* part,
                           float* fin_scores, int64_t* fin_ids, hipStream_t st);
// the launch above ranks two queries per wave (scores_pair_topk_kernel) instead of one per block (scores_slab_topk_kernel)
bool dense_topk_pair_applies(const DenseMfmaPlan& p, long n, int nq, int k);

// ---- fp16 first pass of the two-level top-k on large matrices: dense_hi.hip ----
bool dense_hi_supported(int d);
int dense_hi_max_queries(int d);  // queries per scan: 64, 48 at d = 1 024
int dense_stats_launch(const float* X, long n, int d, unsigned int* words, hipStream_t st);  // (words: dense_fp16.hpp)
// round 4: the tail of a large search in four launches + two gated ones (dense_hi.hip, dense_mfma.hip)
long dense_hi2_sample_stride(long n, int qtiles);
long dense_hi2_sample_items(long n, int qtiles);
size_t dense_hi2_qcap(long n, int qtiles, int kc);
// image (nullable): the resident fp16 image of X (dense_hi_image.hpp) — sample and scan then read it instead of X
int dense_hi2_launch_sample(const float* X, const void* image, long n, int d, const float* Q, int nq, int qtiles, float* MT,
                            hipStream_t st, float x_scale);
int dense_hi2_launch_tau(const float* MT, long n, int d, int nq, int qtiles, int kc, float* tau, unsigned int* qcount,
                         int* flag, unsigned int* stats, hipStream_t st);
int dense_hi2_launch_emit(const float* X, const void* image, long n, int d, const float* Q, int nq, const float* tau, void* qlist,
                          unsigned int* qcount, size_t qcap, hipStream_t st, float x_scale, int qtiles);
int dense_hi2_launch_select(const void* qlist, const unsigned int* qcount, size_t qcap, int m, int kc, int k, const float* Q,
                            int d, float row_norm_max, float x_scale, long n_tiles, int* list, int* count, int* unres,
                            int* flag, unsigned int* unresolved, hipStream_t st);
// rows [row0, n) of X into the image, from the tile that holds row0 on (dense_hi_image.hip)
int dense_hi_image_launch(const float* X, long row0, long n, int d, float x_scale, void* image, hipStream_t st);
// the exact tail behind the tile maxima M (dense_mfma.hip): each query's k best tiles, ascending, into list[q][..] (gate,
// unres: nullable device pointers — null = always, every query; chosen, nullable: the tiles picked already, [m][k] best
// first, to be ordered only) -> the exact scores of their rows -> the final top-k
int dense_exact_select_launch(const float* M, long ldM, long n_tiles, int m, int k, int list_stride, int* list, int* count,
                              const int* unres, const int* gate, const int64_t* chosen, hipStream_t st);
int dense_rescore_tiles_launch(const float* X, long n_real, int d, const float* Q, int m, const int* list, const int* count,
                               int list_stride, int max_tiles, long ldS, float* S, hipStream_t st);
int dense_final_topk_launch(const float* S, long ldS, const int* list, const int* count, int list_stride, int max_tiles,
                            long n_real, int m, int k, float* fin_scores, int64_t* fin_ids, hipStream_t st);


// ---- dense top-k + fusion in one call (dense_tail.hip; dense.hip amdr_dense_search_fuse_device) ----
struct FuseTail {  // the fusion that follows the dense channel: parameters, the BM25 lists, the outputs (device pointers)
  const amdr_fuse_params_t* p;
  const int64_t* dense_row2uid;
  const int64_t* bm25_ids;
  const double* bm25_scores;
  int kb;
  const int64_t* bm25_row2uid;
  int64_t* out_ids;
  double* out_vals;
  int32_t* out_mask;
  int32_t* out_count;
};
// first pass of the two-pass long-batch form (dense_small_hi.hip): the fp16 image of a short chunk matrix (stats: dense_fp16.hpp)
struct DenseFp16Stats;
int dense_small_create_from(int device, const float* X, int64_t n, int d, const DenseFp16Stats& stats,
                            amdr_dense_small_t** out);
int dense_small_reserve(amdr_dense_small_t* h, int nq_max);
// second pass of the two-pass long-batch form (dense_tail.hip dense_hi_select_fuse_kernel): candidates inside the proven margin
// of the approximate scores in S, exact dots, top-k (+ the fusion when t != nullptr)
int dense_hi_select_launch(const FuseTail* t, int q0, const float* S, long ldS, long n, int m, int kd, const float* X,
                           const float* Q, int d, const float* eps, float* fin_scores, int64_t* fin_ids,
                           unsigned int* fallbacks, hipStream_t st);
// one kernel ranks the rows of S and fuses (dense_select_fuse_kernel): single slab, <= 1 024 rows, kd + kb <= 32
bool dense_select_fuse_applies(long n, int slabs, int m, int kd, int kb);
// queries [q0, q0 + m) of the batch: S holds their score rows; writes their dense lists and their fused outputs
int dense_select_fuse_launch(const FuseTail& t, int q0, const float* S, long ldS, long n, int m, int kd, int cap,
                             float* fin_scores, int64_t* fin_ids, hipStream_t st);
// the plain fusion launch over finished dense lists (the unfused path of the same call)
int dense_fuse_plain_launch(const FuseTail& t, int q0, int m, int kd, const float* dense_scores, const int64_t* dense_ids,
                            hipStream_t st);

// ---- the one-launch serving step (dense_tail.hip hybrid_small_kernel): what it needs from the two handles --------------
struct DenseRaw {
  const float* X;
  long n;
  int d;
  float* S;   // [nq][ld] score scratch of the "_device" workspace
  long ld;
};
// ensures the score scratch for nq rows (dense.hip)
int dense_small_raw(amdr_dense_t* h, int nq, DenseRaw* out);
struct Bm25Raw {
  const long long* term_ptr;
  const int* post_doc;
  const double* post_w;
  const double* idf;
  long n_terms, n_docs;
  int* ticket;   // [64] zeroed arrival counters of the one-launch step (self-resetting)
  int slab, nslabs, cap, nvt;
  size_t lds;
  bool argmax, select_on;
};
int bm25_small_raw(amdr_bm25_t* h, int nq, int k, Bm25Raw* out);  // (bm25.hip)
// the split-fp16 token image of a MaxSim store (scope.hip scores a scope's documents against it); img == nullptr: the
// store holds a NaN / infinity and has no image
struct MaxsimRaw {
  const unsigned char* img;
  const long long* doc_ptr;
  long n_docs;
  float unscale_d;  // 1 / the store's power-of-two scale
  int device;
};
int maxsim_raw(amdr_maxsim_t* h, MaxsimRaw* out);  // (maxsim.hip)
int bm25_device_of(const amdr_bm25_t* h);
std::mutex& dense_mutex(amdr_dense_t* h);
std::mutex& bm25_mutex(amdr_bm25_t* h);
int dense_device_of(const amdr_dense_t* h);
// the resident chunk matrix of a dense handle (graph.hip re-scores walked articles against it)
void dense_matrix(const amdr_dense_t* h, const float** X, long* n, int* d);
const DenseFp16Stats& dense_fp16_stats_of(const amdr_dense_t* h);  // its statistics of that matrix
// the staging buffer (>= bytes) and the stream of a dense handle's host-pointer entry points; the caller holds
// dense_mutex(h) until it has synchronised that stream (mmr.hip amdr_mmr)
int dense_host_stage(amdr_dense_t* h, size_t bytes, void** dev, hipStream_t* st);

// ---- ordered row compaction into a new buffer: rows_compact.hip (amdr_dense_remove, amdr_maxsim_remove; the map is
// rows_compact.hpp's; remove_ids is a DEVICE copy of a validated list) ----
// new row j of n_new, row_bytes each (a multiple of 16) <- old row src(j)
int rows_compact_launch(const void* src, long long n_new, long row_bytes, const long long* remove_ids, long n_remove,
                        void* dst, hipStream_t st);
// the doc_ptr rebuild: len / start [n_docs_new] scratch (a new document's length, the old row its rows start at),
// new_ptr [n_docs_new + 1] the exclusive scan of len
int segments_ptr_launch(const long long* doc_ptr, long n_docs_new, const long long* remove_ids, long n_remove,
                        long long* len, long long* start, long long* new_ptr, hipStream_t st);
// the 512-byte token rows of the surviving documents, rows_new = new_ptr[n_docs_new] of them
int segments_compact_launch(const void* src, long long rows_new, const long long* new_ptr, const long long* start,
                            long n_docs_new, void* dst, hipStream_t st);
// the replaces (amdr_dense_replace, amdr_maxsim_replace; replace_ids / add_ptr are DEVICE copies of validated lists):
// staged row i of n_rep -> row replace_ids[i] of dst, in place
int rows_scatter_launch(const void* rows, long long n_rep, long row_bytes, const long long* replace_ids, void* dst,
                        hipStream_t st);
// the doc_ptr of the edited store: len / start [n_docs] scratch (start signed: >= 0 an old row, < 0 staged row ~start),
// new_ptr [n_docs + 1] the exclusive scan of len
int splice_ptr_launch(const long long* doc_ptr, long n_docs, const long long* add_ptr, const long long* replace_ids,
                      long n_rep, long long* len, long long* start, long long* new_ptr, hipStream_t st);
// the 512-byte token rows of the edited store, each from old_rows or add_rows
int segments_splice_launch(const void* old_rows, const void* add_rows, long long rows_new, const long long* new_ptr,
                           const long long* start, long n_docs, void* dst, hipStream_t st);

// ---- long-batch dense path: dense_panel.hip (panel of chunk rows shared by a block through LDS) ----
struct DensePanelPlan {
  int parts, base, rem, nb, m_tiles, gm, waves;
  size_t lds;
};
bool dense_panel_supported(long n, int d, int nq);
void dense_panel_plan(long n, int d, int nq, DensePanelPlan* p);
int dense_panel_launch_scores(const DensePanelPlan& p, const float* X, long n, int d, const float* Q, int nq, long ldS,
                              float* S, hipStream_t st);

}  // namespace amdr

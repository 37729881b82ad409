// Class spans: a Prefix or a OneOf inside a phrase or a Near (sell! /5 good!, "secur! interest", (buyer purchaser) +3
// accept!) resolved into ascending document lists on the device.
//
// No reference counterpart: the reference's BM25 channel scores bags of words (legalrag/retrieval/bm25_retriever.py:74-75)
// and has neither token order, a stemmer nor a filter.  Here an item's SLOTS name token classes (class_span_rule.hpp): a
// plain token, or a class whose member ids are a union item and whose document list the union step (union_lists.hip) has
// already written into the call's list array.  The item is resolved from the resident token stream into ITS OWN ascending
// document list, appended to that same array, which amdr_term_scope_lists (term_scope.hip) reads as one more term.
//
// The three launches of list_step.hpp, no global atomics, deterministic, nothing allocated; the grid is ONE-dimensional,
// n_items x tiles blocks of kPhTile = 256 threads, cell = p * tiles + y (item p, tile y of 256 candidates of its driver):
//   count   the block resolves the item's slots into LDS (cs_slot: a class slot's member range and list), one thread links
//           equal slots and finds the driver — the shortest list, a posting list or a class list, known only here.  (1)
//           thread t tests the conjunction for candidate t: a lower-bound search in every other slot's list.  (2) one WAVE
//           walks one survivor, 64 anchors per round: each token of the round's run is read ONCE, coalesced, turned into
//           the mask of the slots it fills (cs_token_mask: for a class slot a lower-bound search in the member ids) and
//           staged as u16 in LDS; every lane then scans masks only (cs_lane_hit) and a wave vote ends the document at the
//           first round with a hit.  Masks, not tokens, are staged because a lane's window re-reads each position up to
//           n + 1 times: the search is paid once per token and round instead of once per token, lane and slot.  The block
//           ranks its kept candidates, parks rank-or-minus-one per candidate and writes counts[cell]; a driver longer than
//           cand_max: zero counts and status[p] = 1.
//   scan    compact_scan_i64_kernel over the counts: every cell's offset behind the array's start.
//   write   kept candidate -> docs[start + offsets[cell] + rank]; positions >= rows_cap are dropped and their items get
//           status[p] = 2; the block of tile 0 writes the item's list_ptr entry, clamped to rows_cap.
// One list array.  The call CONTINUES the array as the union step does: list_ptr has n_before + n_items + 1 entries of
// which the first n_before + 1 are written — the classes' lists among them, cls_first + n_cls <= n_before — start =
// list_ptr[n_before] is read ON THE DEVICE by the write pass, the entries n_before + 1 .. are written and the documents go
// behind `start`.  The count pass reads entries <= n_before only and documents below `start` only.
// The staging is traffic between the lanes of ONE wave (list_wave_lds_fence), so phase 2 holds no block
// barrier; every block barrier sits under a block-uniform condition.
// LDS: the slots (16 x 56 B), the driver, four runs of 320 u16 (2 560 B), the survivor list (512 B), the keep flags
// (256 B) and the scan's wave sums: under 4.5 KiB.  Workspace per cell: two i64 and 1 KiB of parked ranks.
// Worst case: a round of 319 tokens x 16 class slots x 12 dependent loads (a class of 4 096 ids) per wave, before any lane
// scans; the scan itself is near_rule's len x (n + 1) steps.
#include "class_span_rule.hpp"
#include "list_step.hpp"
#include "union_rule.hpp"

#include <memory>
#include <mutex>
#include <new>

using namespace amdr;

namespace {

constexpr int kCsThreads = kPhTile;
constexpr int kCsWaves = kCsThreads / 64;
constexpr int kCsStage = 320;  // u16 of one wave's staged run (kNearStage, rounded to a whole dword)
static_assert(kCsThreads % 64 == 0 && kPhLanes == 64 && kCsStage >= kNearStage, "whole waves; a run fits its stage");

// Workspace (list_work): a cell's payload is rank-or-minus-one i32 [256]
constexpr size_t kCsCellBytes = kCsThreads * sizeof(int);

struct CsItems {
  const long long* ptr;  // [n + 1]
  const int* slots;      // [ptr[n]]
  const int* kind;       // [n] SpanKind
  const int* dist;       // [n]; read for a Near only
};

// The block's item: its slots resolved into LDS by the first L threads (an item the rule does not define reads none),
// linked and given a driver by thread 0; ends with a barrier.  Returns the item's length, 0 for an undefined item.
__device__ __forceinline__ int cs_block_item(const CsIndex& I, const CsItems& S, long long p, CsSlot* slots, CsDriver* drv,
                                             int* kind_out, int* dist_out) {
  const long long b = S.ptr[p], L = S.ptr[p + 1] - b;
  const int kind = S.kind[p];
  const int dist = kind == kSpanPhrase ? 0 : S.dist[p];
  const bool sized = span_sized(kind, L, dist);  // block-uniform
  if (sized && threadIdx.x < L) slots[threadIdx.x] = cs_slot(I, S.slots[b + threadIdx.x]);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (sized) cs_link_slots(slots, (int)L);
    *drv = sized ? cs_driver(slots, (int)L) : CsDriver{-1, nullptr, 0, 0};
  }
  __syncthreads();
  *kind_out = kind, *dist_out = dist;
  return sized ? (int)L : 0;
}

__global__ __launch_bounds__(kCsThreads) void class_span_count_kernel(CsIndex I, CsItems S, long long tiles, long long cand_max,
                                                                     long long* __restrict__ counts,
                                                                     int* __restrict__ rank_out, int* __restrict__ status) {
  __shared__ CsSlot slots[kPhMaxLen];
  __shared__ CsDriver drv;
  __shared__ unsigned short stage[kCsWaves][kCsStage];
  __shared__ unsigned short surv[kCsThreads];
  __shared__ unsigned char kept[kCsThreads];
  __shared__ int wsum[kCsWaves + 1];
  const long long cell = blockIdx.x;
  const long long p = cell / tiles, tile = cell - p * tiles;
  int kind, dist;
  const int L = cs_block_item(I, S, p, slots, &drv, &kind, &dist);
  const CsDriver D = drv;
  const bool over = D.len > cand_max;
  if (tile == 0 && threadIdx.x == 0) status[p] = over ? kTsCandOverflow : kTsOk;
  const long long i0 = tile * kPhTile;
  if (over || D.at < 0 || i0 >= D.len) {  // block-uniform
    if (threadIdx.x == 0) counts[cell] = 0;
    return;
  }
  // phase 1: the conjunction, one candidate per thread
  const long long i = i0 + threadIdx.x;
  const bool all = i < D.len && cs_has_all(slots, L, D, D.docs[D.begin + i]);
  const int n_surv = list_compact_survivors<kCsThreads>(all, surv, kept, wsum);  // (barriers: every thread is here)
  // phase 2: one wave per survivor (n_surv is block-uniform; the loop holds no barrier)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned short* run = stage[wave];
  for (int s = wave; s < n_surv; s += kCsWaves) {
    const int t = surv[s];
    const long long doc = D.docs[D.begin + i0 + t];
    const long long end = I.ph.doc_ptr[doc + 1];
    bool found = false;
    for (long long base = I.ph.doc_ptr[doc]; base < end && !found; base += kPhLanes) {  // wave-uniform
      const int len = cs_run_len(base, end, kind, L, dist);  // <= kNearStage; base + len <= end
      for (int j = lane; j < len; j += kPhLanes)
        run[j] = (unsigned short)cs_token_mask(I.ph.tokens[base + j], slots, L, I.cls_terms);
      list_wave_lds_fence();
      found = __ballot(cs_lane_hit(run, len, lane, L, kind, dist)) != 0;
      list_wave_lds_fence();  // (the next round overwrites the run)
    }
    if (lane == 0) kept[t] = found ? 1 : 0;
  }
  list_rank_and_park<kCsThreads>(kept, wsum, rank_out + (size_t)cell * kCsThreads, counts + cell);  // (barriers: as above)
}

// (list_ptr and docs are the array the class lists are read from: neither is __restrict__)
__global__ __launch_bounds__(kCsThreads) void class_span_write_kernel(CsIndex I, CsItems S, long long tiles, long long cand_max,
                                                                     long long n_before, long long rows_cap,
                                                                     const long long* __restrict__ offsets,
                                                                     const int* __restrict__ rank_in, long long* list_ptr,
                                                                     int* docs, int* __restrict__ status) {
  __shared__ CsSlot slots[kPhMaxLen];
  __shared__ CsDriver drv;
  const long long cell = blockIdx.x;
  const long long p = cell / tiles, tile = cell - p * tiles;
  const long long start = list_start(list_ptr, n_before);
  if (tile == 0 && threadIdx.x == 0) {
    const int s = list_write_header(list_ptr, n_before, p, start + offsets[p * tiles], start + offsets[(p + 1) * tiles], rows_cap);
    if (s != kTsOk) status[p] = s;  // (an item over cand_max has no row: its 1 stays)
  }
  int kind, dist;
  (void)cs_block_item(I, S, p, slots, &drv, &kind, &dist);
  const CsDriver D = drv;
  const long long i0 = tile * kPhTile;
  if (D.len > cand_max || D.at < 0 || i0 >= D.len) return;  // block-uniform
  const long long at = list_kept_at(rank_in + (size_t)cell * kCsThreads, offsets, (size_t)cell, start, rows_cap);
  if (at >= 0) docs[at] = D.docs[D.begin + i0 + threadIdx.x];  // (a kept candidate lies inside the driver)
}

struct CsOut {
  long long* list_ptr;
  int* docs;
  int* status;
};

int cs_launch(const CsIndex& I, const CsItems& S, int64_t n_items, int64_t n_before, int64_t cand_max, int64_t rows_cap,
              const CsOut& o, unsigned char* work, hipStream_t st) {
  const long long tiles = ph_tiles(cand_max), cells = (long long)n_items * tiles;
  const dim3 grid((unsigned)cells);
  return list_launch(
      st, n_items, n_before, (size_t)cells, kCsCellBytes, o.list_ptr, work,
      [&](long long* counts, unsigned char* rank) {
        hipLaunchKernelGGL(class_span_count_kernel, grid, dim3(kCsThreads), 0, st, I, S, tiles, (long long)cand_max, counts,
                           (int*)rank, o.status);
      },
      [&](const long long* offsets, const unsigned char* rank) {
        hipLaunchKernelGGL(class_span_write_kernel, grid, dim3(kCsThreads), 0, st, I, S, tiles, (long long)cand_max,
                           (long long)n_before, (long long)rows_cap, offsets, (const int*)rank, o.list_ptr, o.docs, o.status);
      });
}

// sizes every entry point refuses (nothing is enqueued); *cells: the cells of the launch
int cs_check_sizes(const char* who, int64_t n_items, int64_t n_cls, int64_t cls_first, int64_t n_before, int64_t cand_max,
                   int64_t rows_cap, long long* cells) {
  AMDR_REQUIRE(n_items >= 0 && n_cls >= 0 && cls_first >= 0 && n_before >= 0 && cand_max >= 0 && rows_cap >= 0,
               "%s: a negative size", who);
  AMDR_REQUIRE(cls_first <= n_before && n_cls <= n_before - cls_first, "%s: the classes' lists %lld .. %lld do not lie among the "
               "%lld lists written before", who, (long long)cls_first, (long long)cls_first + (long long)n_cls, (long long)n_before);
  AMDR_REQUIRE(cs_cells(n_items, cand_max, cells), "%s: %lld items x %lld tiles of %d candidates are more than the %lld cells of "
               "one launch", who, (long long)n_items, ph_tiles(cand_max), kPhTile, kCsMaxCells);
  return AMDR_OK;
}

CsIndex cs_index(const amdr_bm25* h, const long long* x_ptr, const int* x_doc, const long long* cls_ptr, const int* cls_terms,
                 int64_t n_cls, int64_t cls_first) {
  return CsIndex{ph_index(h), x_ptr, x_doc, cls_ptr, cls_terms, (long)n_cls, (long)cls_first};
}

}  // namespace

extern "C" {

int amdr_class_spans_plan(int64_t n_items, int64_t cand_max, int64_t* work_bytes) {
  AMDR_REQUIRE(work_bytes != nullptr, "class_spans_plan: null");
  long long cells = 0;
  int rc = cs_check_sizes("class_spans_plan", n_items, 0, 0, 0, cand_max, 0, &cells);
  if (rc) return rc;
  *work_bytes = (int64_t)list_work((size_t)cells, kCsCellBytes).total;
  return AMDR_OK;
}

int amdr_class_spans_device(amdr_bm25_t* bm25, const int64_t* item_ptr_dev, const int32_t* item_slots_dev,
                            const int32_t* item_kind_dev, const int32_t* item_dist_dev, int64_t n_items,
                            const int64_t* cls_ptr_dev, const int32_t* cls_terms_dev, int64_t n_cls, int64_t cls_first,
                            int64_t n_before, int64_t cand_max, int64_t rows_cap, int64_t* list_ptr_dev, int32_t* docs_dev,
                            int32_t* out_status_dev, void* work_dev, int64_t work_bytes, void* stream) {
  static const char* const who = "class_spans";
  AMDR_REQUIRE(bm25 != nullptr, "%s: null handle", who);
  long long cells = 0;
  int rc = cs_check_sizes(who, n_items, n_cls, cls_first, n_before, cand_max, rows_cap, &cells);
  if (rc) return rc;
  if ((rc = bm_require_tokens(bm25, who))) return rc;
  AMDR_REQUIRE(list_ptr_dev != nullptr, "%s: null list_ptr", who);
  AMDR_REQUIRE(n_items == 0 || (item_ptr_dev && item_slots_dev && item_kind_dev && item_dist_dev && out_status_dev),
               "%s: null operand", who);
  AMDR_REQUIRE(n_cls == 0 || (cls_ptr_dev && cls_terms_dev), "%s: null class arrays", who);
  AMDR_REQUIRE(rows_cap == 0 || docs_dev, "%s: null docs", who);
  const size_t need = n_items ? list_work((size_t)cells, kCsCellBytes).total : 0;
  if ((rc = list_check_work(who, work_dev, work_bytes, need))) return rc;
  AMDR_HIP(hipSetDevice(bm25->device));
  const CsItems S{(const long long*)item_ptr_dev, item_slots_dev, item_kind_dev, item_dist_dev};
  const CsOut o{(long long*)list_ptr_dev, docs_dev, out_status_dev};
  return cs_launch(cs_index(bm25, (const long long*)list_ptr_dev, docs_dev, (const long long*)cls_ptr_dev, cls_terms_dev, n_cls,
                            cls_first),
                   S, n_items, n_before, cand_max, rows_cap, o, static_cast<unsigned char*>(work_dev), (hipStream_t)stream);
}

int amdr_class_spans(amdr_bm25_t* bm25, const int64_t* item_ptr, const int32_t* item_slots, const int32_t* item_kind,
                     const int32_t* item_dist, int64_t n_items, const int64_t* cls_ptr, const int32_t* cls_terms, int64_t n_cls,
                     int64_t cand_max, int64_t rows_cap, int64_t* out_list_ptr, int32_t* out_docs, int32_t* out_status) {
  static const char* const who = "class_spans";
  AMDR_REQUIRE(bm25 != nullptr, "%s: null handle", who);
  AMDR_REQUIRE(out_list_ptr != nullptr, "%s: null out_list_ptr", who);
  AMDR_REQUIRE(n_items <= 0 || out_status, "%s: null out_status", who);
  AMDR_REQUIRE(rows_cap <= 0 || out_docs, "%s: null out_docs", who);
  std::lock_guard<std::mutex> g(bm25->mu);
  long long cells = 0;
  int rc = cs_check_sizes(who, n_items, n_cls, 0, n_cls, cand_max, rows_cap, &cells);
  if (rc) return rc;
  if ((rc = bm_require_tokens(bm25, who))) return rc;
  const int64_t V = bm25->ix.n_terms, n_docs = bm25->ix.n_docs;
  const int bad = cs_validate(item_ptr, item_slots, item_kind, item_dist, n_items, cls_ptr, cls_terms, n_cls, V);
  AMDR_REQUIRE(bad == kPhValid, "%s: %s", who, cs_error_text(bad));
  if (n_items == 0) {
    out_list_ptr[0] = 0;
    return AMDR_OK;
  }
  AMDR_HIP(hipSetDevice(bm25->device));
  // The capacity of the classes' lists: per class min(n_docs, the sum of its known members' document frequencies).
  int64_t cls_cap = 0;
  const size_t n_members = n_cls ? (size_t)cls_ptr[n_cls] : 0;
  if (n_members) {
    std::unique_ptr<long long[]> tp(new (std::nothrow) long long[(size_t)V + 1]);
    if (!tp) return fail(AMDR_ENOMEM, "%s: no host memory for %lld list pointers", who, (long long)V + 1);
    AMDR_HIP(hipMemcpy(tp.get(), bm25->ix.term_ptr, ((size_t)V + 1) * sizeof(long long), hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < n_cls; ++c) {
      int64_t sum = 0;
      for (int64_t j = cls_ptr[c]; j < cls_ptr[c + 1] && sum < n_docs; ++j)
        if (cls_terms[j] >= 0 && cls_terms[j] < V) sum += tp[cls_terms[j] + 1] - tp[cls_terms[j]];
      cls_cap += sum < n_docs ? sum : n_docs;
    }
  }
  int64_t un_bytes = 0;
  if ((rc = amdr_union_lists_plan(n_cls, n_docs, &un_bytes))) return rc;
  const int64_t cap = cls_cap + rows_cap, n_lists = n_cls + n_items;
  // The staging buffer: the item arrays, the class arrays, the outputs of both steps (one list array), the union step's
  // workspace, this step's.
  ListStage s;
  const size_t a_ptr = s.add((size_t)(n_items + 1) * 8, item_ptr), a_slots = s.add((size_t)item_ptr[n_items] * 4, item_slots);
  const size_t a_kind = s.add((size_t)n_items * 4, item_kind), a_dist = s.add((size_t)n_items * 4, item_dist);
  const size_t a_cls_ptr = s.add((size_t)(n_cls + 1) * 8, n_cls ? cls_ptr : nullptr);
  const size_t a_cls_terms = s.add(n_members * 4, cls_terms);
  const size_t a_list_ptr = s.add((size_t)(n_lists + 1) * 8), a_docs = s.add((size_t)cap * 4);
  const size_t a_status = s.add((size_t)n_lists * 4);
  const size_t a_un_work = s.add((size_t)un_bytes), a_work = s.add(list_work((size_t)cells, kCsCellBytes).total);
  if ((rc = s.upload(bm25))) return rc;
  hipStream_t st = bm25->stream;
  long long* lp = s.at<long long>(a_list_ptr);
  int* docs = s.at<int>(a_docs);
  int* status = s.at<int>(a_status);
  // the classes' lists first (n_cls = 0: the union step writes list_ptr[0] = 0), the spans' behind them
  if ((rc = amdr_union_lists_device(bm25, s.at<int64_t>(a_cls_ptr), s.at<int32_t>(a_cls_terms), n_cls, 0, cap, (int64_t*)lp, docs,
                                    status, s.at<void>(a_un_work), un_bytes, st)))
    return rc;
  const CsItems S{s.at<long long>(a_ptr), s.at<int>(a_slots), s.at<int>(a_kind), s.at<int>(a_dist)};
  const CsOut o{lp, docs, status + n_cls};
  if ((rc = cs_launch(cs_index(bm25, lp, docs, s.at<long long>(a_cls_ptr), s.at<int>(a_cls_terms), n_cls, 0), S, n_items, n_cls,
                      cand_max, cap, o, s.at<unsigned char>(a_work), st)))
    return rc;
  std::unique_ptr<long long[]> got(new (std::nothrow) long long[(size_t)n_lists + 1]);
  if (!got) return fail(AMDR_ENOMEM, "%s: no host memory for %lld list pointers", who, (long long)n_lists + 1);
  if ((rc = list_fetch_heads(st, lp, n_lists + 1, got.get(), o.status, n_items, out_status))) return rc;
  // The classes' lists fit by construction and usually end below cls_cap, which leaves the spans more room than rows_cap:
  // the caller's capacity is applied here, with the write pass's own clamp and status.
  const long long first = got[n_cls];
  for (int64_t p = 0; p < n_items; ++p)
    if (un_status(got[n_cls + p] - first, got[n_cls + p + 1] - first, rows_cap) != kTsOk) out_status[p] = kTsRowsOverflow;
  for (int64_t p = 0; p <= n_items; ++p) out_list_ptr[p] = un_clamp(got[n_cls + p] - first, rows_cap);
  // (<= rows_cap: only the documents the lists name come back)
  return list_fetch_rows(st, docs + first, 4, out_list_ptr[n_items], out_docs);
}

}  // extern "C"

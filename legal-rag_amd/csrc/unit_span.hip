// Unit spans: the same-sentence and same-paragraph connectors (buyer /s seller, buyer +p seller) resolved into ascending
// document lists on the device, and the break flags they read (amdr_bm25_set_breaks: one byte per token of the resident
// stream, bit 0 a sentence start, bit 1 a paragraph start).
//
// No reference counterpart: the reference's BM25 channel scores bags of words (legalrag/retrieval/bm25_retriever.py:74-75)
// and has neither token order nor a filter.  An item's SLOTS name token classes exactly as a class span's do
// (class_span_rule.hpp: a plain token, or a class whose member ids are a union item and whose document list the union step
// has already written into the call's list array); the item is resolved from the resident token stream and its break
// flags into ITS OWN ascending document list, appended to that same array BEHIND the class spans', which
// amdr_term_scope_lists reads as one more term.
//
// The three launches of list_step.hpp, no global atomics, deterministic, nothing allocated; the grid is ONE-dimensional,
// n_items x tiles blocks of kPhTile = 256 threads, cell = p * tiles + y, as class_span.hip's:
//   count   the block resolves the item's slots into LDS, one thread links equal slots, finds the driver and the item's
//           shape (us_shape).  (1) thread t tests the conjunction for candidate t.  (2) one WAVE walks one survivor, 64
//           tokens per round: each lane reads its token (4 B) and its break byte (1 B), both coalesced, turns the token once
//           into the mask of the slots it fills (cs_token_mask) and the wave forms the ballots of the unit starts and of
//           every slot; us_round decides the round in wave-uniform arithmetic and carries the open unit's state into the
//           next round.  No halo, no staged re-reads, no LDS traffic in the walk.  A wave vote (the ballots are uniform:
//           the rule's result is) ends the document at the first unit that holds the item.
//   scan    compact_scan_i64_kernel over the counts.
//   write   kept candidate -> docs[start + offsets[cell] + rank]; positions >= rows_cap are dropped and their items get
//           status[p] = 2; the block of tile 0 writes the item's list_ptr entry, clamped to rows_cap.
// One list array, continued as class_span.hip continues it: list_ptr has n_before + n_items + 1 entries of which the first
// n_before + 1 are written, the classes' lists among them.
// LDS: the slots (8 x 56 B), the driver, the shape, the survivor list (512 B), the keep flags (256 B) and the scan's wave
// sums: about 1.3 KiB.  Workspace per cell: two i64 and 1 KiB of parked ranks.
// Algorithmic traffic of the walk: 5 B per token of a surviving document, read once.
#include "list_step.hpp"
#include "union_rule.hpp"
#include "unit_span_rule.hpp"

#include <memory>
#include <mutex>
#include <new>

using namespace amdr;

namespace {

constexpr int kUsThreads = kPhTile;
constexpr int kUsWaves = kUsThreads / 64;
static_assert(kUsThreads % 64 == 0, "whole waves");

// Workspace (list_work): a cell's payload is rank-or-minus-one i32 [256]
constexpr size_t kUsCellBytes = kUsThreads * sizeof(int);

struct UsItems {
  const long long* ptr;  // [n + 1]
  const int* slots;      // [ptr[n]]
  const int* kind;       // [n] UsKind bits
};

// The block's item: its slots resolved into LDS by the first L threads (an item the rule does not define reads none),
// linked and given a driver and a shape by thread 0; ends with a barrier.  Returns the item's length, 0 for an undefined
// item.
__device__ __forceinline__ int us_block_item(const CsIndex& I, const UsItems& S, long long p, CsSlot* slots, CsDriver* drv,
                                             UsShape* shape, int* kind_out) {
  const long long b = S.ptr[p], L = S.ptr[p + 1] - b;
  const int kind = S.kind[p];
  const bool sized = us_sized(kind, L);  // block-uniform
  if (sized && threadIdx.x < L) slots[threadIdx.x] = cs_slot(I, S.slots[b + threadIdx.x]);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (sized) cs_link_slots(slots, (int)L);
    *drv = sized ? cs_driver(slots, (int)L) : CsDriver{-1, nullptr, 0, 0};
    if (shape) *shape = us_shape(slots, sized ? (int)L : 0, kind);
  }
  __syncthreads();
  *kind_out = kind;
  return sized ? (int)L : 0;
}

__global__ __launch_bounds__(kUsThreads) void unit_span_count_kernel(CsIndex I, const unsigned char* __restrict__ brk, UsItems S,
                                                                    long long tiles, long long cand_max,
                                                                    long long* __restrict__ counts, int* __restrict__ rank_out,
                                                                    int* __restrict__ status) {
  __shared__ CsSlot slots[kUsMaxSlots];
  __shared__ CsDriver drv;
  __shared__ UsShape shape_s;
  __shared__ unsigned short surv[kUsThreads];
  __shared__ unsigned char kept[kUsThreads];
  __shared__ int wsum[kUsWaves + 1];
  const long long cell = blockIdx.x;
  const long long p = cell / tiles, tile = cell - p * tiles;
  int kind;
  const int L = us_block_item(I, S, p, slots, &drv, &shape_s, &kind);
  const CsDriver D = drv;
  const bool over = D.len > cand_max;
  if (tile == 0 && threadIdx.x == 0) status[p] = over ? kTsCandOverflow : kTsOk;
  const long long i0 = tile * kPhTile;
  if (over || D.at < 0 || i0 >= D.len) {  // block-uniform
    if (threadIdx.x == 0) counts[cell] = 0;
    return;
  }
  // phase 1: the conjunction, one candidate per thread (a document id outside the index is no candidate)
  const long long i = i0 + threadIdx.x;
  const long long cand = i < D.len ? D.docs[D.begin + i] : -1;
  const bool all = cand >= 0 && cand < I.ph.n_docs && cs_has_all(slots, L, D, cand);
  const int n_surv = list_compact_survivors<kUsThreads>(all, surv, kept, wsum);  // (barriers: every thread is here)
  // phase 2: one wave per survivor (n_surv is block-uniform; the loop holds no barrier)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const UsShape shape = shape_s;
  const int bit = us_break_bit(kind);
  for (int s = wave; s < n_surv; s += kUsWaves) {
    const int t = surv[s];
    const long long doc = D.docs[D.begin + i0 + t];
    const long long beg = I.ph.doc_ptr[doc], end = I.ph.doc_ptr[doc + 1];
    UsCarry carry = us_carry_clear();
    bool found = false;
    for (long long base = beg; base < end && !found; base += kPhLanes) {  // wave-uniform
      const int len = end - base < kPhLanes ? (int)(end - base) : kPhLanes;
      const bool in = lane < len;
      const int x = in ? I.ph.tokens[base + lane] : -1;
      const int f = in ? brk[base + lane] : 0;
      const unsigned m = in ? cs_token_mask(x, slots, L, I.cls_terms) : 0u;
      unsigned long long starts = __ballot(in && (f & bit));
      if (base == beg) starts |= 1ull;  // the document's first token begins a unit whatever its byte says
      unsigned long long B[kUsMaxSlots];
#pragma unroll
      for (int j = 0; j < kUsMaxSlots; ++j) B[j] = j < L ? __ballot((m >> j) & 1u) : 0ull;
      found = us_round(shape, B, starts, len, carry);  // wave-uniform operands, a wave-uniform result
    }
    if (lane == 0) kept[t] = found ? 1 : 0;
  }
  list_rank_and_park<kUsThreads>(kept, wsum, rank_out + (size_t)cell * kUsThreads, counts + cell);  // (barriers: as above)
}

// (list_ptr and docs are the array the class lists are read from: neither is __restrict__)
__global__ __launch_bounds__(kUsThreads) void unit_span_write_kernel(CsIndex I, UsItems S, long long tiles, long long cand_max,
                                                                    long long n_before, long long rows_cap,
                                                                    const long long* __restrict__ offsets,
                                                                    const int* __restrict__ rank_in, long long* list_ptr, int* docs,
                                                                    int* __restrict__ status) {
  __shared__ CsSlot slots[kUsMaxSlots];
  __shared__ CsDriver drv;
  const long long cell = blockIdx.x;
  const long long p = cell / tiles, tile = cell - p * tiles;
  const long long start = list_start(list_ptr, n_before);
  if (tile == 0 && threadIdx.x == 0) {
    const int s = list_write_header(list_ptr, n_before, p, start + offsets[p * tiles], start + offsets[(p + 1) * tiles], rows_cap);
    if (s != kTsOk) status[p] = s;  // (an item over cand_max has no row: its 1 stays)
  }
  int kind;
  (void)us_block_item(I, S, p, slots, &drv, nullptr, &kind);
  const CsDriver D = drv;
  const long long i0 = tile * kPhTile;
  if (D.len > cand_max || D.at < 0 || i0 >= D.len) return;  // block-uniform
  const long long at = list_kept_at(rank_in + (size_t)cell * kUsThreads, offsets, (size_t)cell, start, rows_cap);
  if (at >= 0) docs[at] = D.docs[D.begin + i0 + threadIdx.x];  // (a kept candidate lies inside the driver)
}

struct UsOut {
  long long* list_ptr;
  int* docs;
  int* status;
};

int us_launch(const CsIndex& I, const unsigned char* brk, const UsItems& S, int64_t n_items, int64_t n_before, int64_t cand_max,
              int64_t rows_cap, const UsOut& o, unsigned char* work, hipStream_t st) {
  const long long tiles = ph_tiles(cand_max), cells = (long long)n_items * tiles;
  const dim3 grid((unsigned)cells);
  return list_launch(
      st, n_items, n_before, (size_t)cells, kUsCellBytes, o.list_ptr, work,
      [&](long long* counts, unsigned char* rank) {
        hipLaunchKernelGGL(unit_span_count_kernel, grid, dim3(kUsThreads), 0, st, I, brk, S, tiles, (long long)cand_max, counts,
                           (int*)rank, o.status);
      },
      [&](const long long* offsets, const unsigned char* rank) {
        hipLaunchKernelGGL(unit_span_write_kernel, grid, dim3(kUsThreads), 0, st, I, S, tiles, (long long)cand_max,
                           (long long)n_before, (long long)rows_cap, offsets, (const int*)rank, o.list_ptr, o.docs, o.status);
      });
}

// sizes every entry point refuses (nothing is enqueued); *cells: the cells of the launch
int us_check_sizes(const char* who, int64_t n_items, int64_t n_cls, int64_t cls_first, int64_t n_before, int64_t cand_max,
                   int64_t rows_cap, long long* cells) {
  AMDR_REQUIRE(n_items >= 0 && n_cls >= 0 && cls_first >= 0 && n_before >= 0 && cand_max >= 0 && rows_cap >= 0,
               "%s: a negative size", who);
  AMDR_REQUIRE(cls_first <= n_before && n_cls <= n_before - cls_first, "%s: the classes' lists %lld .. %lld do not lie among the "
               "%lld lists written before", who, (long long)cls_first, (long long)cls_first + (long long)n_cls, (long long)n_before);
  AMDR_REQUIRE(cs_cells(n_items, cand_max, cells), "%s: %lld items x %lld tiles of %d candidates are more than the %lld cells of "
               "one launch", who, (long long)n_items, ph_tiles(cand_max), kPhTile, kCsMaxCells);
  return AMDR_OK;
}

// What a unit step asks of the handle beyond the token stream (under h->mu where the call takes it).
int us_require_breaks(const amdr_bm25* h, const char* who) {
  if (int rc = bm_require_tokens(h, who)) return rc;
  AMDR_REQUIRE(h->has_breaks, "%s: no break flags are resident (amdr_bm25_set_breaks; amdr_bm25_set_tokens and every update "
               "drop them)", who);
  return AMDR_OK;
}

CsIndex us_index(const amdr_bm25* h, const long long* x_ptr, const int* x_doc, const long long* cls_ptr, const int* cls_terms,
                 int64_t n_cls, int64_t cls_first) {
  return CsIndex{ph_index(h), x_ptr, x_doc, cls_ptr, cls_terms, (long)n_cls, (long)cls_first};
}

}  // namespace

extern "C" {

int amdr_bm25_set_breaks(amdr_bm25_t* h, const uint8_t* brk, int64_t n_tokens) {
  static const char* const who = "bm25_set_breaks";
  AMDR_REQUIRE(h != nullptr, "%s: null handle", who);
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc = bm_require_tokens(h, who)) return rc;
  AMDR_REQUIRE(n_tokens == h->n_tokens, "%s: %lld flags for a stream of %lld tokens", who, (long long)n_tokens,
               (long long)h->n_tokens);
  AMDR_REQUIRE(n_tokens == 0 || brk != nullptr, "%s: null array", who);
  for (int64_t i = 0; i < n_tokens; ++i)
    AMDR_REQUIRE(us_break_valid(brk[i]), "%s: flag %d at token %lld (0, 1 a sentence start, 3 a paragraph start)", who, (int)brk[i],
                 (long long)i);
  AMDR_HIP(hipSetDevice(h->device));
  unsigned char* nb = nullptr;
  int rc = dev_alloc(&nb, (size_t)n_tokens + 1, who);  // (+ 1: never an empty allocation)
  if (!rc && n_tokens && hipMemcpy(nb, brk, (size_t)n_tokens, hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(AMDR_EHIP, "%s: the upload failed: %s", who, hipGetErrorString(hipGetLastError()));
  if (rc) {  // the handle keeps what it had
    if (nb) (void)hipFree(nb);
    return rc;
  }
  h->drop_breaks();
  h->brk = nb, h->has_breaks = true;
  return AMDR_OK;
}

int amdr_bm25_breaks_info(amdr_bm25_t* h, int64_t* out2) {
  AMDR_REQUIRE(h && out2, "bm25_breaks_info: null");
  std::lock_guard<std::mutex> g(h->mu);
  out2[0] = h->has_breaks ? 1 : 0;
  out2[1] = h->has_breaks ? h->n_tokens : 0;
  return AMDR_OK;
}

int amdr_bm25_read_breaks(amdr_bm25_t* h, uint8_t* out) {
  static const char* const who = "bm25_read_breaks";
  AMDR_REQUIRE(h != nullptr, "%s: null handle", who);
  std::lock_guard<std::mutex> g(h->mu);
  if (int rc = us_require_breaks(h, who)) return rc;
  AMDR_REQUIRE(h->n_tokens == 0 || out != nullptr, "%s: null array", who);
  AMDR_HIP(hipSetDevice(h->device));
  if (h->n_tokens) AMDR_HIP(hipMemcpy(out, h->brk, (size_t)h->n_tokens, hipMemcpyDeviceToHost));
  return AMDR_OK;
}

int amdr_unit_spans_plan(int64_t n_items, int64_t cand_max, int64_t* work_bytes) {
  AMDR_REQUIRE(work_bytes != nullptr, "unit_spans_plan: null");
  long long cells = 0;
  int rc = us_check_sizes("unit_spans_plan", n_items, 0, 0, 0, cand_max, 0, &cells);
  if (rc) return rc;
  *work_bytes = (int64_t)list_work((size_t)cells, kUsCellBytes).total;
  return AMDR_OK;
}

int amdr_unit_spans_device(amdr_bm25_t* bm25, const int64_t* item_ptr_dev, const int32_t* item_slots_dev,
                           const int32_t* item_kind_dev, int64_t n_items, const int64_t* cls_ptr_dev, const int32_t* cls_terms_dev,
                           int64_t n_cls, int64_t cls_first, int64_t n_before, int64_t cand_max, int64_t rows_cap,
                           int64_t* list_ptr_dev, int32_t* docs_dev, int32_t* out_status_dev, void* work_dev, int64_t work_bytes,
                           void* stream) {
  static const char* const who = "unit_spans";
  AMDR_REQUIRE(bm25 != nullptr, "%s: null handle", who);
  long long cells = 0;
  int rc = us_check_sizes(who, n_items, n_cls, cls_first, n_before, cand_max, rows_cap, &cells);
  if (rc) return rc;
  if ((rc = us_require_breaks(bm25, who))) return rc;
  AMDR_REQUIRE(list_ptr_dev != nullptr, "%s: null list_ptr", who);
  AMDR_REQUIRE(n_items == 0 || (item_ptr_dev && item_slots_dev && item_kind_dev && out_status_dev), "%s: null operand", who);
  AMDR_REQUIRE(n_cls == 0 || (cls_ptr_dev && cls_terms_dev), "%s: null class arrays", who);
  AMDR_REQUIRE(rows_cap == 0 || docs_dev, "%s: null docs", who);
  const size_t need = n_items ? list_work((size_t)cells, kUsCellBytes).total : 0;
  if ((rc = list_check_work(who, work_dev, work_bytes, need))) return rc;
  AMDR_HIP(hipSetDevice(bm25->device));
  const UsItems S{(const long long*)item_ptr_dev, item_slots_dev, item_kind_dev};
  const UsOut o{(long long*)list_ptr_dev, docs_dev, out_status_dev};
  return us_launch(us_index(bm25, (const long long*)list_ptr_dev, docs_dev, (const long long*)cls_ptr_dev, cls_terms_dev, n_cls,
                            cls_first),
                   bm25->brk, S, n_items, n_before, cand_max, rows_cap, o, static_cast<unsigned char*>(work_dev),
                   (hipStream_t)stream);
}

int amdr_unit_spans(amdr_bm25_t* bm25, const int64_t* item_ptr, const int32_t* item_slots, const int32_t* item_kind,
                    int64_t n_items, const int64_t* cls_ptr, const int32_t* cls_terms, int64_t n_cls, int64_t cand_max,
                    int64_t rows_cap, int64_t* out_list_ptr, int32_t* out_docs, int32_t* out_status) {
  static const char* const who = "unit_spans";
  AMDR_REQUIRE(bm25 != nullptr, "%s: null handle", who);
  AMDR_REQUIRE(out_list_ptr != nullptr, "%s: null out_list_ptr", who);
  AMDR_REQUIRE(n_items <= 0 || out_status, "%s: null out_status", who);
  AMDR_REQUIRE(rows_cap <= 0 || out_docs, "%s: null out_docs", who);
  std::lock_guard<std::mutex> g(bm25->mu);
  long long cells = 0;
  int rc = us_check_sizes(who, n_items, n_cls, 0, n_cls, cand_max, rows_cap, &cells);
  if (rc) return rc;
  if ((rc = us_require_breaks(bm25, who))) return rc;
  const int64_t V = bm25->ix.n_terms, n_docs = bm25->ix.n_docs;
  const int bad = us_validate(item_ptr, item_slots, item_kind, n_items, cls_ptr, cls_terms, n_cls, V);
  AMDR_REQUIRE(bad == kPhValid, "%s: %s", who, us_error_text(bad));
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
  const size_t a_kind = s.add((size_t)n_items * 4, item_kind);
  const size_t a_cls_ptr = s.add((size_t)(n_cls + 1) * 8, n_cls ? cls_ptr : nullptr);
  const size_t a_cls_terms = s.add(n_members * 4, cls_terms);
  const size_t a_list_ptr = s.add((size_t)(n_lists + 1) * 8), a_docs = s.add((size_t)cap * 4);
  const size_t a_status = s.add((size_t)n_lists * 4);
  const size_t a_un_work = s.add((size_t)un_bytes), a_work = s.add(list_work((size_t)cells, kUsCellBytes).total);
  if ((rc = s.upload(bm25))) return rc;
  hipStream_t st = bm25->stream;
  long long* lp = s.at<long long>(a_list_ptr);
  int* docs = s.at<int>(a_docs);
  int* status = s.at<int>(a_status);
  // the classes' lists first (n_cls = 0: the union step writes list_ptr[0] = 0), the unit spans' behind them
  if ((rc = amdr_union_lists_device(bm25, s.at<int64_t>(a_cls_ptr), s.at<int32_t>(a_cls_terms), n_cls, 0, cap, (int64_t*)lp, docs,
                                    status, s.at<void>(a_un_work), un_bytes, st)))
    return rc;
  const UsItems S{s.at<long long>(a_ptr), s.at<int>(a_slots), s.at<int>(a_kind)};
  const UsOut o{lp, docs, status + n_cls};
  if ((rc = us_launch(us_index(bm25, lp, docs, s.at<long long>(a_cls_ptr), s.at<int>(a_cls_terms), n_cls, 0), bm25->brk, S, n_items,
                      n_cls, cand_max, cap, o, s.at<unsigned char>(a_work), st)))
    return rc;
  std::unique_ptr<long long[]> got(new (std::nothrow) long long[(size_t)n_lists + 1]);
  if (!got) return fail(AMDR_ENOMEM, "%s: no host memory for %lld list pointers", who, (long long)n_lists + 1);
  if ((rc = list_fetch_heads(st, lp, n_lists + 1, got.get(), o.status, n_items, out_status))) return rc;
  // The classes' lists fit by construction and usually end below cls_cap, which leaves the items more room than rows_cap:
  // the caller's capacity is applied here, with the write pass's own clamp and status.
  const long long first = got[n_cls];
  for (int64_t p = 0; p < n_items; ++p)
    if (un_status(got[n_cls + p] - first, got[n_cls + p + 1] - first, rows_cap) != kTsOk) out_status[p] = kTsRowsOverflow;
  for (int64_t p = 0; p <= n_items; ++p) out_list_ptr[p] = un_clamp(got[n_cls + p] - first, rows_cap);
  // (<= rows_cap: only the documents the lists name come back)
  return list_fetch_rows(st, docs + first, 4, out_list_ptr[n_items], out_docs);
}

}  // extern "C"

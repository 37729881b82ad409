// Vocabulary patterns: Wildcard (s?ll*, *ee) and Fuzzy (warrenty within one edit) resolved into the term ids they name by
// a scan of the resident vocabulary on the device.
//
// No reference counterpart: the reference's BM25 channel looks a query token up exactly
// (legalrag/retrieval/bm25_retriever.py:74-75) and has no pattern of any kind.  Beside it stands the host expansion of a
// Prefix (retrieval/terms.py prefix_tokens), a bisection that works because a prefix is a contiguous range of the sorted
// vocabulary; a wildcard or an edit-distance pattern has no such range and is a scan of every token.  The rule is
// vocab_match_rule.hpp.
//
// The handle (amdr_vocab_t) is a resident copy of the vocabulary as the tokeniser takes it — a UTF-8 blob and offsets,
// term i the token with id i — and the code-point count of every term, computed once at create.
//
// The three launches of the list resolvers (list_step.hpp), no global atomics, deterministic, nothing allocated; the
// grid is ONE-dimensional, n_pat x tiles blocks of kVmThreads threads, cell = p * tiles + y (pattern p, tile y of kVmTile
// term ids):
//   count   the block clears a bitmap of kVmTile bits in LDS and stages its pattern's code points in LDS once
//           (vm_stage); its threads stride over the tile's terms, apply the length pre-test, then the rule, and set bit
//           term - tile base with an LDS atomic OR — idempotent and independent of order.  After a barrier the block
//           counts the set bits into counts[cell] and PARKS the bitmap in the workspace, 1 KiB per cell.
//   scan    compact_scan_i64_kernel over the counts: every cell's offset.
//   write   thread t reads its kVmPer words of the parked bitmap, the block scans their bit counts, and the thread
//           expands its bits, ascending, into the pattern's row of the FIXED-STRIDE outputs ids [n_pat, item_cap] and
//           dist [n_pat, item_cap] at rank offsets[cell] - offsets[p * tiles] + rank in cell; a rank >= item_cap is
//           dropped.  The distance is computed again for the kept terms only.  The block of tile 0 writes n_match[p], the
//           TRUE count, and pads the row's tail with (-1, 255): every output byte is determined.
// Nothing needs clearing between calls: every word of counts, offsets and the parked bitmaps is written before it is read.
// Every barrier sits under a block-uniform condition: vm_stage and the scans are called by every thread, the term loop
// holds none, and nothing returns before the last one.
// LDS: the pattern (256 B), the bitmap (1 KiB, count only) and the scan's wave sums.
#include "common.hpp"
#include "compact.hpp"
#include "vocab_match_rule.hpp"

#include <mutex>
#include <vector>

using namespace amdr;

struct amdr_vocab {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  unsigned char* blob = nullptr;
  long long* offs = nullptr;
  int* cp_len = nullptr;
  long long n_terms = 0, bytes = 0;
  amdr::DevBuf stage;  // the host twin: the patterns, the outputs and the workspace
};

namespace {

constexpr int kVmWaves = kVmThreads / 64;
static_assert(kVmThreads % 64 == 0 && kVmThreads >= kVmMaxLen, "whole waves; one thread per code point of a pattern");

struct VmPats {  // the patterns as they lie on the device
  const unsigned* cp;
  const long long* ptr;
  const int* kind;
  const int* arg;
  long long cp_total;
};

// Pattern p into LDS (pat [kVmMaxLen]) and what the match needs to know of it.  Holds a barrier: EVERY thread of the
// block calls it.  A span outside the code-point array is not read: the pattern is staged with no code point and names
// nothing.
__device__ __forceinline__ VmPat vm_stage(const VmPats& A, long long p, unsigned* pat) {
  const long long b = A.ptr[p], e = A.ptr[p + 1];
  const int m = vm_span_ok(b, e, A.cp_total) ? (int)(e - b) : 0;
  if ((int)threadIdx.x < m) pat[threadIdx.x] = A.cp[b + threadIdx.x];
  __syncthreads();
  return vm_pattern_info(pat, m, A.kind[p], A.arg[p]);
}

__global__ __launch_bounds__(kVmThreads) void vm_count_kernel(VmVocab V, VmPats A, long long tiles, long long* __restrict__ counts,
                                                             unsigned* __restrict__ parked) {
  __shared__ unsigned pat[kVmMaxLen];
  __shared__ unsigned bits[kVmWords];
  __shared__ int wsum[kVmWaves + 1];
  const long long cell = blockIdx.x;
  const long long p = cell / tiles, tile = cell - p * tiles;
#pragma unroll
  for (int j = 0; j < kVmPer; ++j) bits[threadIdx.x * kVmPer + j] = 0u;
  const VmPat P = vm_stage(A, p, pat);  // (its barrier also publishes the cleared bitmap)
  if (P.ok) {                           // block-uniform; no barrier inside
    const long long base = tile * kVmTile;
    const long long end = base + kVmTile < V.n_terms ? base + kVmTile : V.n_terms;
    for (long long term = base + threadIdx.x; term < end; term += kVmThreads) {
      int dist;
      if (vm_term_match(V, pat, P, term, &dist)) atomicOr(&bits[vm_bit_word(term, tile) & (kVmWords - 1)], vm_bit_mask(term));
    }
  }
  __syncthreads();
  int mine = 0;
#pragma unroll
  for (int j = 0; j < kVmPer; ++j) {
    const unsigned w = bits[threadIdx.x * kVmPer + j];
    parked[(size_t)cell * kVmWords + threadIdx.x * kVmPer + j] = w;
    mine += vm_popcount(w);
  }
  int total;
  (void)compact_block_exclusive<kVmThreads, int>(mine, wsum, &total);
  if (threadIdx.x == 0) counts[cell] = total;
}

__global__ __launch_bounds__(kVmThreads) void vm_write_kernel(VmVocab V, VmPats A, long long tiles, long long item_cap,
                                                             const long long* __restrict__ offsets,
                                                             const unsigned* __restrict__ parked, int* __restrict__ ids,
                                                             unsigned char* __restrict__ dist, long long* __restrict__ n_match) {
  __shared__ unsigned pat[kVmMaxLen];
  __shared__ int wsum[kVmWaves + 1];
  const long long cell = blockIdx.x;
  const long long p = cell / tiles, tile = cell - p * tiles;
  const VmPat P = vm_stage(A, p, pat);
  int* ids_row = ids + (size_t)p * (size_t)item_cap;
  unsigned char* dist_row = dist + (size_t)p * (size_t)item_cap;
  const long long first = offsets[p * tiles];
  if (tile == 0) {  // the true count, and the tail of the row behind the kept matches
    const long long all = offsets[(p + 1) * tiles] - first;
    if (threadIdx.x == 0) n_match[p] = all;
    for (long long r = (all < 0 ? 0 : all) + threadIdx.x; r < item_cap; r += kVmThreads) ids_row[r] = -1, dist_row[r] = kVmNoDist;
  }
  unsigned word[kVmPer];
  int mine = 0;
#pragma unroll
  for (int j = 0; j < kVmPer; ++j) {
    word[j] = parked[(size_t)cell * kVmWords + threadIdx.x * kVmPer + j];
    mine += vm_popcount(word[j]);
  }
  int total;
  const int rank = compact_block_exclusive<kVmThreads, int>(mine, wsum, &total);
  long long at = offsets[cell] - first + rank;
#pragma unroll
  for (int j = 0; j < kVmPer; ++j)
    at += vm_expand_word(word[j], tile, (int)threadIdx.x * kVmPer + j, at, item_cap, V, pat, P, ids_row, dist_row);
}

struct VmOut {
  int* ids;
  unsigned char* dist;
  long long* n_match;
};

int vm_launch(const VmVocab& V, const VmPats& A, int64_t n_pat, long long cells, int64_t item_cap, const VmOut& o,
              unsigned char* work, hipStream_t st) {
  if (n_pat == 0) return AMDR_OK;
  const long long tiles = vm_tiles(V.n_terms);
  const VmWork w = vm_work(cells);
  long long* counts = reinterpret_cast<long long*>(work + w.off_counts);
  long long* offsets = reinterpret_cast<long long*>(work + w.off_offsets);
  unsigned* parked = reinterpret_cast<unsigned*>(work + w.off_parked);
  const dim3 grid((unsigned)cells);
  hipLaunchKernelGGL(vm_count_kernel, grid, dim3(kVmThreads), 0, st, V, A, tiles, counts, parked);
  AMDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(compact_scan_i64_kernel, dim3(1), dim3(kCompactScanThreads), 0, st, (const long long*)counts, (long)cells,
                     offsets);
  AMDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(vm_write_kernel, grid, dim3(kVmThreads), 0, st, V, A, tiles, (long long)item_cap, (const long long*)offsets,
                     (const unsigned*)parked, o.ids, o.dist, o.n_match);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

VmVocab vm_vocab(const amdr_vocab* h) { return VmVocab{h->blob, h->offs, h->cp_len, h->n_terms}; }

size_t vm_stage_align(size_t b) { return (size_t)vm_align((long long)b + 1); }  // (a region is never empty)

}  // namespace

extern "C" {

int amdr_vocab_create(const char* blob, const int64_t* offsets, int64_t n_terms, int32_t device, amdr_vocab_t** out) {
  static const char* const who = "vocab_create";
  AMDR_REQUIRE(out != nullptr, "%s: out is null", who);
  *out = nullptr;
  std::vector<int32_t> cp_len((size_t)(n_terms > 0 && n_terms <= 0x7fffffffLL ? n_terms : 0));
  const int bad = vm_validate_vocab(reinterpret_cast<const unsigned char*>(blob), offsets, n_terms, cp_len.data());
  AMDR_REQUIRE(bad == kVmValid, "%s: %s", who, vm_error_text(bad));
  if (int rc = check_device(device)) return rc;
  amdr_vocab* h = new amdr_vocab();
  h->device = device, h->n_terms = n_terms, h->bytes = offsets[n_terms];
  auto fail_with = [&](hipError_t e, const char* what) {
    amdr_vocab_destroy(h);
    return fail(e == hipErrorOutOfMemory ? AMDR_ENOMEM : AMDR_EHIP, "%s: %s failed: %s", who, what, hipGetErrorString(e));
  };
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return fail_with(e, "hipStreamCreate");
  if ((e = hipMalloc((void**)&h->blob, (size_t)h->bytes + 1)) != hipSuccess) return fail_with(e, "hipMalloc");
  if ((e = hipMalloc((void**)&h->offs, (size_t)(n_terms + 1) * 8)) != hipSuccess) return fail_with(e, "hipMalloc");
  if ((e = hipMalloc((void**)&h->cp_len, (size_t)(n_terms + 1) * 4)) != hipSuccess) return fail_with(e, "hipMalloc");
  if (h->bytes && (e = hipMemcpy(h->blob, blob, (size_t)h->bytes, hipMemcpyHostToDevice)) != hipSuccess) return fail_with(e, "hipMemcpy");
  if ((e = hipMemcpy(h->offs, offsets, (size_t)(n_terms + 1) * 8, hipMemcpyHostToDevice)) != hipSuccess) return fail_with(e, "hipMemcpy");
  if (n_terms && (e = hipMemcpy(h->cp_len, cp_len.data(), (size_t)n_terms * 4, hipMemcpyHostToDevice)) != hipSuccess)
    return fail_with(e, "hipMemcpy");
  *out = h;
  return AMDR_OK;
}

int amdr_vocab_destroy(amdr_vocab_t* h) {
  if (!h) return AMDR_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->blob) (void)hipFree(h->blob);
  if (h->offs) (void)hipFree(h->offs);
  if (h->cp_len) (void)hipFree(h->cp_len);
  h->stage.release();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return AMDR_OK;
}

int amdr_vocab_info(amdr_vocab_t* h, int64_t* out2) {
  AMDR_REQUIRE(h != nullptr && out2 != nullptr, "vocab_info: null");
  out2[0] = h->n_terms, out2[1] = h->bytes;
  return AMDR_OK;
}

int amdr_vocab_match_plan(int64_t n_terms, int64_t n_pat, int64_t* work_bytes) {
  static const char* const who = "vocab_match_plan";
  AMDR_REQUIRE(work_bytes != nullptr, "%s: null", who);
  AMDR_REQUIRE(n_terms >= 0 && n_pat >= 0, "%s: %s", who, vm_error_text(kVmSizes));
  AMDR_REQUIRE(n_terms <= 0x7fffffffLL, "%s: %s", who, vm_error_text(kVmTerms));
  long long cells = 0;
  AMDR_REQUIRE(vm_cells(n_pat, n_terms, &cells), "%s: %lld patterns x %lld tiles of %d terms: %s", who, (long long)n_pat,
               vm_tiles(n_terms), kVmTile, vm_error_text(kVmCells));
  *work_bytes = vm_work(cells).total;
  return AMDR_OK;
}

int amdr_vocab_match_device(amdr_vocab_t* h, const uint32_t* pat_cp_dev, const int64_t* pat_ptr_dev, const int32_t* pat_kind_dev,
                            const int32_t* pat_arg_dev, int64_t n_pat, int64_t cp_total, int32_t item_cap, int32_t* ids_dev,
                            uint8_t* dist_dev, int64_t* n_match_dev, void* work_dev, int64_t work_bytes, void* stream) {
  static const char* const who = "vocab_match";
  long long cells = 0;
  const int bad = vm_check_args(h, h ? h->n_terms : 0, pat_cp_dev, pat_ptr_dev, pat_kind_dev, pat_arg_dev, n_pat, cp_total,
                                item_cap, ids_dev, dist_dev, n_match_dev, &cells);
  AMDR_REQUIRE(bad == kVmValid, "%s: %s", who, vm_error_text(bad));
  const long long need = vm_work(cells).total;
  AMDR_REQUIRE(work_bytes >= need && (need == 0 || work_dev), "%s: a workspace of %lld bytes, the plan asks for %lld", who,
               (long long)work_bytes, need);
  AMDR_REQUIRE(((uintptr_t)work_dev & 7u) == 0, "%s: the workspace is not aligned to its int64 counts", who);
  const VmPats A{pat_cp_dev, (const long long*)pat_ptr_dev, pat_kind_dev, pat_arg_dev, (long long)cp_total};
  const VmOut o{ids_dev, dist_dev, (long long*)n_match_dev};
  return vm_launch(vm_vocab(h), A, n_pat, cells, item_cap, o, static_cast<unsigned char*>(work_dev), (hipStream_t)stream);
}

int amdr_vocab_match(amdr_vocab_t* h, const uint32_t* pat_cp, const int64_t* pat_ptr, const int32_t* pat_kind,
                     const int32_t* pat_arg, int64_t n_pat, int64_t cp_total, int32_t item_cap, int32_t* out_ids,
                     uint8_t* out_dist, int64_t* out_n_match) {
  static const char* const who = "vocab_match";
  long long cells = 0;
  int bad = vm_check_args(h, h ? h->n_terms : 0, pat_cp, pat_ptr, pat_kind, pat_arg, n_pat, cp_total, item_cap, out_ids,
                          out_dist, out_n_match, &cells);
  AMDR_REQUIRE(bad == kVmValid, "%s: %s", who, vm_error_text(bad));
  bad = vm_validate(pat_cp, pat_ptr, pat_kind, pat_arg, n_pat, cp_total);
  AMDR_REQUIRE(bad == kVmValid, "%s: %s", who, vm_error_text(bad));
  if (n_pat == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  // The staging buffer: the patterns, the outputs, the workspace — each region aligned and never empty.
  const size_t rows = (size_t)n_pat * (size_t)item_cap;
  const size_t sizes[8] = {(size_t)cp_total * 4, (size_t)(n_pat + 1) * 8, (size_t)n_pat * 4, (size_t)n_pat * 4,
                           rows * 4, rows, (size_t)n_pat * 8, (size_t)vm_work(cells).total};
  size_t off[9] = {0};
  for (int i = 0; i < 8; ++i) off[i + 1] = off[i] + vm_stage_align(sizes[i]);
  if (int rc = h->stage.ensure(off[8])) return rc;
  unsigned char* base = h->stage.as<unsigned char>();
  hipStream_t st = h->stream;
  const void* src[4] = {pat_cp, pat_ptr, pat_kind, pat_arg};
  for (int i = 0; i < 4; ++i)
    if (sizes[i]) AMDR_HIP(hipMemcpyAsync(base + off[i], src[i], sizes[i], hipMemcpyHostToDevice, st));
  const VmPats A{(const unsigned*)(base + off[0]), (const long long*)(base + off[1]), (const int*)(base + off[2]),
                 (const int*)(base + off[3]), (long long)cp_total};
  const VmOut o{(int*)(base + off[4]), base + off[5], (long long*)(base + off[6])};
  if (int rc = vm_launch(vm_vocab(h), A, n_pat, cells, item_cap, o, base + off[7], st)) return rc;
  void* dst[3] = {out_ids, out_dist, out_n_match};
  for (int i = 0; i < 3; ++i) AMDR_HIP(hipMemcpyAsync(dst[i], base + off[4 + i], sizes[4 + i], hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipStreamSynchronize(st));
  return AMDR_OK;
}

}  // extern "C"

// Facets: how the rows of each constraint of a scope table spread over the values of a chunk field — the counts behind
// "Article 2 – Sales: 61, Article 9 – Secured Transactions: 22" and the bare "109 articles match".
//
// No reference counterpart: the reference returns hits and counts nothing.  Here the result set of a constraint is the
// scope table amdr_term_scope*_device (or an upload) left on the device, and the rule is facet_rule.hpp's: per
// (constraint, field) the total, the rows without a value, the number of distinct values and the `top` most frequent codes
// by (count descending, code ascending).  All integers: deterministic whatever the order the adds arrive in.
//
// Three launches on the caller's stream, nothing allocated, capturable:
//   zero    facet_zero_kernel over the counters int32 [n_cons][sum of (n_codes + 1)] — inside the call, every time, so a
//           captured call may be replayed.  A kernel, not hipMemsetAsync: the memset NODE of a captured graph zeroed the
//           counters on the first replay only — from the second replay of the same executable graph on, the ROCm 7.2
//           runtime filled them with a stale 16-byte pattern (measured on the MI355X: DESIGN.md 4.23), on top of which
//           the two kernels then counted correctly.  A kernel node replays as it was captured.
//   count   grid (n_cons x tiles, n_fields): cell = blockIdx.x = p * tiles + y (constraint p, tile y of kFcTile rows of its
//           scope, the grid shape of the list resolvers), field = blockIdx.y <= 8.  A block whose tile starts past its
//           scope's end leaves at once.  The others read their rows once, coalesced (thread t takes rows t, t + 256, ...),
//           and gather each row's code.  A field of n_codes <= kFcBins is binned in LDS — int32 [n_codes + 1], the last bin
//           `missing`, LDS atomicAdd — and after a barrier only the NON-ZERO bins are added to the constraint's counters in
//           global memory: a constraint of many tiles costs each of its hot values one global atomic per tile, not one per
//           row.  A wider field adds straight to the global counters: its rows spread over more than kFcBins values, so
//           two rows seldom meet in a counter, and sweeping the field in windows of kFcBins codes would read the rows and
//           gather the codes ceil(n_codes / kFcBins) times to save atomics that do not collide.
//   select  one block per (constraint, field), blockIdx.x = p * n_fields + f.  Its waves sweep the n_codes counters, 64 per
//           step, push the keys (count, ~code) of the non-zero ones through WaveTopK (topk.hpp) and count them; the lists of
//           a block's waves are merged by block_combine_topk.  Wave 0 writes the list and its padding, lane 0 the rest; the
//           block of field 0 writes the constraint's total: the sum of its counters, `missing` included.
// A block is one wave when no field has more than 1 024 codes, four waves otherwise.
// Every barrier sits under a block-uniform condition.  LDS: count 16 388 B; select 1 KiB per wave and a few words.
#include "facet_rule.hpp"
#include "scope_handle.hpp"
#include "topk.hpp"

#include <mutex>

using namespace amdr;

static_assert(kFcTile == AMDR_FACET_TILE_ROWS && kFcBins == AMDR_FACET_LDS_BINS && kFcMaxTop == AMDR_FACET_MAX_TOP,
              "the header exports the rule's constants");

namespace {

constexpr int kFcCap = 128;  // a wave's staging list: a power of two >= top + 64
static_assert(kFcCap >= kFcMaxTop + 64, "one wave of appends always fits");
constexpr int kFcOneWaveCodes = 1024;  // the widest field one wave per (constraint, field) sweeps: 16 steps

struct FcOut {
  long long* total;    // [n_cons]
  long long* missing;  // [n_cons, n_fields]
  int* distinct;       // [n_cons, n_fields]
  int* code;           // [n_cons, n_fields, top]
  long long* count;    // [n_cons, n_fields, top]
};

constexpr int kFcZeroBlocks = 1024;  // at most: the threads stride over the rest

__global__ __launch_bounds__(kFcThreads) void facet_zero_kernel(int* __restrict__ counters, long long n) {
  for (long long i = (long long)blockIdx.x * kFcThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kFcThreads) counters[i] = 0;
}

__global__ __launch_bounds__(kFcThreads) void facet_count_kernel(const long long* __restrict__ scope_ptr,
                                                                const long long* __restrict__ rows, long long tiles,
                                                                long long rows_max, const int* __restrict__ codes,
                                                                long long n_rows, FcFields F, int* __restrict__ counters) {
  __shared__ int bins[kFcBins + 1];
  const long long cell = blockIdx.x;
  const long long p = cell / tiles, tile = cell - p * tiles;
  const int f = blockIdx.y;
  const long long b = scope_ptr[p];
  long long lo, hi;
  if (!fc_tile_range(scope_ptr[p + 1] - b, rows_max, tile, &lo, &hi)) return;  // block-uniform, before any barrier
  const long long nc = F.n_codes[f];
  int* __restrict__ mine = counters + (size_t)p * (size_t)F.stride + (size_t)F.off[f];
  const int* __restrict__ col = codes + (size_t)f * (size_t)n_rows;
  const bool in_lds = fc_in_lds(nc);  // block-uniform
  if (in_lds) {
    for (int i = threadIdx.x; i <= nc; i += kFcThreads) bins[i] = 0;
    __syncthreads();
  }
  for (long long i = lo + threadIdx.x; i < hi; i += kFcThreads) {
    const long long r = rows[b + i];
    if (!fc_row_ok(r, n_rows)) continue;  // never dereferenced, counted nowhere
    const long long bin = fc_bin(col[r], nc);
    if (in_lds)
      atomicAdd(&bins[bin], 1);
    else
      atomicAdd(&mine[bin], 1);
  }
  if (in_lds) {
    __syncthreads();
    for (int i = threadIdx.x; i <= nc; i += kFcThreads) {
      const int v = bins[i];
      if (v) atomicAdd(&mine[i], v);
    }
  }
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void facet_select_kernel(const int* __restrict__ counters, FcFields F, int top, FcOut o) {
  __shared__ C32 lists[WAVES * kFcCap];
  __shared__ int cnts[WAVES];
  __shared__ int w_distinct[WAVES];
  __shared__ int w_sum[WAVES];
  const long long pf = blockIdx.x;
  const long long p = pf / F.n_fields;
  const int f = (int)(pf - p * F.n_fields);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long nc = F.n_codes[f];
  const int* __restrict__ mine = counters + (size_t)p * (size_t)F.stride + (size_t)F.off[f];
  WaveTopK<C32> tk;
  tk.init(lists + wave * kFcCap, kFcCap, top);
  int distinct = 0, sum = 0;  // (a constraint's counters sum to at most n_rows < 2^31)
  for (long long base = (long long)wave * 64; base < nc; base += WAVES * 64) {  // wave-uniform
    const long long c = base + lane;
    const int n = c < nc ? mine[c] : 0;
    const bool has = n > 0;
    distinct += has ? 1 : 0, sum += n;
    C32 key;
    key.c = has ? fc_key(n, c) : 0ull;
    tk.push_lanes(key, has, lane);
  }
  tk.finalize(lane);
  distinct = wave_allsum_i32(distinct), sum = wave_allsum_i32(sum);
  if (lane == 0) w_distinct[wave] = distinct, w_sum[wave] = sum;
  block_combine_topk(tk, lists, kFcCap, WAVES, wave, lane, cnts);  // (its first barrier publishes the words above too)
  if (wave != 0) return;
  const unsigned long long* keys = reinterpret_cast<const unsigned long long*>(lists);
  for (int j = lane; j < top; j += 64) {
    o.code[(size_t)pf * top + j] = fc_slot_code(keys, tk.cnt, j);
    o.count[(size_t)pf * top + j] = fc_slot_count(keys, tk.cnt, j);
  }
  if (lane == 0) {
    long long all = 0;
    int d = 0;
    for (int w = 0; w < WAVES; ++w) d += w_distinct[w], all += w_sum[w];
    const long long missing = mine[nc];
    o.distinct[pf] = d, o.missing[pf] = missing;
    if (f == 0) o.total[p] = all + missing;
  }
}

int fc_launch(const long long* scope_ptr, const long long* rows, int64_t n_cons, int64_t rows_max, const int* codes,
              int64_t n_rows, const FcFields& F, long long cells, int top, const FcOut& o, int* counters, long long work_bytes,
              hipStream_t st) {
  if (n_cons == 0) return AMDR_OK;
  const long long n_counters = work_bytes / 4;
  const long long zero_blocks = (n_counters + kFcThreads - 1) / kFcThreads;
  hipLaunchKernelGGL(facet_zero_kernel, dim3((unsigned)(zero_blocks < kFcZeroBlocks ? zero_blocks : kFcZeroBlocks)), dim3(kFcThreads),
                     0, st, counters, n_counters);
  AMDR_HIP(hipGetLastError());
  const long long tiles = fc_tiles(rows_max, n_rows);
  hipLaunchKernelGGL(facet_count_kernel, dim3((unsigned)cells, (unsigned)F.n_fields), dim3(kFcThreads), 0, st, scope_ptr, rows,
                     tiles, (long long)fc_rows_max(rows_max, n_rows), codes, (long long)n_rows, F, counters);
  AMDR_HIP(hipGetLastError());
  long long widest = 0;
  for (int f = 0; f < F.n_fields; ++f) widest = F.n_codes[f] > widest ? F.n_codes[f] : widest;
  const dim3 grid((unsigned)(n_cons * F.n_fields));
  if (widest <= kFcOneWaveCodes)
    hipLaunchKernelGGL(facet_select_kernel<1>, grid, dim3(64), 0, st, (const int*)counters, F, top, o);
  else
    hipLaunchKernelGGL(facet_select_kernel<4>, grid, dim3(256), 0, st, (const int*)counters, F, top, o);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

constexpr size_t kFcAlign = 256;
size_t fc_align(size_t b) { return (b + kFcAlign - 1) / kFcAlign * kFcAlign; }

}  // namespace

extern "C" {

int amdr_facet_plan(int64_t n_cons, int32_t n_fields, const int64_t* n_codes, int64_t* work_bytes) {
  static const char* const who = "facet_plan";
  AMDR_REQUIRE(work_bytes != nullptr && n_codes != nullptr, "%s: null", who);
  FcFields F;
  AMDR_REQUIRE(fc_fields(n_fields, n_codes, &F), "%s: n_fields=%d outside 1 .. %d or an n_codes outside [0, 2^31)", who,
               (int)n_fields, kFcMaxFields);
  long long bytes = 0;
  AMDR_REQUIRE(fc_work_bytes(n_cons, F, &bytes), "%s: n_cons=%lld", who, (long long)n_cons);
  *work_bytes = bytes;
  return AMDR_OK;
}

int amdr_facet_counts_device(const int64_t* scope_ptr_dev, const int64_t* rows_dev, int64_t n_cons, int64_t rows_max,
                             const int32_t* codes_dev, int64_t n_rows, int32_t n_fields, const int64_t* n_codes, int32_t top,
                             int64_t* out_total_dev, int64_t* out_missing_dev, int32_t* out_distinct_dev,
                             int32_t* out_code_dev, int64_t* out_count_dev, void* work_dev, int64_t work_bytes, void* stream) {
  static const char* const who = "facet_counts";
  FcFields F;
  long long cells = 0, need = 0;
  const int bad = fc_check_args(scope_ptr_dev, rows_dev, n_cons, rows_max, codes_dev, n_rows, n_fields, n_codes, top,
                                out_total_dev, out_missing_dev, out_distinct_dev, out_code_dev, out_count_dev, &F, &cells);
  AMDR_REQUIRE(bad == kFcValid, "%s: %s", who, fc_error_text(bad));
  AMDR_REQUIRE(fc_work_bytes(n_cons, F, &need), "%s: the counters of %lld constraints do not fit", who, (long long)n_cons);
  AMDR_REQUIRE(work_bytes >= need && (need == 0 || work_dev), "%s: a workspace of %lld bytes, the plan asks for %lld", who,
               (long long)work_bytes, need);
  AMDR_REQUIRE(((uintptr_t)work_dev & 3u) == 0, "%s: the workspace is not aligned to its int32 counters", who);
  const FcOut o{(long long*)out_total_dev, (long long*)out_missing_dev, out_distinct_dev, out_code_dev, (long long*)out_count_dev};
  return fc_launch((const long long*)scope_ptr_dev, (const long long*)rows_dev, n_cons, rows_max, codes_dev, n_rows, F, cells,
                   top, o, static_cast<int*>(work_dev), need, (hipStream_t)stream);
}

int amdr_facet_counts(amdr_scope_t* h, const int64_t* scope_ptr, const int64_t* rows, int64_t n_cons, int64_t rows_max,
                      const int32_t* codes, int64_t n_rows, int32_t n_fields, const int64_t* n_codes, int32_t top,
                      int64_t* out_total, int64_t* out_missing, int32_t* out_distinct, int32_t* out_code, int64_t* out_count) {
  static const char* const who = "facet_counts";
  AMDR_REQUIRE(h != nullptr, "%s: null handle", who);
  FcFields F;
  long long cells = 0, need = 0;
  int bad = fc_check_args(scope_ptr, rows, n_cons, rows_max, codes, n_rows, n_fields, n_codes, top, out_total, out_missing,
                          out_distinct, out_code, out_count, &F, &cells);
  AMDR_REQUIRE(bad == kFcValid, "%s: %s", who, fc_error_text(bad));
  bad = fc_validate(scope_ptr, rows, n_cons, rows_max, n_rows);
  AMDR_REQUIRE(bad == kFcValid, "%s: %s", who, fc_error_text(bad));
  AMDR_REQUIRE(fc_work_bytes(n_cons, F, &need), "%s: the counters of %lld constraints do not fit", who, (long long)n_cons);
  if (n_cons == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  // The staging buffer: the table, the code columns, the outputs, the counters — each region aligned and never empty.
  const size_t cf = (size_t)n_cons * (size_t)n_fields;
  const size_t n_scope_rows = (size_t)scope_ptr[n_cons];
  const size_t sizes[9] = {(size_t)(n_cons + 1) * 8, n_scope_rows * 8, (size_t)n_fields * (size_t)n_rows * 4, (size_t)n_cons * 8,
                           cf * 8, cf * 4, cf * (size_t)top * 4, cf * (size_t)top * 8, (size_t)need};
  size_t off[10] = {0};
  for (int i = 0; i < 9; ++i) off[i + 1] = off[i] + fc_align(sizes[i] + 1);
  if (int rc = h->stage.ensure(off[9])) return rc;
  unsigned char* base = h->stage.as<unsigned char>();
  hipStream_t st = h->stream;
  const void* src[3] = {scope_ptr, rows, codes};
  for (int i = 0; i < 3; ++i)
    if (sizes[i]) AMDR_HIP(hipMemcpyAsync(base + off[i], src[i], sizes[i], hipMemcpyHostToDevice, st));
  const FcOut o{(long long*)(base + off[3]), (long long*)(base + off[4]), (int*)(base + off[5]), (int*)(base + off[6]),
                (long long*)(base + off[7])};
  if (int rc = fc_launch((const long long*)(base + off[0]), (const long long*)(base + off[1]), n_cons, rows_max,
                         (const int*)(base + off[2]), n_rows, F, cells, top, o, (int*)(base + off[8]), need, st))
    return rc;
  void* dst[5] = {out_total, out_missing, out_distinct, out_code, out_count};
  for (int i = 0; i < 5; ++i) AMDR_HIP(hipMemcpyAsync(dst[i], base + off[3 + i], sizes[3 + i], hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipStreamSynchronize(st));
  return AMDR_OK;
}

}  // extern "C"

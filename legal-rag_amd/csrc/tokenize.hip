// Query tokeniser + vocabulary lookup of the BM25 channel on the device: the CSR amdr_bm25_search_device takes, from
// the query texts as one UTF-8 blob in HBM (include/amdretrieval.h, amdr_tokenizer_encode_device).
//
// Replaces, as the host form in tokenize.cpp does, `tokens = list(jieba.cut(query))` + the term lookup of rank_bm25's
// get_scores (legalrag/retrieval/bm25_retriever.py:73-74) for text without Han characters.  The rule is
// tokenize_rule.hpp, the same source the host form compiles, and the vocabulary is a copy of a host amdr_tokenizer_t's
// open-addressing table: the output is amdr_tokenizer_encode's, byte for byte.  That holds for Han text too: the copy
// takes the host handle's Han mode (amdr_tokenizer_set_han) and, in the dictionary mode, its key table, and
// tok_count_kernel calls the same tokenize().  The table is read from HBM where it lies (a few hundred KB at most, so
// L2-resident); the route of a query (one double and one int32 per byte) lives in the query's own byte range of two more
// workspace arrays, so no lane holds an array sized by its query and nothing goes to scratch.
//
// Four launches, all enqueued on the caller's stream, no allocation (the workspace is sized by reserve):
//   1. tok_count_kernel   one lane per query, the block's bytes staged in LDS by coalesced loads (when they fit in
//                         32 KiB): cuts the query by the rule, writes its token spans into the query's own
//                         byte range of a span buffer (tokens <= bytes, so they always fit), its count into
//                         q_ptr[q + 1], its needs_segmenter flag, and the block's total count;
//   2. tok_scan_kernel    one block: exclusive scan of the block totals;
//   3. tok_place_kernel   one lane per query (same blocks as 1): the block's counts scanned on top of the block's
//                         offset -> q_ptr, and the query's spans copied to their place in a compacted span list;
//   4. tok_lookup_kernel  one lane per TOKEN: hash, probe, compare -> term id.  The lookups are dependent loads; a lane
//                         per token keeps tens of thousands of them in flight.
// Queries average ~60 bytes, so a lane per query in 1 and 3 is short serial work; one long query is correct (a lane
// walks it) but not fast.
//
// Offsets that are not ascending or run past n_bytes are clamped (q_ptr never exceeds n_bytes): such input gives
// unspecified term ids, never an access outside the buffers.
#include <mutex>
#include <new>

#include "common.hpp"
#include "tokenize_rule.hpp"

using namespace amdr;

struct amdr_tokenizer_device {
  int device = 0;
  int64_t n_terms = 0, n_slots = 0;
  uint32_t mask = 0;
  int32_t* slots = nullptr;        // [n_slots]: -1 empty, else a term id (the host table, slot for slot)
  int64_t* offs = nullptr;         // [n_terms + 1]: term i = blob[offs[i] .. offs[i + 1])
  unsigned char* blob = nullptr;   // the terms' bytes
  int32_t* single = nullptr;       // [256]: id of each one-byte term
  amdr_tok::HanRule han;           // the host handle's Han mode; its table pointers are the device copies below
  int32_t* han_slots = nullptr;
  int32_t* han_offs = nullptr;
  unsigned char* han_blob = nullptr;
  double* han_logw = nullptr;
  unsigned char* han_word = nullptr;
  int32_t nq_max = 0;
  int64_t bytes_max = -1;          // -1: reserve not called yet
  DevBuf spans, cspans, bsum;      // per-query span slots, compacted spans, block totals
  DevBuf route_v, route_x;         // dictionary mode: the route, per byte of text (double, int32)
  std::mutex mu;
};

namespace {

constexpr int kTokBlock = 256;  // queries per block of the per-query kernels
constexpr int kTokStage = 32768;  // LDS bytes of query text a block of tok_count_kernel stages (~2x its average range)

__device__ inline int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// inclusive scan of one value per lane over a 256-lane block (Hillis-Steele in LDS); returns the lane's inclusive sum
__device__ inline long long block_scan_incl(long long v, long long* s) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int off = 1; off < kTokBlock; off <<= 1) {
    const long long x = t >= off ? s[t - off] : 0;
    __syncthreads();
    s[t] += x;
    __syncthreads();
  }
  const long long r = s[t];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kTokBlock) void tok_count_kernel(const unsigned char* __restrict__ text,
                                                              const int64_t* __restrict__ offs, int nq, int64_t n_bytes,
                                                              uint2* __restrict__ spans, int64_t* __restrict__ q_ptr,
                                                              int32_t* __restrict__ flags, long long* __restrict__ bsum,
                                                              const amdr_tok::HanRule han, double* __restrict__ route_v,
                                                              int32_t* __restrict__ route_x) {
  __shared__ long long s[kTokBlock];
  __shared__ unsigned char stage[kTokStage];
  const int q = blockIdx.x * kTokBlock + threadIdx.x;
  // the block's queries are one byte range of the blob: staged into LDS by coalesced loads when it fits (a lane then
  // walks its query in LDS instead of issuing one global load per byte), else read where it lies
  const int q0 = blockIdx.x * kTokBlock, q1 = min(q0 + kTokBlock, nq);
  const int64_t blo = clamp64(offs[q0], 0, n_bytes), bhi = clamp64(offs[q1], blo, n_bytes);
  const bool staged = bhi - blo <= kTokStage;  // block-uniform
  if (staged) {
    const int nb = (int)(bhi - blo);
#pragma unroll 4
    for (int i = threadIdx.x; i < nb; i += kTokBlock) stage[i] = text[blo + i];
    __syncthreads();
  }
  long long c = 0;
  if (q < nq) {
    const int64_t lo = clamp64(offs[q], 0, n_bytes), hi = clamp64(offs[q + 1], lo, n_bytes);
    uint2* out = spans + lo;
    int n_tok = 0;
    auto emit = [&](int a, int b) { out[n_tok++] = make_uint2((unsigned)a, (unsigned)(b - a)); };
    // (offsets that are not ascending can leave a query outside the staged range: it is read from the blob)
    bool ok;
    if (staged && lo >= blo && hi <= bhi)
      ok = amdr_tok::tokenize(stage + (lo - blo), (int)(hi - lo), han, route_v + lo, route_x + lo, emit);
    else
      ok = amdr_tok::tokenize(text + lo, (int)(hi - lo), han, route_v + lo, route_x + lo, emit);
    flags[q] = ok ? 0 : 1;
    c = ok ? n_tok : 0;
    q_ptr[q + 1] = c;  // the count; tok_place_kernel turns it into the offset
  }
  const long long tot = block_scan_incl(c, s);
  if (threadIdx.x == kTokBlock - 1) bsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kTokBlock) void tok_scan_kernel(long long* __restrict__ bsum, int nb) {
  __shared__ long long s[kTokBlock];
  long long carry = 0;
  for (int base = 0; base < nb; base += kTokBlock) {
    const int i = base + threadIdx.x;
    const long long v = i < nb ? bsum[i] : 0;
    const long long incl = block_scan_incl(v, s);  // (s still holds the inclusive sums)
    const long long tile = s[kTokBlock - 1];
    __syncthreads();
    if (i < nb) bsum[i] = carry + incl - v;
    carry += tile;
  }
}

__global__ __launch_bounds__(kTokBlock) void tok_place_kernel(const int64_t* __restrict__ offs, int nq, int64_t n_bytes,
                                                              const uint2* __restrict__ spans, uint2* __restrict__ cspans,
                                                              int64_t* __restrict__ q_ptr,
                                                              const long long* __restrict__ bsum) {
  __shared__ long long s[kTokBlock];
  const int q = blockIdx.x * kTokBlock + threadIdx.x;
  const long long c = q < nq ? q_ptr[q + 1] : 0;
  const long long incl = block_scan_incl(c, s) + bsum[blockIdx.x];
  if (q >= nq) return;
  const int64_t end = incl < n_bytes ? incl : n_bytes;
  const int64_t beg = (incl - c) < n_bytes ? (incl - c) : n_bytes;
  q_ptr[q + 1] = end;
  if (q == 0) q_ptr[0] = 0;
  const int64_t lo = clamp64(offs[q], 0, n_bytes);
  for (int64_t j = 0; j < end - beg; ++j) {
    const uint2 sp = spans[lo + j];
    cspans[beg + j] = make_uint2((unsigned)(lo + sp.x), sp.y);  // absolute start (n_bytes < 2^31)
  }
}

__global__ __launch_bounds__(kTokBlock) void tok_lookup_kernel(const unsigned char* __restrict__ text, int nq,
                                                               const uint2* __restrict__ cspans,
                                                               const int64_t* __restrict__ q_ptr,
                                                               const int32_t* __restrict__ slots, int64_t n_slots,
                                                               uint32_t mask, const int64_t* __restrict__ voffs,
                                                               const unsigned char* __restrict__ vblob,
                                                               const int32_t* __restrict__ single,
                                                               int32_t* __restrict__ term_ids) {
  const int64_t total = q_ptr[nq];
  for (int64_t t = (int64_t)blockIdx.x * kTokBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kTokBlock) {
    const uint2 sp = cspans[t];
    const unsigned char* p = text + sp.x;
    const int n = (int)sp.y;
    int32_t id = -1;
    if (n == 1) {
      id = single[p[0]];
    } else if (n_slots > 0) {
      for (uint32_t i = amdr_tok::hash(p, n) & mask;; i = (i + 1) & mask) {
        const int32_t cand = slots[i];
        if (cand < 0) break;
        const int64_t lo = voffs[cand];
        if (voffs[cand + 1] - lo == n) {
          int k = 0;
          while (k < n && vblob[lo + k] == p[k]) ++k;
          if (k == n) {
            id = cand;
            break;
          }
        }
      }
    }
    term_ids[t] = id;
  }
}

template <class T>
int upload(T** dst, const T* src, size_t count) {
  *dst = nullptr;
  if (!count) return AMDR_OK;
  AMDR_HIP(hipMalloc((void**)dst, count * sizeof(T)));
  AMDR_HIP(hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
  return AMDR_OK;
}

}  // namespace

extern "C" {

int amdr_tokenizer_device_create(const amdr_tokenizer_t* host, int32_t device, amdr_tokenizer_device_t** out) {
  AMDR_REQUIRE(out != nullptr, "tokenizer_device_create: out is null");
  *out = nullptr;
  AMDR_REQUIRE(host != nullptr, "tokenizer_device_create: null host tokenizer");
  int rc = check_device(device);
  if (rc) return rc;
  amdr_tokenizer_device* h = new (std::nothrow) amdr_tokenizer_device();
  if (!h) return fail(AMDR_ENOMEM, "tokenizer_device_create: host alloc");
  h->device = device;
  h->n_terms = host->offs.empty() ? 0 : (int64_t)host->offs.size() - 1;
  h->n_slots = (int64_t)host->slots.size();
  h->mask = host->mask;
  rc = upload(&h->slots, host->slots.data(), host->slots.size());
  if (!rc) rc = upload(&h->offs, host->offs.data(), host->offs.size());
  if (!rc) rc = upload(&h->blob, reinterpret_cast<const unsigned char*>(host->blob.data()), host->blob.size());
  if (!rc) rc = upload(&h->single, host->single, 256);
  h->han = host->han;
  if (!rc) rc = upload(&h->han_slots, host->han_slots.data(), host->han_slots.size());
  if (!rc) rc = upload(&h->han_offs, host->han_offs.data(), host->han_offs.size());
  if (!rc) rc = upload(&h->han_blob, reinterpret_cast<const unsigned char*>(host->han_blob.data()), host->han_blob.size());
  if (!rc) rc = upload(&h->han_logw, host->han_logw.data(), host->han_logw.size());
  if (!rc) rc = upload(&h->han_word, host->han_word.data(), host->han_word.size());
  h->han.slots = h->han_slots;
  h->han.offs = h->han_offs;
  h->han.blob = h->han_blob;
  h->han.logw = h->han_logw;
  h->han.is_word = h->han_word;
  if (rc) {
    amdr_tokenizer_device_destroy(h);
    return rc;
  }
  *out = h;
  return AMDR_OK;
}

int amdr_tokenizer_device_reserve(amdr_tokenizer_device_t* h, int32_t nq_max, int64_t bytes_max) {
  AMDR_REQUIRE(h != nullptr, "tokenizer_device_reserve: null handle");
  AMDR_REQUIRE(nq_max >= 0 && bytes_max >= 0 && bytes_max < (1ll << 31), "tokenizer_device_reserve: bad sizes");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  const size_t nb = (size_t)(nq_max + kTokBlock - 1) / kTokBlock + 1;
  int rc = h->spans.ensure((size_t)(bytes_max + 1) * sizeof(uint2));
  if (!rc) rc = h->cspans.ensure((size_t)(bytes_max + 1) * sizeof(uint2));
  if (!rc) rc = h->bsum.ensure(nb * sizeof(long long));
  if (h->han.mode == AMDR_HAN_DICT) {
    if (!rc) rc = h->route_v.ensure((size_t)(bytes_max + 1) * sizeof(double));
    if (!rc) rc = h->route_x.ensure((size_t)(bytes_max + 1) * sizeof(int32_t));
  }
  if (rc) return rc;
  if (nq_max > h->nq_max) h->nq_max = nq_max;
  if (bytes_max > h->bytes_max) h->bytes_max = bytes_max;
  return AMDR_OK;
}

int amdr_tokenizer_encode_device(amdr_tokenizer_device_t* h, const char* text_dev, const int64_t* offs_dev, int32_t nq,
                                 int64_t n_bytes, int32_t* term_ids_dev, int64_t capacity, int64_t* q_ptr_dev,
                                 int32_t* needs_segmenter_dev, void* stream) {
  AMDR_REQUIRE(h != nullptr, "tokenizer_encode_device: null handle");
  AMDR_REQUIRE(nq >= 0 && n_bytes >= 0 && capacity >= 0, "tokenizer_encode_device: bad sizes");
  AMDR_REQUIRE(h->bytes_max >= 0, "tokenizer_encode_device: call amdr_tokenizer_device_reserve first");
  AMDR_REQUIRE(nq <= h->nq_max && n_bytes <= h->bytes_max,
               "tokenizer_encode_device: %d queries / %lld bytes exceed the reserve (%d / %lld)", nq, (long long)n_bytes,
               h->nq_max, (long long)h->bytes_max);
  AMDR_REQUIRE(capacity >= n_bytes, "tokenizer_encode_device: term capacity %lld < n_bytes %lld (tokens <= bytes)",
               (long long)capacity, (long long)n_bytes);
  AMDR_REQUIRE(q_ptr_dev && (nq == 0 || (offs_dev && needs_segmenter_dev)) && (n_bytes == 0 || text_dev) &&
                   (capacity == 0 || term_ids_dev),
               "tokenizer_encode_device: null buffer");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  if (nq == 0) {
    AMDR_HIP(hipMemsetAsync(q_ptr_dev, 0, sizeof(int64_t), st));
    return AMDR_OK;
  }
  const unsigned char* text = reinterpret_cast<const unsigned char*>(text_dev);
  const int nb = (nq + kTokBlock - 1) / kTokBlock;
  uint2* spans = h->spans.as<uint2>();
  uint2* cspans = h->cspans.as<uint2>();
  long long* bsum = h->bsum.as<long long>();
  tok_count_kernel<<<nb, kTokBlock, 0, st>>>(text, offs_dev, nq, n_bytes, spans, q_ptr_dev, needs_segmenter_dev, bsum, h->han,
                                             h->route_v.as<double>(), h->route_x.as<int32_t>());
  tok_scan_kernel<<<1, kTokBlock, 0, st>>>(bsum, nb);
  tok_place_kernel<<<nb, kTokBlock, 0, st>>>(offs_dev, nq, n_bytes, spans, cspans, q_ptr_dev, bsum);
  // tokens <= n_bytes: a grid for that many lanes, capped (the lanes stride over the rest)
  const int64_t want = (n_bytes + kTokBlock - 1) / kTokBlock;
  const int grid = (int)(want < 1 ? 1 : want > 8192 ? 8192 : want);
  tok_lookup_kernel<<<grid, kTokBlock, 0, st>>>(text, nq, cspans, q_ptr_dev, h->slots, h->n_slots, h->mask, h->offs,
                                                h->blob, h->single, term_ids_dev);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

int amdr_tokenizer_device_destroy(amdr_tokenizer_device_t* h) {
  if (!h) return AMDR_OK;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();  // work of this handle may still be in flight on a caller's stream
  if (h->slots) (void)hipFree(h->slots);
  if (h->offs) (void)hipFree(h->offs);
  if (h->blob) (void)hipFree(h->blob);
  if (h->single) (void)hipFree(h->single);
  if (h->han_slots) (void)hipFree(h->han_slots);
  if (h->han_offs) (void)hipFree(h->han_offs);
  if (h->han_blob) (void)hipFree(h->han_blob);
  if (h->han_logw) (void)hipFree(h->han_logw);
  if (h->han_word) (void)hipFree(h->han_word);
  h->spans.release();
  h->cspans.release();
  h->bsum.release();
  h->route_v.release();
  h->route_x.release();
  delete h;
  return AMDR_OK;
}

}  // extern "C"

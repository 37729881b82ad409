// ColBERT channel: updates of the resident token store (maxsim_handle.hpp) — amdr_maxsim_add, amdr_maxsim_remove,
// amdr_maxsim_replace — the statistics and images they and amdr_maxsim_create (maxsim.hip) take from the token rows, and
// what reads the store back.  After any sequence of updates the handle is what amdr_maxsim_create makes of the resulting
// store, byte for byte.  Every update builds an MsStagedStore beside the live store and commits it by one exchange after
// the device has finished: a failed update leaves the store it had.
#include "common.hpp"

#include <cstring>
#include <memory>
#include <mutex>
#include <new>

#include "call_scratch.hpp"
#include "maxsim_core.hpp"
#include "maxsim_handle.hpp"
#include "rows_compact.hpp"

namespace amdr {

// fp32 token rows -> the [hi | lo] image (one thread per 8 components), scaled by the store's power of two
__global__ __launch_bounds__(256) void ms_split_store_kernel(const float* __restrict__ D, long n_tokens, float scale,
                                                             unsigned char* __restrict__ img,
                                                             unsigned char* __restrict__ img_hi /* [tok][128 x fp16] */) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;  // (token, group of 8 components)
  if (i >= n_tokens * 16) return;
  const long tok = i >> 4;
  const int g = (int)(i & 15);
  float x[8];
  const f32x4 v0 = *reinterpret_cast<const f32x4*>(D + tok * kDim + 8 * g);
  const f32x4 v1 = *reinterpret_cast<const f32x4*>(D + tok * kDim + 8 * g + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = v0[j], x[4 + j] = v1[j];
  h8 hi, lo;
  ms_split(x, scale, hi, lo);
  *reinterpret_cast<h8*>(img + tok * 512 + 16 * g) = hi;
  *reinterpret_cast<h8*>(img + tok * 512 + 256 + 16 * g) = lo;
  *reinterpret_cast<h8*>(img_hi + tok * 256 + 16 * g) = hi;
}

// largest token L2 norm of the SCALED store (rows x `scale`, the store's power of two: components in [-1, 1], so no
// square underflows to nothing or overflows whatever the store's magnitude), as float bits (error bound of the first
// pass of the two-pass top-k)
__global__ __launch_bounds__(256) void ms_tokmax_kernel(const float* __restrict__ D, long n_tokens, float scale,
                                                        unsigned int* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long wv = ((long)blockIdx.x * 256 + threadIdx.x) >> 6, nw = (long)gridDim.x * 4;
  float m = 0.f;
  for (long t = wv; t < n_tokens; t += nw) {
    const float a = D[t * kDim + lane] * scale, b = D[t * kDim + 64 + lane] * scale;
    float ss = a * a + b * b;
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) ss += __shfl_xor(ss, sft);
    m = fmaxf(m, sqrtf(ss));
  }
  if (lane == 0) atomicMax(out, __float_as_uint(m));
}

// largest |component| of the store as float bits (non-negative floats order like unsigned integers; NaN sorts
// above infinity, so a non-finite store is visible in the result)
__global__ __launch_bounds__(256) void ms_absmax_kernel(const float* __restrict__ D, long n, unsigned int* __restrict__ out) {
  unsigned int m = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    m = max(m, __float_as_uint(D[i]) & 0x7fffffffu);
#pragma unroll
  for (int sft = 1; sft < 64; sft <<= 1) m = max(m, (unsigned int)__shfl_xor((int)m, sft));
  if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

}  // namespace amdr

using namespace amdr;

namespace {

// ---- the store's statistics and images, over a range of token rows (amdr_maxsim_create: all of them; amdr_maxsim_add:
// the new ones).  Synchronous, on the null stream. -------------------------------------------------------------------
// largest |component| of token rows [t0, t1) as float bits (>= 0x7f800000: the range holds a NaN or an infinity)
hipError_t ms_absmax(const float* D, int64_t t0, int64_t t1, unsigned int* bits) {
  unsigned int* mx = nullptr;
  hipError_t e = hipMalloc((void**)&mx, sizeof(unsigned int));
  if (e == hipSuccess) e = hipMemset(mx, 0, sizeof(unsigned int));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(ms_absmax_kernel, dim3(1024), dim3(256), 0, 0, D + (size_t)t0 * kDim, (long)((t1 - t0) * kDim), mx);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(bits, mx, sizeof(unsigned int), hipMemcpyDeviceToHost);
  if (mx) (void)hipFree(mx);
  return e;
}
// Token rows [t0, t1) of D -> both images at `scale`, t1 being the store's end: the zero tile behind it (32 tokens of
// img, 64 of img_hi) is written too.  *norm_max = the largest L2 norm of the scaled rows of the range.
hipError_t ms_convert(const float* D, int64_t t0, int64_t t1, float scale, unsigned char* img, unsigned char* img_hi,
                      float* norm_max) {
  unsigned int* nm = nullptr;
  unsigned int nbits = 0;
  hipError_t e = hipMemset(img + (size_t)t1 * 512, 0, (size_t)32 * 512);
  if (e == hipSuccess) e = hipMemset(img_hi + (size_t)t1 * 256, 0, (size_t)64 * 256);
  if (e == hipSuccess) e = hipMalloc((void**)&nm, sizeof(unsigned int));
  if (e == hipSuccess) e = hipMemset(nm, 0, sizeof(unsigned int));
  if (e == hipSuccess) {
    const int64_t nt = t1 - t0;
    hipLaunchKernelGGL(ms_split_store_kernel, dim3(ceil_div(nt * 16, 256)), dim3(256), 0, 0, D + (size_t)t0 * kDim, (long)nt,
                       scale, img + (size_t)t0 * 512, img_hi + (size_t)t0 * 256);
    e = hipGetLastError();
    if (e == hipSuccess) {
      hipLaunchKernelGGL(ms_tokmax_kernel, dim3(1024), dim3(256), 0, 0, D + (size_t)t0 * kDim, (long)nt, scale, nm);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(&nbits, nm, sizeof(unsigned int), hipMemcpyDeviceToHost);
    memcpy(norm_max, &nbits, sizeof(float));
  }
  if (nm) (void)hipFree(nm);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e;
}
hipError_t ms_alloc_images(int64_t cap_tokens, unsigned char** img, unsigned char** img_hi) {
  hipError_t e = hipMalloc((void**)img, (size_t)(cap_tokens + 32) * 512);  // + one tile: the last tile of the last document reads on
  if (e == hipSuccess) e = hipMalloc((void**)img_hi, (size_t)(cap_tokens + 64) * 256);  // + one 64-token tile
  return e;
}
float ms_scale_of(unsigned int amax_bits) {
  float m;
  memcpy(&m, &amax_bits, sizeof(float));
  return pow2_scale(pow2_exp(m));
}

// ---- amdr_maxsim_add: the incremental form of ms_finish_store -------------------------------------------------------
// nx (a copy of `old` with the new counts) becomes the grown store: the old buffers where there is room, otherwise new
// ones (double, or to fit).  What create() does for a whole store, on the new rows: their largest |component| joins the
// store's, and only when that raises the store's power-of-two scale are the images made again from D — otherwise the old
// rows' image bytes are already what create() would write for the concatenated store.  ptr_host: doc_ptr's new entries.
int ms_add_build(const MsStore& old, MsStagedStore& nx, const float* D_host, const long long* ptr_host, int64_t n_add,
                 const char* who) {
  const int64_t t0 = old.n_tokens, t1 = nx.n_tokens, nd0 = old.n_docs, nd1 = nx.n_docs;
  const bool grow_t = t1 > old.cap_tokens, grow_d = nd1 > old.cap_docs;
  if (grow_t) {
    nx.cap_tokens = old.cap_tokens * 2 > t1 ? old.cap_tokens * 2 : t1;
    AMDR_TRY(dev_alloc(&nx.D, (size_t)nx.cap_tokens * kDim, who));
    AMDR_HIP(hipMemcpy(nx.D, old.D, (size_t)t0 * kDim * sizeof(float), hipMemcpyDeviceToDevice));
  }
  if (grow_d) {
    nx.cap_docs = old.cap_docs * 2 > nd1 ? old.cap_docs * 2 : nd1;
    AMDR_TRY(dev_alloc(&nx.doc_ptr, (size_t)nx.cap_docs + 1, who));
    AMDR_HIP(hipMemcpy(nx.doc_ptr, old.doc_ptr, (size_t)(nd0 + 1) * sizeof(long long), hipMemcpyDeviceToDevice));
  }
  AMDR_HIP(hipMemcpy(nx.D + (size_t)t0 * kDim, D_host, (size_t)(t1 - t0) * kDim * sizeof(float), hipMemcpyHostToDevice));
  AMDR_HIP(hipMemcpy(nx.doc_ptr + nd0 + 1, ptr_host, (size_t)n_add * sizeof(long long), hipMemcpyHostToDevice));
  // statistics from the new rows; the images follow them
  unsigned int add_bits = 0;
  AMDR_HIP(ms_absmax(nx.D, t0, t1, &add_bits));
  if (add_bits > nx.amax_bits) nx.amax_bits = add_bits;  // (float bits of non-negative values order like the values; NaN on top)
  if (old.img) {
    if (nx.amax_bits >= 0x7f800000u) {  // the store is no longer finite: the fp32-input forms serve, as after such a create()
      nx.img = nx.img_hi = nullptr;
      nx.d_scale = 1.f;
      nx.d_norm_max = 0.f;
    } else {
      nx.d_scale = ms_scale_of(nx.amax_bits);
      const bool rescale = nx.d_scale != old.d_scale;  // the exponent can only rise
      if (grow_t || rescale) {  // (a re-split goes to new images too: the old ones serve until it has succeeded)
        nx.img = nx.img_hi = nullptr;
        AMDR_HIP(ms_alloc_images(nx.cap_tokens, &nx.img, &nx.img_hi));
        if (!rescale) {
          AMDR_HIP(hipMemcpy(nx.img, old.img, (size_t)t0 * 512, hipMemcpyDeviceToDevice));
          AMDR_HIP(hipMemcpy(nx.img_hi, old.img_hi, (size_t)t0 * 256, hipMemcpyDeviceToDevice));
        }
      }
      float nm = 0.f;
      AMDR_HIP(ms_convert(nx.D, rescale ? 0 : t0, t1, nx.d_scale, nx.img, nx.img_hi, &nm));
      nx.d_norm_max = rescale || nm > old.d_norm_max ? nm : old.d_norm_max;
      nx.conversions += rescale ? 1 : 0;
    }
  }
  AMDR_HIP(hipDeviceSynchronize());
  return AMDR_OK;
}

// ---- amdr_maxsim_remove and amdr_maxsim_replace: one rebuild into new buffers ----------------------------------------
// The store of n_docs_new documents that the launchers describe (the caller has staged its lists on h->stream), built
// beside the live one and committed at the end; until then every search reads the old store.
//   ptr_launch(len, start, new_ptr, st)          the doc_ptr rebuild (segments_ptr_launch / splice_ptr_launch)
//   plausible(rows)                              the host's look at the new token count new_ptr[n_docs_new]
//   row_launch(rows, new_ptr, start, D_new, st)  the token rows (segments_compact_launch / segments_splice_launch)
// Then create()'s own sequence on the new D: the scale and the bound can FALL here, and a store whose last NaN / infinity
// goes gets its images.  *kernel_ms: the device time of the two launchers, set on success only.
template <class PtrLaunch, class Plausible, class RowLaunch>
int ms_rebuild(amdr_maxsim* h, const char* who, int64_t n_docs_new, double* kernel_ms, PtrLaunch&& ptr_launch,
               Plausible&& plausible, RowLaunch&& row_launch) {
  hipStream_t st = h->stream;
  MsStagedStore nx(*h);
  nx.start_empty();
  nx.n_docs = nx.cap_docs = n_docs_new;
  CallScratch tmp;
  long long *len, *start;
  AMDR_TRY(tmp.alloc(&len, (size_t)n_docs_new, who));
  AMDR_TRY(tmp.alloc(&start, (size_t)n_docs_new, who));
  AMDR_TRY(dev_alloc(&nx.doc_ptr, (size_t)n_docs_new + 1, who));
  // the doc_ptr rebuild, then the host's look at the new token count
  KernelSpans timer(2);
  AMDR_TRY(timer.begin(0, st));
  AMDR_TRY(ptr_launch(len, start, nx.doc_ptr, st));
  AMDR_TRY(timer.end(0, st));
  long long rows = 0;
  AMDR_HIP(hipMemcpyAsync(&rows, nx.doc_ptr + n_docs_new, sizeof(long long), hipMemcpyDeviceToHost, st));
  AMDR_HIP(hipStreamSynchronize(st));
  AMDR_TRY(plausible(rows));
  nx.n_tokens = nx.cap_tokens = rows;
  // the token rows
  AMDR_TRY(dev_alloc(&nx.D, (size_t)rows * kDim, who));
  AMDR_TRY(timer.begin(1, st));
  AMDR_TRY(row_launch(rows, nx.doc_ptr, start, nx.D, st));
  AMDR_TRY(timer.end(1, st));
  AMDR_HIP(hipStreamSynchronize(st));
  AMDR_TRY(ms_finish_store(nx));
  *kernel_ms = timer.ms();
  nx.commit();  // from here on nothing can fail
  return AMDR_OK;
}

}  // namespace

namespace amdr {

int ms_finish_store(MsStore& s) {
  // the split-fp16 image: the store's largest |component| fixes a power-of-two scale into [0.5, 1), then every
  // token row is split once (a store with a NaN / infinity keeps the fp32-input form only); synchronous
  s.d_scale = 1.f, s.d_norm_max = 0.f;
  AMDR_HIP(ms_absmax(s.D, 0, s.n_tokens, &s.amax_bits));
  if (s.amax_bits < 0x7f800000u) {
    s.d_scale = ms_scale_of(s.amax_bits);
    AMDR_HIP(ms_alloc_images(s.cap_tokens, &s.img, &s.img_hi));
    AMDR_HIP(ms_convert(s.D, 0, s.n_tokens, s.d_scale, s.img, s.img_hi, &s.d_norm_max));
    ++s.conversions;
  }
  AMDR_HIP(hipDeviceSynchronize());
  return AMDR_OK;
}

}  // namespace amdr

extern "C" {

int amdr_maxsim_info(amdr_maxsim_t* h, int64_t* out6) {
  AMDR_REQUIRE(h && out6, "maxsim_info: null");
  std::lock_guard<std::mutex> g(h->mu);
  out6[0] = h->n_docs;
  out6[1] = h->n_tokens;
  out6[2] = h->cap_tokens;
  out6[3] = pow2_exp(h->d_scale) - 1;  // d_scale = 2^e = 0.5 * 2^(e + 1)
  out6[4] = h->img ? 1 : 0;
  out6[5] = h->conversions;
  return AMDR_OK;
}

int amdr_maxsim_stats(amdr_maxsim_t* h, float* out2) {
  AMDR_REQUIRE(h && out2, "maxsim_stats: null");
  std::lock_guard<std::mutex> g(h->mu);
  out2[0] = h->d_scale;
  out2[1] = h->d_norm_max;
  return AMDR_OK;
}

// Append documents.  Everything that can fail — allocations, copies, the conversion kernels — runs on buffers or buffer
// tails that no search reads (ms_add_build): a failed add leaves the store it had.
int amdr_maxsim_add(amdr_maxsim_t* h, const float* D_host, const int64_t* doc_ptr_add, int64_t n_add) {
  static const char* const who = "maxsim_add";
  AMDR_REQUIRE(h != nullptr, "maxsim_add: null handle");
  AMDR_REQUIRE(n_add >= 0, "maxsim_add: n_add=%lld", (long long)n_add);
  if (n_add == 0) return AMDR_OK;
  AMDR_REQUIRE(D_host && doc_ptr_add, "maxsim_add: null D / doc_ptr");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_REQUIRE(n_add < (1ll << 32) && h->n_docs + n_add < (1ll << 32), "maxsim_add: too many documents");  // (before doc_ptr_add is walked)
  AMDR_REQUIRE(doc_ptr_add[0] == 0, "maxsim_add: doc_ptr[0] != 0");
  for (int64_t i = 0; i < n_add; ++i)
    AMDR_REQUIRE(doc_ptr_add[i + 1] > doc_ptr_add[i], "maxsim_add: document %lld has no tokens", (long long)i);
  AMDR_HIP(hipSetDevice(h->device));
  const int64_t t0 = h->n_tokens;
  std::unique_ptr<long long[]> ptr_host(new (std::nothrow) long long[(size_t)n_add]);
  if (!ptr_host) return fail(AMDR_ENOMEM, "maxsim_add: host alloc");
  for (int64_t i = 0; i < n_add; ++i) ptr_host[i] = (long long)(t0 + doc_ptr_add[i + 1]);
  MsStagedStore nx(*h);
  nx.n_tokens = t0 + doc_ptr_add[n_add];
  nx.n_docs = h->n_docs + n_add;
  const int rc = ms_add_build(*h, nx, D_host, ptr_host.get(), n_add, who);
  if (rc) {
    if (nx.img && nx.img == h->img) {  // the tail written behind the old end becomes the zero tile again (masked either way)
      (void)hipMemset(h->img + (size_t)t0 * 512, 0, (size_t)32 * 512);
      (void)hipMemset(h->img_hi + (size_t)t0 * 256, 0, (size_t)64 * 256);
    }
    return rc;
  }
  nx.commit();
  return AMDR_OK;
}

// Remove documents: the rebuild from the old store alone.
int amdr_maxsim_remove(amdr_maxsim_t* h, const int64_t* remove_ids, int64_t n_remove) {
  static const char* const who = "maxsim_remove";
  AMDR_REQUIRE(h != nullptr, "maxsim_remove: null handle");
  AMDR_REQUIRE(n_remove >= 0, "maxsim_remove: n_remove=%lld", (long long)n_remove);
  if (n_remove == 0) return AMDR_OK;
  std::lock_guard<std::mutex> g(h->mu);
  const int bad = rc_validate(remove_ids, n_remove, h->n_docs);
  AMDR_REQUIRE(bad == kRcOk, "maxsim_remove: %s", rc_error_text(bad));
  AMDR_REQUIRE(n_remove < h->n_docs, "maxsim_remove: n_remove=%lld would leave no document of %lld", (long long)n_remove,
               (long long)h->n_docs);
  AMDR_HIP(hipSetDevice(h->device));
  const int64_t nd1 = h->n_docs - n_remove;
  CallScratch tmp;
  long long* rm;
  AMDR_TRY(tmp.alloc(&rm, (size_t)n_remove, who));
  AMDR_HIP(hipMemcpyAsync(rm, remove_ids, (size_t)n_remove * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  return ms_rebuild(
      h, who, nd1, &h->remove_kernel_ms,
      [&](long long* len, long long* start, long long* new_ptr, hipStream_t st) {
        return segments_ptr_launch(h->doc_ptr, (long)nd1, rm, (long)n_remove, len, start, new_ptr, st);
      },
      [&](long long rows) {
        if (rows < nd1 || rows >= h->n_tokens)
          return fail(AMDR_EHIP, "maxsim_remove: counted %lld of %lld token rows", rows, (long long)h->n_tokens);
        return (int)AMDR_OK;
      },
      [&](long long rows, const long long* new_ptr, const long long* start, float* D_new, hipStream_t st) {
        return segments_compact_launch(h->D, rows, new_ptr, start, (long)nd1, D_new, st);
      });
}

int amdr_maxsim_remove_kernel_ms(amdr_maxsim_t* h, double* ms) {
  AMDR_REQUIRE(h && ms, "maxsim_remove_kernel_ms: null");
  std::lock_guard<std::mutex> g(h->mu);
  *ms = h->remove_kernel_ms;
  return AMDR_OK;
}

// Replace documents under their pids: the rebuild with a second source, the new token rows and their doc_ptr staged.
int amdr_maxsim_replace(amdr_maxsim_t* h, const int64_t* replace_ids, const float* D_host, const int64_t* doc_ptr_add,
                        int64_t n_rep) {
  static const char* const who = "maxsim_replace";
  AMDR_REQUIRE(h != nullptr, "maxsim_replace: null handle");
  AMDR_REQUIRE(n_rep >= 0, "maxsim_replace: n_rep=%lld", (long long)n_rep);
  if (n_rep == 0) return AMDR_OK;
  AMDR_REQUIRE(D_host && doc_ptr_add, "maxsim_replace: null D / doc_ptr");
  std::lock_guard<std::mutex> g(h->mu);
  const int bad = rc_validate(replace_ids, n_rep, h->n_docs);  // (n_rep <= n_docs, before doc_ptr_add is walked)
  AMDR_REQUIRE(bad == kRcOk, "maxsim_replace: %s", rs_error_text(bad));
  AMDR_REQUIRE(doc_ptr_add[0] == 0, "maxsim_replace: doc_ptr[0] != 0");
  for (int64_t i = 0; i < n_rep; ++i)
    AMDR_REQUIRE(doc_ptr_add[i + 1] > doc_ptr_add[i], "maxsim_replace: document %lld has no tokens", (long long)i);
  AMDR_HIP(hipSetDevice(h->device));
  const int64_t nd = h->n_docs, t_add = doc_ptr_add[n_rep];
  CallScratch tmp;
  long long *ids, *add_ptr;
  float* add_rows;
  AMDR_TRY(tmp.alloc(&ids, (size_t)n_rep, who));
  AMDR_TRY(tmp.alloc(&add_ptr, (size_t)n_rep + 1, who));
  AMDR_TRY(tmp.alloc(&add_rows, (size_t)t_add * kDim, who));
  AMDR_HIP(hipMemcpyAsync(ids, replace_ids, (size_t)n_rep * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  AMDR_HIP(hipMemcpyAsync(add_ptr, doc_ptr_add, (size_t)(n_rep + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  AMDR_HIP(hipMemcpyAsync(add_rows, D_host, (size_t)t_add * kDim * sizeof(float), hipMemcpyHostToDevice, h->stream));
  return ms_rebuild(
      h, who, nd, &h->replace_kernel_ms,
      [&](long long* len, long long* start, long long* new_ptr, hipStream_t st) {
        return splice_ptr_launch(h->doc_ptr, (long)nd, add_ptr, ids, (long)n_rep, len, start, new_ptr, st);
      },
      [&](long long rows) {
        if (rows < nd || rows < t_add || rows - t_add > h->n_tokens - n_rep)
          return fail(AMDR_EHIP, "maxsim_replace: counted %lld token rows from %lld old and %lld new", rows,
                      (long long)h->n_tokens, (long long)t_add);
        return (int)AMDR_OK;
      },
      [&](long long rows, const long long* new_ptr, const long long* start, float* D_new, hipStream_t st) {
        return segments_splice_launch(h->D, add_rows, rows, new_ptr, start, (long)nd, D_new, st);
      });
}

int amdr_maxsim_replace_kernel_ms(amdr_maxsim_t* h, double* ms) {
  AMDR_REQUIRE(h && ms, "maxsim_replace_kernel_ms: null");
  std::lock_guard<std::mutex> g(h->mu);
  *ms = h->replace_kernel_ms;
  return AMDR_OK;
}

int amdr_maxsim_read(amdr_maxsim_t* h, float* D_host, int64_t* doc_ptr_host) {
  AMDR_REQUIRE(h != nullptr, "maxsim_read: null handle");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  if (D_host) AMDR_HIP(hipMemcpy(D_host, h->D, (size_t)h->n_tokens * kDim * sizeof(float), hipMemcpyDeviceToHost));
  if (doc_ptr_host)
    AMDR_HIP(hipMemcpy(doc_ptr_host, h->doc_ptr, (size_t)(h->n_docs + 1) * sizeof(long long), hipMemcpyDeviceToHost));
  return AMDR_OK;
}

}  // extern "C"

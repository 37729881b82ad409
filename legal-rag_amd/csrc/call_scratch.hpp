// Per-call plumbing of the update entry points of all three channels (bm25_update.hip, maxsim_store.hip, dense.hip; the
// token stream of bm25_update.hip allocates through dev_alloc): device arrays that live for one call, the event timer of
// a call's kernels, and the early return on a bad status.  With these an entry point is a straight line of AMDR_TRY /
// AMDR_HIP steps: whatever it leaves through, its scratch and its events go with it.
#pragma once
#include "common.hpp"

namespace amdr {

// count elements of T on the device (count may be 0); a failure names the entry point `who`
template <class T>
int dev_alloc(T** dst, size_t count, const char* who) {
  *dst = nullptr;
  const size_t bytes = count * sizeof(T);
  if (hipMalloc((void**)dst, bytes) != hipSuccess) {
    (void)hipGetLastError();
    *dst = nullptr;
    return fail(AMDR_ENOMEM, "%s: device allocation of %zu B failed", who, bytes);
  }
  return AMDR_OK;
}

// Typed device arrays that live for one call: freed on return.  (Not DevBuf: a call's scratch is no workspace growth.)
struct CallScratch {
  void* held[16] = {};
  int n = 0;
  CallScratch() = default;
  CallScratch(const CallScratch&) = delete;
  CallScratch& operator=(const CallScratch&) = delete;
  ~CallScratch() {
    for (int i = 0; i < n; ++i) (void)hipFree(held[i]);
  }
  template <class T>
  int alloc(T** p, size_t count, const char* who) {
    *p = nullptr;
    if (n == (int)(sizeof(held) / sizeof(held[0]))) return fail(AMDR_EINVAL, "%s: too many scratch arrays", who);
    const int rc = dev_alloc(p, count, who);
    if (!rc && *p) held[n++] = (void*)*p;
    return rc;
  }
};

// Device time of up to two stretches of a stream between events.  Events that cannot be made only lose the time: the
// spans then record nothing and ms() is -1.
struct KernelSpans {
  hipEvent_t ev[4] = {};
  int spans, recorded = 0;
  bool ok = true;
  explicit KernelSpans(int spans_) : spans(spans_) {
    for (int i = 0; i < 2 * spans && ok; ++i)
      if (hipEventCreate(&ev[i]) != hipSuccess) {
        (void)hipGetLastError();
        ev[i] = nullptr;
        ok = false;
      }
  }
  KernelSpans(const KernelSpans&) = delete;
  KernelSpans& operator=(const KernelSpans&) = delete;
  ~KernelSpans() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  int begin(int i, hipStream_t st) {
    if (ok) AMDR_HIP(hipEventRecord(ev[2 * i], st));
    return AMDR_OK;
  }
  int end(int i, hipStream_t st) {
    if (ok) AMDR_HIP(hipEventRecord(ev[2 * i + 1], st));
    ++recorded;
    return AMDR_OK;
  }
  // the summed milliseconds of the recorded spans, once the stream has finished; exactly -1.0 when there is no time
  double ms() const {
    if (!ok || recorded == 0) return -1.0;
    double sum = 0;
    for (int i = 0; i < recorded; ++i) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]) != hipSuccess) {
        (void)hipGetLastError();
        return -1.0;
      }
      sum += (double)t;
    }
    return sum;
  }
};

#define AMDR_TRY(expr)         \
  do {                         \
    const int _rc = (expr);    \
    if (_rc) return _rc;       \
  } while (0)

}  // namespace amdr

// The ColBERT handle, shared by maxsim.hip (create, route, search, destroy) and maxsim_store.hip (add, remove, replace,
// info, read).
#pragma once
#include "common.hpp"

#include <mutex>
#include <utility>

namespace amdr {

// The resident token store, a plain value: the handle is one, and an update builds a second beside it (MsStagedStore).
struct MsStore {
  float* D = nullptr;               // [cap_tokens][128] fp32 token rows
  long long* doc_ptr = nullptr;     // [cap_docs + 1]
  unsigned char* img = nullptr;     // [hi 128 x fp16 | lo 128 x fp16] per token, scaled by d_scale (split-fp16 form)
  unsigned char* img_hi = nullptr;  // [hi 128 x fp16] per token: first pass of the two-pass top-k
  int64_t n_docs = 0;
  int64_t n_tokens = 0;                  // doc_ptr[n_docs]
  int64_t cap_tokens = 0, cap_docs = 0;  // rows that D / img / img_hi and entries (+ 1) that doc_ptr have room for (amdr_maxsim_add)
  unsigned int amax_bits = 0;  // largest |component| of the store as float bits (what d_scale was taken from)
  float d_scale = 1.f;         // power of two; img == nullptr: the store is not finite -> fp32-input form only
  float d_norm_max = 0.f;      // largest token L2 norm of the store x d_scale (error bound of the first pass)
  int64_t conversions = 0;     // whole-store conversions to the images so far (amdr_maxsim_info)
};

// A store in the making: it starts as a copy of the live one, and of its four pointers it OWNS those that are not the live
// store's — the destructor frees them.  Before commit() these are the new buffers (a failed update leaves the store it
// had); commit() exchanges the two values, so afterwards they are the buffers the live store gave up.  One rule for the
// add in place (live buffers reused, tails written), the add that grows and the rebuilds (start_empty(): all new).
struct MsStagedStore : MsStore {
  explicit MsStagedStore(MsStore& live) : MsStore(live), live_(live) {}
  MsStagedStore(const MsStagedStore&) = delete;
  MsStagedStore& operator=(const MsStagedStore&) = delete;
  // (hipFree waits for the device: host-pointer searches are behind the handle's mutex, "_device" work is the caller's to order)
  ~MsStagedStore() {
    if (D && D != live_.D) (void)hipFree(D);
    if (doc_ptr && doc_ptr != live_.doc_ptr) (void)hipFree(doc_ptr);
    if (img && img != live_.img) (void)hipFree(img);
    if (img_hi && img_hi != live_.img_hi) (void)hipFree(img_hi);
  }
  void start_empty() { D = nullptr, doc_ptr = nullptr, img = img_hi = nullptr; }
  void commit() { std::swap(live_, static_cast<MsStore&>(*this)); }

 private:
  MsStore& live_;
};

// What amdr_maxsim_create does on a matrix (maxsim_store.hip): s.D holds s.n_tokens rows and s has no images yet.
int ms_finish_store(MsStore& s);

}  // namespace amdr

struct amdr_maxsim : amdr::MsStore {
  int device = 0;
  double remove_kernel_ms = -1.0;  // device time of the doc_ptr rebuild + the compaction of the last successful amdr_maxsim_remove
  double replace_kernel_ms = -1.0;  // device time of the doc_ptr rebuild + the splice of the last successful amdr_maxsim_replace
  int cus = 0;  // compute units of `device` (the re-scoring pass's grid)
  hipStream_t stream = nullptr;
  std::mutex mu;
  amdr::DevBuf full[2], qbuf, sbuf, ibuf;  // full[0]: "_device" calls, full[1]: host-pointer calls (see dense.hip)
};

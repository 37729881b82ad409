// One merge kernel for every place that ranks in slabs or parts: the GEMV scan and the slab top-k of the batched dense
// forms (packed C32 lists), BM25 (packed C64 lists), the scoped channels and the shard exchange ((scores, ids) lists).
// The instantiations differ only in how a candidate is fetched (the sources below) and in the result row they store
// (topk.hpp topk_store).
#include "topk_merge.hpp"

namespace amdr {

constexpr int kMergeWaves = 4;  // 256-thread blocks

// packed lists part[nparts][nq][k_in] of candidates C; C::pad() = no entry
template <class C>
struct PackedParts {
  typedef C Cand;
  const C* __restrict__ part;
  __device__ __forceinline__ int k_in(int k_out) const { return k_out; }  // a slab list is as deep as the result
  __device__ __forceinline__ bool fetch(size_t off, C& c) const {
    c = part[off];
    return !c.is_pad();
  }
};
// lists scores[nparts][nq][depth], ids[...]; id < 0 = no entry.  Keys: fp64 (T = double) or 32-bit (T = float)
template <class T>
struct ListParts {
  typedef C64 Cand;
  const T* __restrict__ scores;
  const long long* __restrict__ ids;
  int depth;
  __device__ __forceinline__ int k_in(int) const { return depth; }
  __device__ __forceinline__ bool fetch(size_t off, C64& c) const {
    const long long id = ids[off];
    if (id < 0) return false;
    c = sizeof(T) == 8 ? C64::make((double)scores[off], id) : C64::make32((float)scores[off], id);
    return true;
  }
};

// One block per query: stream the nparts lists, keep the best k_out, decode.  LDS: TopkLds<Cand>(kMergeWaves, cap)
template <class Src, class T>
__global__ __launch_bounds__(256) void merge_parts_kernel(Src src, int nparts, int nq, int k_out, int cap,
                                                           T* __restrict__ out_scores, long long* __restrict__ out_ids) {
  typedef typename Src::Cand C;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const TopkLds<C> L(smem, kMergeWaves, cap);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qi = blockIdx.x, k_in = src.k_in(k_out);
  WaveTopK<C> tk;
  tk.init(L.list(wave), cap, k_out);
  const long total = (long)nparts * k_in;
  for (long base = (long)wave * 64; base < total; base += (long)kMergeWaves * 64) {
    const long i = base + lane;
    bool v = i < total;
    C c = C::pad();
    if (v) {
      const long p = i / k_in, j = i - p * k_in;
      v = src.fetch(((size_t)p * nq + qi) * k_in + j, c);
    }
    tk.push_lanes(c, v, lane);
  }
  tk.finalize(lane);
  block_combine_topk(tk, L, kMergeWaves, wave, lane);
  if (wave == 0) topk_store(tk.buf, tk.cnt, k_out, lane, out_scores + (size_t)qi * k_out, out_ids + (size_t)qi * k_out);
}

template <class Src, class T>
static int launch_merge(const Src& src, int nparts, int nq, int k_out, int cap, T* out_scores, int64_t* out_ids,
                        hipStream_t st) {
  const size_t lds = TopkLds<typename Src::Cand>::bytes(kMergeWaves, cap);
  hipLaunchKernelGGL((merge_parts_kernel<Src, T>), dim3(nq), dim3(256), lds, st, src, nparts, nq, k_out, cap, out_scores,
                     (long long*)out_ids);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

template <class T>
int launch_merge_parts(const T* scores, const int64_t* ids, int nparts, int nq, int k_in, int k_out, T* out_scores,
                       int64_t* out_ids, hipStream_t st) {
  return launch_merge(ListParts<T>{scores, (const long long*)ids, k_in}, nparts, nq, k_out, topk_cap(k_out), out_scores, out_ids, st);
}
template int launch_merge_parts<float>(const float*, const int64_t*, int, int, int, int, float*, int64_t*, hipStream_t);
template int launch_merge_parts<double>(const double*, const int64_t*, int, int, int, int, double*, int64_t*,
                                        hipStream_t);

template <class C, class T>
int launch_merge_packed(const C* part, int nparts, int nq, int k, int cap, T* out_scores, int64_t* out_ids, hipStream_t st) {
  return launch_merge(PackedParts<C>{part}, nparts, nq, k, cap, out_scores, out_ids, st);
}
template int launch_merge_packed<C32, float>(const C32*, int, int, int, int, float*, int64_t*, hipStream_t);
template int launch_merge_packed<C64, double>(const C64*, int, int, int, int, double*, int64_t*, hipStream_t);

}  // namespace amdr

using namespace amdr;

extern "C" {

int amdr_merge_topk_f32_device(const float* scores, const int64_t* ids, int32_t n_parts, int32_t nq, int32_t k_in,
                               int32_t k_out, float* out_scores, int64_t* out_ids, int32_t device, void* stream) {
  AMDR_REQUIRE(scores && ids && out_scores && out_ids, "merge_topk: null buffer");
  AMDR_REQUIRE(n_parts >= 1 && nq >= 1 && k_in >= 1 && k_out >= 1 && k_out <= AMDR_MAX_K, "merge_topk: bad sizes");
  AMDR_HIP(hipSetDevice(device));
  return launch_merge_parts<float>(scores, ids, n_parts, nq, k_in, k_out, out_scores, out_ids, (hipStream_t)stream);
}
int amdr_merge_topk_f64_device(const double* scores, const int64_t* ids, int32_t n_parts, int32_t nq, int32_t k_in,
                               int32_t k_out, double* out_scores, int64_t* out_ids, int32_t device, void* stream) {
  AMDR_REQUIRE(scores && ids && out_scores && out_ids, "merge_topk: null buffer");
  AMDR_REQUIRE(n_parts >= 1 && nq >= 1 && k_in >= 1 && k_out >= 1 && k_out <= AMDR_MAX_K, "merge_topk: bad sizes");
  AMDR_HIP(hipSetDevice(device));
  return launch_merge_parts<double>(scores, ids, n_parts, nq, k_in, k_out, out_scores, out_ids, (hipStream_t)stream);
}

}  // extern "C"

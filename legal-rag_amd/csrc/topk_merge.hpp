// The merge of per-part top-k lists (topk_merge.hip): one block per query streams its nparts lists through the staged
// selector.  Order as everywhere: score descending, ties -> lower id, NaN behind every real score, -0.0 as +0.0.
#pragma once
#include "common.hpp"
#include "topk.hpp"

namespace amdr {

// [n_parts, nq, k_in] (score, id) lists -> [nq, k_out]; id < 0 = padding.  T = float (32-bit keys) or double.  The shard
// exchange, the scoped channels and the C entries amdr_merge_topk_f32/f64_device.
template <class T>
int launch_merge_parts(const T* scores, const int64_t* ids, int nparts, int nq, int k_in, int k_out, T* out_scores,
                       int64_t* out_ids, hipStream_t st);
// packed slab lists part[nparts][nq][k] (topk_store_part) -> [nq, k]; cap: the staging capacity of the search's plan.
// C32 -> float (the dense forms), C64 -> double (BM25).  nparts = 0: padding only.
template <class C, class T>
int launch_merge_packed(const C* part, int nparts, int nq, int k, int cap, T* out_scores, int64_t* out_ids, hipStream_t st);

}  // namespace amdr

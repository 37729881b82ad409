// Graph channel of a batch on the device (include/amdretrieval.h amdr_graph_*): per query, the bounded breadth-first
// walk of LawGraphStore.walk from the query's seed rows, then the re-scoring and top-k of GraphRetriever.search
// (retrieval/graph_store.py, retrieval/graph_retriever.py).  Two launches per batch:
//
//   graph_walk_kernel          one block per query.  The host walk is a FIFO BFS cut at `limit` found nodes; its found
//                              order is level order, the children of level L taken in (parent position, edge index)
//                              order.  Every candidate edge gets a position from one counter that only increases
//                              (seeds 0 .. S-1, then level by level); a node's claim slot keeps the smallest position
//                              that reached it (atomicMin), so "seen" = claimed and a candidate wins when the slot
//                              holds its own position.  Winners that are stored nodes are compacted in position order
//                              (wave ballots + a prefix sum over the frontier) and the level is cut at `limit`.
//                              Claim slots: LDS up to kGraphLdsNodes interned ids; beyond, per-block slots in the
//                              workspace stamped with a per-block epoch (tag << 32 | position, the tag DEcreasing with
//                              the epoch so atomicMin lets a new query's claim beat any older one) — never zeroed per
//                              query.
//   graph_score_select_kernel  one block per query.  Per found node: its chunk row (node_row, the language filter),
//                              semantic = dot / (qn * rn + 1e-9f) in fp32 with dot = dense_row_dot (the instruction
//                              sequence of amdr_dense_score_rows), final = ((double)semantic * decay[depth]) *
//                              relw[rel] * conf in fp64; then the top-k by final, ties -> earlier walk position
//                              (Python's stable sort), by rank counting over the <= limit entries in LDS.  A NaN
//                              final ranks behind every number, NaN entries in walk order ("NaN last", as the
//                              other channels).
//
// The one difference from the host path: qn = sqrtf(<q, q>) here, numpy's norm (BLAS, its own summation order) there —
// the semantic term may differ in the last bit.  Built with -ffp-contract=off (Makefile EXACT): qn * rn + 1e-9f and
// the fp64 product must round as Python's separate operations do.
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "dense_dot.hpp"

namespace {

using namespace amdr;

constexpr int kGraphLdsNodes = 12288;   // claim slots in LDS (48 KiB) up to this many interned ids
constexpr int kGraphMaxLimit = 4096;    // found nodes per query (the score kernel keeps 16 B per node in LDS)
constexpr int kGraphMaxSeeds = 1024;    // seed rows per query
constexpr int kWalkThreads = 256;
constexpr int kScoreThreads = 512;
constexpr unsigned kEpochMax = 0xFFFFFFF0u;
constexpr size_t kLdsDefault = 65536;   // LDS a launch gets without hipFuncAttributeMaxDynamicSharedMemorySize
constexpr size_t kStaticLdsMax = 64;    // bound on the __shared__ scalars of either kernel, which count against it

struct GraphTables {  // device copies of the handle's tables
  const long long* node_ptr;
  const int* edge_dst;
  const int* edge_rel;
  const double* conf_raw;
  const double* conf_eff;
  const int* evid;
  const int* present;
  const long long* node_row;
  const int* row_node;
  const float* row_norm;
  const int* row_lang;  // nullable
  int n_nodes;
  long n_rows;
};

struct WalkArgs {
  int limit, default_depth, seed_n, ld, ng, fcap;
  double min_conf;
  const int* rel_max_depth;
  const int* rel_allowed;
  const int* qsel;               // nullable: query g of the call is row qsel[g] of the inputs
  const long long* seeds;        // [*, ld] chunk rows (or node ids when seeds_are_nodes)
  const int* seed_count;         // [*]
  int seeds_are_nodes;
  bool lds_claims;
  unsigned long long* claims;    // [gridDim.x, n_nodes] when !lds_claims
  unsigned* epoch;               // [gridDim.x]
  int* f_edge;                   // [ng, limit] edge that found the node
  int* f_parent;                 // [ng, limit] parent node
  int* f_depth;                  // [ng, limit]
  int* f_count;                  // [ng]
};

struct ScoreArgs {
  int limit, ng, k, lang, d;
  long n_dense;
  const float* X;
  const float* Q;
  const int* qsel;
  const double* rel_weight;
  const double* decay;
  const int* f_edge;
  const int* f_depth;
  const int* f_count;
  int* out_count;
  long long* out_rows;
  double* out_final;
  float* out_sem;
  int* out_depth;
  int* out_rel;
  double* out_conf;
};

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) {
  return lane ? (~0ull >> (64 - lane)) : 0ull;
}

// exclusive prefix sum of a[0, n) in place by one wave; returns the total (in every lane)
__device__ __forceinline__ int wave_exclusive_scan(int* a, int n, int lane) {
  int run = 0;
  for (int b = 0; b < n; b += 64) {
    const int i = b + lane;
    const int v = i < n ? a[i] : 0;
    const int incl = wave_incl_scan(v, lane);
    if (i < n) a[i] = run + incl - v;
    run += __shfl(incl, 63, 64);
  }
  return run;
}

__global__ __launch_bounds__(kWalkThreads) void graph_walk_kernel(GraphTables g, WalkArgs a) {
  extern __shared__ int lds[];
  int* scan = lds;                 // [fcap] candidate offsets of the frontier entries
  int* cnt = lds + a.fcap;         // [fcap] emitted-node offsets
  int* seeds = cnt + a.fcap;       // [seed_n]
  int* lclaim = seeds + a.seed_n;  // [n_nodes] when lds_claims
  __shared__ int s_S, s_total, s_new, s_reset;
  __shared__ unsigned s_tag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = kWalkThreads / 64;
  unsigned long long* gclaim = a.lds_claims ? nullptr : a.claims + (size_t)blockIdx.x * g.n_nodes;

  for (int gq = blockIdx.x; gq < a.ng; gq += gridDim.x) {
    const int q = a.qsel ? a.qsel[gq] : gq;
    int* f_edge = a.f_edge + (size_t)gq * a.limit;
    int* f_parent = a.f_parent + (size_t)gq * a.limit;
    int* f_depth = a.f_depth + (size_t)gq * a.limit;

    // claim slots of this query: LDS -> unclaimed; workspace -> a fresh tag (the slots are refilled only when the
    // block's epoch counter is about to run out)
    if (a.lds_claims) {
      for (int i = tid; i < g.n_nodes; i += kWalkThreads) lclaim[i] = INT_MAX;
    } else {
      if (tid == 0) {
        unsigned e = a.epoch[blockIdx.x];
        s_reset = e >= kEpochMax;
        if (e >= kEpochMax) e = 0;
        s_tag = 0xFFFFFFFEu - e;
        a.epoch[blockIdx.x] = e + 1;
      }
      __syncthreads();
      if (s_reset)
        for (int i = tid; i < g.n_nodes; i += kWalkThreads) __hip_atomic_store(&gclaim[i], ~0ull, __ATOMIC_RELAXED,
                                                                                 __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned long long tag = (unsigned long long)s_tag << 32;

    // seeds: the first min(seed_n, count) rows mapped to nodes, rows without an article key dropped, order kept
    if (wave == 0) {
      int c = a.seed_count[q];
      c = c < 0 ? 0 : (c > a.seed_n ? a.seed_n : c);
      const long long* srow = a.seeds + (size_t)q * a.ld;
      int S = 0;
      for (int b = 0; b < c; b += 64) {
        const int j = b + lane;
        int node = -1;
        if (j < c) {
          const long long r = srow[j];
          if (a.seeds_are_nodes) node = (r >= 0 && r < g.n_nodes) ? (int)r : -1;
          else node = (r >= 0 && r < g.n_rows) ? g.row_node[r] : -1;
        }
        const unsigned long long m = __ballot(node >= 0);
        if (node >= 0) seeds[S + __popcll(m & lanes_below(lane))] = node;
        S += __popcll(m);
      }
      if (lane == 0) s_S = S;
    }
    __syncthreads();
    const int S = s_S;

    auto claim = [&](int node, int pos) {
      if (a.lds_claims) atomicMin(&lclaim[node], pos);
      else atomicMin(&gclaim[node], tag | (unsigned)pos);
    };
    auto owns = [&](int node, int pos) -> bool {
      if (a.lds_claims) return lclaim[node] == pos;
      return __hip_atomic_load(&gclaim[node], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (tag | (unsigned)pos);
    };
    auto passes = [&](long long e) -> bool {
      return !(a.min_conf > 0.0 && g.conf_raw[e] < a.min_conf) && a.rel_allowed[g.edge_rel[e]] != 0;
    };

    for (int s = tid; s < S; s += kWalkThreads) claim(seeds[s], s);
    __syncthreads();

    int found = 0, fs = 0, fn = S, base = S, level = 0;
    while (fn > 0 && found < a.limit) {
      // frontier entry i: (node, edge range if it expands at this level)
      auto entry = [&](int i, long long* e0, int* deg) -> int {
        int node, via;
        if (level == 0) {
          node = seeds[i];
          via = -1;
        } else {
          const int e = f_edge[fs + i];
          node = g.edge_dst[e];
          via = g.edge_rel[e];
        }
        const int md = via < 0 ? a.default_depth : a.rel_max_depth[via];
        *e0 = g.node_ptr[node];
        *deg = level < md ? (int)(g.node_ptr[node + 1] - *e0) : 0;
        return node;
      };
      // candidate offsets: exclusive prefix of the degrees of the expanding entries
      if (wave == 0) {
        for (int i = lane; i < fn; i += 64) {
          long long e0;
          int deg;
          entry(i, &e0, &deg);
          scan[i] = deg;
        }
        const int tot = wave_exclusive_scan(scan, fn, lane);
        if (lane == 0) s_total = tot;
      }
      __syncthreads();
      // claims: candidate (i, j) has position base + scan[i] + j
      for (int i = wave; i < fn; i += nw) {
        long long e0;
        int deg;
        entry(i, &e0, &deg);
        for (int j = lane; j < deg; j += 64)
          if (passes(e0 + j)) claim(g.edge_dst[e0 + j], base + scan[i] + j);
      }
      __syncthreads();
      // winners that are stored nodes, per entry
      for (int i = wave; i < fn; i += nw) {
        long long e0;
        int deg, c = 0;
        entry(i, &e0, &deg);
        for (int jb = 0; jb < deg; jb += 64) {
          const int j = jb + lane;
          bool win = false;
          if (j < deg && passes(e0 + j)) {
            const int dst = g.edge_dst[e0 + j];
            win = owns(dst, base + scan[i] + j) && g.present[dst];
          }
          c += __popcll(__ballot(win));
        }
        if (lane == 0) cnt[i] = c;
      }
      __syncthreads();
      if (wave == 0) {
        const int tot = wave_exclusive_scan(cnt, fn, lane);
        if (lane == 0) s_new = tot;
      }
      __syncthreads();
      // emit in position order, cut at limit
      for (int i = wave; i < fn; i += nw) {
        long long e0;
        int deg;
        const int node = entry(i, &e0, &deg);
        int out = found + cnt[i];
        for (int jb = 0; jb < deg && out < a.limit; jb += 64) {
          const int j = jb + lane;
          bool win = false;
          if (j < deg && passes(e0 + j)) {
            const int dst = g.edge_dst[e0 + j];
            win = owns(dst, base + scan[i] + j) && g.present[dst];
          }
          const unsigned long long m = __ballot(win);
          const int o = out + __popcll(m & lanes_below(lane));
          if (win && o < a.limit) {
            f_edge[o] = (int)(e0 + j);
            f_parent[o] = node;
            f_depth[o] = level + 1;
          }
          out += __popcll(m);
        }
      }
      const int nf = found + s_new < a.limit ? found + s_new : a.limit;
      base += s_total;
      fs = found;
      fn = nf - found;
      found = nf;
      ++level;
      __syncthreads();  // shared counters and the LDS arrays are rewritten by the next level
    }
    if (tid == 0) a.f_count[gq] = found;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kScoreThreads) void graph_score_select_kernel(GraphTables g, ScoreArgs a) {
  extern __shared__ double sfin[];                      // [limit]
  float* ssem = reinterpret_cast<float*>(sfin + a.limit);  // [limit]
  int* srow = reinterpret_cast<int*>(ssem + a.limit);      // [limit]
  __shared__ float s_qn;
  __shared__ int s_valid;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = kScoreThreads / 64;
  const int gq = blockIdx.x;
  const int q = a.qsel ? a.qsel[gq] : gq;
  const float* qv = a.Q + (size_t)q * a.d;
  const int F = a.f_count[gq];
  const int* f_edge = a.f_edge + (size_t)gq * a.limit;
  const int* f_depth = a.f_depth + (size_t)gq * a.limit;
  if (wave == 0) {
    const float qq = dense_row_dot(qv, qv, a.d, lane);
    if (lane == 63) s_qn = sqrtf(qq);
  }
  if (tid == 0) s_valid = 0;
  __syncthreads();
  const float qn = s_qn;

  auto row_of = [&](int i) -> long long {
    const int node = g.edge_dst[f_edge[i]];
    long long r = g.node_row[node];
    if (r >= a.n_dense) r = -1;
    if (r >= 0 && a.lang >= 0 && g.row_lang && g.row_lang[r] != a.lang) r = -1;
    return r;
  };
  auto finish = [&](int i, long long r, float dot) {
    if (lane != 63) return;
    const int e = f_edge[i];
    const float sem = dot / (qn * g.row_norm[r] + 1e-9f);
    sfin[i] = (double)sem * a.decay[f_depth[i]] * a.rel_weight[g.edge_rel[e]] * g.conf_eff[e];
    ssem[i] = sem;
  };
  // two rows per wave and iteration: their loads overlap
  for (int i0 = wave * 2; i0 < F; i0 += nw * 2) {
    const int i1 = i0 + 1;
    const long long r0 = row_of(i0);
    const long long r1 = i1 < F ? row_of(i1) : -1;
    if (lane == 63) {
      srow[i0] = (int)r0;
      if (i1 < F) srow[i1] = (int)r1;
    }
    if (r0 >= 0 && r1 >= 0) {
      const float d0 = dense_row_dot(a.X + (size_t)r0 * a.d, qv, a.d, lane);
      const float d1 = dense_row_dot(a.X + (size_t)r1 * a.d, qv, a.d, lane);
      finish(i0, r0, d0);
      finish(i1, r1, d1);
    } else if (r0 >= 0) {
      finish(i0, r0, dense_row_dot(a.X + (size_t)r0 * a.d, qv, a.d, lane));
    } else if (r1 >= 0) {
      finish(i1, r1, dense_row_dot(a.X + (size_t)r1 * a.d, qv, a.d, lane));
    }
  }
  __syncthreads();
  // rank = entries ahead of i: larger final, or equal final and earlier in the walk.  A NaN final compares false both
  // ways: it ranks behind every number (-inf included), NaN entries among themselves in walk order, so that every
  // valid entry has a rank of its own.
  const size_t o = (size_t)gq * a.k;
  for (int i = tid; i < F; i += kScoreThreads) {
    const int r = srow[i];
    if (r < 0) continue;
    atomicAdd(&s_valid, 1);
    const double fi = sfin[i];
    int rank = 0;
    if (fi == fi) {  // a number: a NaN fj is never ahead of it
      for (int j = 0; j < F; ++j) {
        const double fj = sfin[j];
        rank += (srow[j] >= 0) & ((fj > fi) | ((fj == fi) & (j < i)));
      }
    } else {  // NaN: every number is ahead, and the NaN entries before it
      for (int j = 0; j < F; ++j) {
        const double fj = sfin[j];
        rank += (srow[j] >= 0) & ((fj == fj) | (j < i));
      }
    }
    if (rank < a.k) {
      const int e = f_edge[i];
      a.out_rows[o + rank] = r;
      a.out_final[o + rank] = fi;
      a.out_sem[o + rank] = ssem[i];
      a.out_depth[o + rank] = f_depth[i];
      a.out_rel[o + rank] = g.edge_rel[e];
      a.out_conf[o + rank] = g.conf_eff[e];
    }
  }
  __syncthreads();
  const int c = s_valid < a.k ? s_valid : a.k;
  for (int r = c + tid; r < a.k; r += kScoreThreads) {
    a.out_rows[o + r] = -1;
    a.out_final[o + r] = 0.0;
    a.out_sem[o + r] = 0.f;
    a.out_depth[o + r] = 0;
    a.out_rel[o + r] = -1;
    a.out_conf[o + r] = 0.0;
  }
  if (tid == 0) a.out_count[gq] = c;
}

}  // namespace

struct amdr_graph {
  int device = 0;
  int n_nodes = 0, n_rel = 0, max_deg = 0;
  long n_edges = 0, n_rows = 0;
  bool has_lang = false;
  DevBuf node_ptr, edge_dst, edge_rel, conf_raw, conf_eff, evid, present, node_row, row_node, row_norm, row_lang;
  std::vector<int> h_edge_dst, h_edge_rel, h_evid;  // the walk hook returns edge fields from these
  std::vector<double> h_conf_raw;
  hipStream_t stream = nullptr;
  std::mutex mu;
  // [0]: the "_device" calls; [1]: the host-pointer calls (own stream, inside the mutex)
  struct Work {
    DevBuf f_edge, f_parent, f_depth, f_count, claims, epoch;
    int blocks = 0;  // claim-slot sets of the workspace path
    // host-pointer calls only: inputs, per-call tables and outputs
    DevBuf q, seeds, seed_count, tables, out;
  } ws[2];
};

namespace {

GraphTables tables_of(const amdr_graph* h) {
  GraphTables t;
  t.node_ptr = h->node_ptr.as<long long>();
  t.edge_dst = h->edge_dst.as<int>();
  t.edge_rel = h->edge_rel.as<int>();
  t.conf_raw = h->conf_raw.as<double>();
  t.conf_eff = h->conf_eff.as<double>();
  t.evid = h->evid.as<int>();
  t.present = h->present.as<int>();
  t.node_row = h->node_row.as<long long>();
  t.row_node = h->row_node.as<int>();
  t.row_norm = h->row_norm.as<float>();
  t.row_lang = h->has_lang ? h->row_lang.as<int>() : nullptr;
  t.n_nodes = h->n_nodes;
  t.n_rows = h->n_rows;
  return t;
}

bool lds_claims(const amdr_graph* h) { return h->n_nodes <= kGraphLdsNodes; }

// claim-slot sets of the workspace path: one per resident block, at most 256 MiB of slots
int ws_blocks(const amdr_graph* h, int nq) {
  long by_mem = (256l << 20) / ((long)h->n_nodes * 8);
  long b = by_mem < 256 ? by_mem : 256;
  if (b < 1) b = 1;
  return (int)(b < nq ? b : nq);
}

int ensure_work(amdr_graph* h, int w, int nq, int limit, hipStream_t st) {
  amdr_graph::Work& W = h->ws[w];
  const size_t lists = (size_t)nq * limit * sizeof(int);
  int rc = W.f_edge.ensure(lists);
  if (!rc) rc = W.f_parent.ensure(lists);
  if (!rc) rc = W.f_depth.ensure(lists);
  if (!rc) rc = W.f_count.ensure((size_t)nq * sizeof(int));
  if (rc || lds_claims(h)) return rc;
  const int b = ws_blocks(h, nq);
  if (b > W.blocks) {
    if ((rc = W.claims.ensure((size_t)b * h->n_nodes * sizeof(unsigned long long)))) return rc;
    if ((rc = W.epoch.ensure((size_t)b * sizeof(unsigned)))) return rc;
    AMDR_HIP(hipMemsetAsync(W.claims.p, 0xFF, (size_t)b * h->n_nodes * sizeof(unsigned long long), st));
    AMDR_HIP(hipMemsetAsync(W.epoch.p, 0, (size_t)b * sizeof(unsigned), st));
    W.blocks = b;
  }
  return AMDR_OK;
}

int check_params(const amdr_graph* h, const amdr_graph_params_t* p, int seed_n, int k) {
  AMDR_REQUIRE(p != nullptr, "graph: null params");
  AMDR_REQUIRE(p->limit >= 1 && p->limit <= kGraphMaxLimit, "graph: limit %d outside [1, %d]", p->limit, kGraphMaxLimit);
  AMDR_REQUIRE(seed_n >= 0 && seed_n <= kGraphMaxSeeds, "graph: seed_n %d outside [0, %d]", seed_n, kGraphMaxSeeds);
  AMDR_REQUIRE(k >= 1 && k <= AMDR_MAX_K, "graph: k %d outside [1, %d]", k, AMDR_MAX_K);
  AMDR_REQUIRE(p->rel_max_depth && p->rel_allowed && p->rel_weight && p->decay, "graph: null parameter table");
  // candidate positions stay below INT_MAX (the unclaimed value of an LDS slot)
  const long long pos = ((long long)seed_n + p->limit) * (long long)h->max_deg + seed_n;
  AMDR_REQUIRE(pos < INT_MAX, "graph: (seed_n + limit) * largest out-degree %d exceeds the position range", h->max_deg);
  return AMDR_OK;
}

int fcap_of(int seed_n, int limit) { return seed_n > limit ? seed_n : limit; }

int launch_walk(amdr_graph* h, int w, const amdr_graph_params_t* p, const int* rel_max_depth, const int* rel_allowed,
                const int* qsel, const long long* seeds, const int* seed_count, int ld, int seed_n, int ng,
                int seeds_are_nodes, hipStream_t st) {
  amdr_graph::Work& W = h->ws[w];
  WalkArgs a;
  a.limit = p->limit;
  a.default_depth = p->default_depth;
  a.seed_n = seed_n;
  a.ld = ld;
  a.ng = ng;
  a.fcap = fcap_of(seed_n, p->limit);
  a.min_conf = p->min_conf;
  a.rel_max_depth = rel_max_depth;
  a.rel_allowed = rel_allowed;
  a.qsel = qsel;
  a.seeds = seeds;
  a.seed_count = seed_count;
  a.seeds_are_nodes = seeds_are_nodes;
  a.lds_claims = lds_claims(h);
  a.claims = W.claims.as<unsigned long long>();
  a.epoch = W.epoch.as<unsigned>();
  a.f_edge = W.f_edge.as<int>();
  a.f_parent = W.f_parent.as<int>();
  a.f_depth = W.f_depth.as<int>();
  a.f_count = W.f_count.as<int>();
  const size_t lds = ((size_t)2 * a.fcap + seed_n + (a.lds_claims ? h->n_nodes : 0)) * sizeof(int);
  const int grid = a.lds_claims ? ng : (ng < W.blocks ? ng : W.blocks);
  if (lds + kStaticLdsMax > kLdsDefault)
    AMDR_HIP(hipFuncSetAttribute((const void*)graph_walk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(graph_walk_kernel, dim3(grid), dim3(kWalkThreads), lds, st, tables_of(h), a);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

int launch_score(amdr_graph* h, int w, const float* X, long n_dense, int d, const float* Q, const int* qsel, int ng,
                 int k, int limit, int lang, const double* rel_weight, const double* decay, int* out_count,
                 long long* out_rows, double* out_final, float* out_sem, int* out_depth, int* out_rel, double* out_conf,
                 hipStream_t st) {
  amdr_graph::Work& W = h->ws[w];
  ScoreArgs a;
  a.limit = limit;
  a.ng = ng;
  a.k = k;
  a.lang = lang;
  a.d = d;
  a.n_dense = n_dense;
  a.X = X;
  a.Q = Q;
  a.qsel = qsel;
  a.rel_weight = rel_weight;
  a.decay = decay;
  a.f_edge = W.f_edge.as<int>();
  a.f_depth = W.f_depth.as<int>();
  a.f_count = W.f_count.as<int>();
  a.out_count = out_count;
  a.out_rows = out_rows;
  a.out_final = out_final;
  a.out_sem = out_sem;
  a.out_depth = out_depth;
  a.out_rel = out_rel;
  a.out_conf = out_conf;
  const size_t lds = (size_t)limit * (sizeof(double) + sizeof(float) + sizeof(int));
  if (lds + kStaticLdsMax > kLdsDefault)  // limit 4096: 65 536 B dynamic + the static words
    AMDR_HIP(hipFuncSetAttribute((const void*)graph_score_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds));
  hipLaunchKernelGGL(graph_score_select_kernel, dim3(ng), dim3(kScoreThreads), lds, st, tables_of(h), a);
  AMDR_HIP(hipGetLastError());
  return AMDR_OK;
}

template <class T>
int upload(DevBuf& b, const T* src, size_t n, hipStream_t st) {
  int rc = b.ensure(n * sizeof(T) + 8);
  if (rc) return rc;
  if (n) AMDR_HIP(hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, st));
  return AMDR_OK;
}

// the per-call tables of a host-pointer call, packed into one device buffer:
// decay f64 [limit + 1] | weight f64 [n_rel] | max_depth i32 [n_rel] | allowed i32 [n_rel]
int upload_tables(amdr_graph* h, const amdr_graph_params_t* p, const double** decay, const double** weight,
                  const int** max_depth, const int** allowed) {
  const size_t nd = (size_t)p->limit + 1, nr = h->n_rel ? h->n_rel : 1;
  std::vector<char> blob((nd + nr) * 8 + 2 * nr * 4, 0);
  memcpy(blob.data(), p->decay, nd * 8);
  if (h->n_rel) {
    memcpy(blob.data() + nd * 8, p->rel_weight, h->n_rel * 8);
    memcpy(blob.data() + (nd + nr) * 8, p->rel_max_depth, h->n_rel * 4);
    memcpy(blob.data() + (nd + nr) * 8 + nr * 4, p->rel_allowed, h->n_rel * 4);
  }
  DevBuf& b = h->ws[1].tables;
  int rc = upload(b, blob.data(), blob.size(), h->stream);
  if (rc) return rc;
  char* base = b.as<char>();
  *decay = reinterpret_cast<const double*>(base);
  *weight = reinterpret_cast<const double*>(base + nd * 8);
  *max_depth = reinterpret_cast<const int*>(base + (nd + nr) * 8);
  *allowed = reinterpret_cast<const int*>(base + (nd + nr) * 8 + nr * 4);
  return AMDR_OK;
}

}  // namespace

extern "C" {

int amdr_graph_create(const int64_t* node_ptr, const int32_t* edge_dst, const int32_t* edge_rel,
                      const double* edge_conf_raw, const double* edge_conf_eff, const int32_t* edge_has_evidence,
                      const int32_t* node_present, const int64_t* node_row, const int32_t* row_node,
                      const float* row_norm, const int32_t* row_lang, int32_t n_nodes, int64_t n_edges,
                      int64_t n_rows, int32_t n_rel, int32_t device, amdr_graph_t** out) {
  AMDR_REQUIRE(out != nullptr, "graph_create: out is null");
  *out = nullptr;
  AMDR_REQUIRE(n_nodes >= 0 && n_edges >= 0 && n_edges < INT_MAX && n_rows >= 0 && n_rows < INT_MAX && n_rel >= 0,
               "graph_create: bad sizes");
  AMDR_REQUIRE(node_ptr && node_present && node_row && (row_node || !n_rows) && (row_norm || !n_rows),
               "graph_create: null table");
  AMDR_REQUIRE(!n_edges || (edge_dst && edge_rel && edge_conf_raw && edge_conf_eff && edge_has_evidence),
               "graph_create: null edge table");
  AMDR_REQUIRE(node_ptr[0] == 0 && node_ptr[n_nodes] == n_edges, "graph_create: node_ptr must run from 0 to n_edges");
  int max_deg = 0;
  for (int32_t i = 0; i < n_nodes; ++i) {
    const int64_t deg = node_ptr[i + 1] - node_ptr[i];
    AMDR_REQUIRE(deg >= 0, "graph_create: node_ptr not monotone at %d", i);
    if (deg > max_deg) max_deg = (int)deg;
    AMDR_REQUIRE(node_row[i] >= -1 && node_row[i] < n_rows, "graph_create: node_row[%d] outside [-1, n_rows)", i);
  }
  for (int64_t e = 0; e < n_edges; ++e)
    AMDR_REQUIRE(edge_dst[e] >= 0 && edge_dst[e] < n_nodes && edge_rel[e] >= 0 && edge_rel[e] < n_rel,
                 "graph_create: edge %lld: destination or relation out of range", (long long)e);
  for (int64_t r = 0; r < n_rows; ++r)
    AMDR_REQUIRE(row_node[r] >= -1 && row_node[r] < n_nodes, "graph_create: row_node[%lld] out of range", (long long)r);
  int rc = check_device(device);
  if (rc) return rc;
  amdr_graph* h = new (std::nothrow) amdr_graph;
  if (!h) return fail(AMDR_ENOMEM, "graph_create: host allocation");
  h->device = device;
  h->n_nodes = n_nodes;
  h->n_edges = n_edges;
  h->n_rows = n_rows;
  h->n_rel = n_rel;
  h->max_deg = max_deg;
  h->has_lang = row_lang != nullptr;
  h->h_edge_dst.assign(edge_dst, edge_dst + n_edges);
  h->h_edge_rel.assign(edge_rel, edge_rel + n_edges);
  h->h_evid.assign(edge_has_evidence, edge_has_evidence + n_edges);
  h->h_conf_raw.assign(edge_conf_raw, edge_conf_raw + n_edges);
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete h;
    return fail(AMDR_EHIP, "graph_create: hipStreamCreate: %s", hipGetErrorString(e));
  }
  hipStream_t st = h->stream;
  rc = upload(h->node_ptr, reinterpret_cast<const long long*>(node_ptr), (size_t)n_nodes + 1, st);
  if (!rc) rc = upload(h->edge_dst, edge_dst, n_edges, st);
  if (!rc) rc = upload(h->edge_rel, edge_rel, n_edges, st);
  if (!rc) rc = upload(h->conf_raw, edge_conf_raw, n_edges, st);
  if (!rc) rc = upload(h->conf_eff, edge_conf_eff, n_edges, st);
  if (!rc) rc = upload(h->evid, edge_has_evidence, n_edges, st);
  if (!rc) rc = upload(h->present, node_present, n_nodes, st);
  if (!rc) rc = upload(h->node_row, reinterpret_cast<const long long*>(node_row), n_nodes, st);
  if (!rc) rc = upload(h->row_node, row_node, n_rows, st);
  if (!rc) rc = upload(h->row_norm, row_norm, n_rows, st);
  if (!rc && row_lang) rc = upload(h->row_lang, row_lang, n_rows, st);
  if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail(AMDR_EHIP, "graph_create: upload failed");
  if (rc) {
    amdr_graph_destroy(h);
    return rc;
  }
  *out = h;
  return AMDR_OK;
}

int amdr_graph_reserve(amdr_graph_t* h, int32_t nq_max, int32_t k_max, int32_t limit_max) {
  AMDR_REQUIRE(h != nullptr, "graph_reserve: null handle");
  AMDR_REQUIRE(nq_max >= 1 && k_max >= 1 && k_max <= AMDR_MAX_K && limit_max >= 1 && limit_max <= kGraphMaxLimit,
               "graph_reserve: bad sizes");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  int rc = ensure_work(h, 0, nq_max, limit_max, h->stream);
  if (!rc) AMDR_HIP(hipStreamSynchronize(h->stream));
  return rc;
}

int amdr_graph_walk(amdr_graph_t* h, const int64_t* seeds_host, const int32_t* seed_count_host, int32_t ld,
                    int32_t seed_n, int32_t nq, const amdr_graph_params_t* params, int32_t* out_count,
                    int32_t* out_node, int32_t* out_depth, int32_t* out_parent, int32_t* out_rel, int32_t* out_evidence,
                    double* out_conf) {
  AMDR_REQUIRE(h != nullptr, "graph_walk: null handle");
  int rc = check_params(h, params, seed_n, 1);
  if (rc) return rc;
  AMDR_REQUIRE(nq >= 0 && ld >= seed_n, "graph_walk: bad sizes");
  if (nq == 0) return AMDR_OK;
  AMDR_REQUIRE(seeds_host && seed_count_host && out_count && out_node && out_depth && out_parent && out_rel &&
               out_evidence && out_conf, "graph_walk: null buffer");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  amdr_graph::Work& W = h->ws[1];
  const int L = params->limit;
  const double* decay;
  const double* weight;
  const int *max_depth, *allowed;
  if ((rc = ensure_work(h, 1, nq, L, h->stream))) return rc;
  if ((rc = upload_tables(h, params, &decay, &weight, &max_depth, &allowed))) return rc;
  if ((rc = upload(W.seeds, reinterpret_cast<const long long*>(seeds_host), (size_t)nq * ld, h->stream))) return rc;
  if ((rc = upload(W.seed_count, seed_count_host, (size_t)nq, h->stream))) return rc;
  if ((rc = launch_walk(h, 1, params, max_depth, allowed, nullptr, W.seeds.as<long long>(), W.seed_count.as<int>(), ld,
                        seed_n, nq, 1, h->stream)))
    return rc;
  std::vector<int> fe((size_t)nq * L), fp((size_t)nq * L), fd((size_t)nq * L);
  AMDR_HIP(hipMemcpyAsync(out_count, W.f_count.p, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipMemcpyAsync(fe.data(), W.f_edge.p, fe.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipMemcpyAsync(fp.data(), W.f_parent.p, fp.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipMemcpyAsync(fd.data(), W.f_depth.p, fd.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipStreamSynchronize(h->stream));
  for (int q = 0; q < nq; ++q)
    for (int i = 0; i < L; ++i) {
      const size_t o = (size_t)q * L + i;
      if (i < out_count[q]) {
        const int e = fe[o];
        out_node[o] = h->h_edge_dst[e];
        out_depth[o] = fd[o];
        out_parent[o] = fp[o];
        out_rel[o] = h->h_edge_rel[e];
        out_evidence[o] = h->h_evid[e];
        out_conf[o] = h->h_conf_raw[e];
      } else {
        out_node[o] = out_parent[o] = out_rel[o] = -1;
        out_depth[o] = out_evidence[o] = 0;
        out_conf[o] = 0.0;
      }
    }
  return AMDR_OK;
}

int amdr_graph_search(amdr_graph_t* h, amdr_dense_t* dense, const float* Q_host, const int64_t* seeds_host,
                      const int32_t* seed_count_host, int32_t ld, int32_t seed_n, int32_t nq, int32_t k,
                      const amdr_graph_params_t* params, int32_t* out_count, int64_t* out_rows, double* out_final,
                      float* out_semantic, int32_t* out_depth, int32_t* out_rel, double* out_conf) {
  AMDR_REQUIRE(h != nullptr && dense != nullptr, "graph_search: null handle");
  int rc = check_params(h, params, seed_n, k);
  if (rc) return rc;
  AMDR_REQUIRE(nq >= 0 && ld >= seed_n, "graph_search: bad sizes");
  if (nq == 0) return AMDR_OK;
  AMDR_REQUIRE(Q_host && seeds_host && seed_count_host && out_count && out_rows && out_final && out_semantic &&
               out_depth && out_rel && out_conf, "graph_search: null buffer");
  const float* X;
  long n_dense;
  int d;
  dense_matrix(dense, &X, &n_dense, &d);
  AMDR_REQUIRE(dense_device_of(dense) == h->device, "graph_search: the dense index lives on another device");
  std::lock_guard<std::mutex> g(h->mu);
  AMDR_HIP(hipSetDevice(h->device));
  amdr_graph::Work& W = h->ws[1];
  const double* decay;
  const double* weight;
  const int *max_depth, *allowed;
  if ((rc = ensure_work(h, 1, nq, params->limit, h->stream))) return rc;
  if ((rc = upload_tables(h, params, &decay, &weight, &max_depth, &allowed))) return rc;
  if ((rc = upload(W.q, Q_host, (size_t)nq * d, h->stream))) return rc;
  if ((rc = upload(W.seeds, reinterpret_cast<const long long*>(seeds_host), (size_t)nq * ld, h->stream))) return rc;
  if ((rc = upload(W.seed_count, seed_count_host, (size_t)nq, h->stream))) return rc;
  const size_t nk = (size_t)nq * k;
  // outputs: count | rows | final | conf | semantic | depth | rel
  if ((rc = W.out.ensure(nq * 4 + nk * (8 + 8 + 8 + 4 + 4 + 4) + 64))) return rc;
  char* ob = W.out.as<char>();
  long long* rows_d = reinterpret_cast<long long*>(ob);
  double* fin_d = reinterpret_cast<double*>(ob + nk * 8);
  double* conf_d = reinterpret_cast<double*>(ob + nk * 16);
  float* sem_d = reinterpret_cast<float*>(ob + nk * 24);
  int* depth_d = reinterpret_cast<int*>(ob + nk * 28);
  int* rel_d = reinterpret_cast<int*>(ob + nk * 32);
  int* cnt_d = reinterpret_cast<int*>(ob + nk * 36);
  if ((rc = launch_walk(h, 1, params, max_depth, allowed, nullptr, W.seeds.as<long long>(), W.seed_count.as<int>(), ld,
                        seed_n, nq, 0, h->stream)))
    return rc;
  if ((rc = launch_score(h, 1, X, n_dense, d, W.q.as<float>(), nullptr, nq, k, params->limit, params->lang, weight, decay,
                         cnt_d, rows_d, fin_d, sem_d, depth_d, rel_d, conf_d, h->stream)))
    return rc;
  AMDR_HIP(hipMemcpyAsync(out_rows, rows_d, nk * 8, hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipMemcpyAsync(out_final, fin_d, nk * 8, hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipMemcpyAsync(out_conf, conf_d, nk * 8, hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipMemcpyAsync(out_semantic, sem_d, nk * 4, hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipMemcpyAsync(out_depth, depth_d, nk * 4, hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipMemcpyAsync(out_rel, rel_d, nk * 4, hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipMemcpyAsync(out_count, cnt_d, (size_t)nq * 4, hipMemcpyDeviceToHost, h->stream));
  AMDR_HIP(hipStreamSynchronize(h->stream));
  return AMDR_OK;
}

int amdr_graph_search_device(amdr_graph_t* h, amdr_dense_t* dense, const float* Q_dev, const int32_t* qsel_dev,
                             const int64_t* seeds_dev, const int32_t* seed_count_dev, int32_t ld, int32_t seed_n,
                             int32_t ng, int32_t k, const amdr_graph_params_t* params, int32_t* out_count,
                             int64_t* out_rows, double* out_final, float* out_semantic, int32_t* out_depth,
                             int32_t* out_rel, double* out_conf, void* stream) {
  AMDR_REQUIRE(h != nullptr && dense != nullptr, "graph_search_device: null handle");
  int rc = check_params(h, params, seed_n, k);
  if (rc) return rc;
  AMDR_REQUIRE(ng >= 0 && ld >= seed_n, "graph_search_device: bad sizes");
  if (ng == 0) return AMDR_OK;
  AMDR_REQUIRE(Q_dev && seeds_dev && seed_count_dev && out_count && out_rows && out_final && out_semantic && out_depth &&
               out_rel && out_conf, "graph_search_device: null buffer");
  const float* X;
  long n_dense;
  int d;
  dense_matrix(dense, &X, &n_dense, &d);
  AMDR_REQUIRE(dense_device_of(dense) == h->device, "graph_search_device: the dense index lives on another device");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  AMDR_HIP(hipSetDevice(h->device));
  if ((rc = ensure_work(h, 0, ng, params->limit, st))) return rc;
  if ((rc = launch_walk(h, 0, params, params->rel_max_depth, params->rel_allowed, qsel_dev,
                        reinterpret_cast<const long long*>(seeds_dev), seed_count_dev, ld, seed_n, ng, 0, st)))
    return rc;
  return launch_score(h, 0, X, n_dense, d, Q_dev, qsel_dev, ng, k, params->limit, params->lang, params->rel_weight,
                      params->decay, out_count, reinterpret_cast<long long*>(out_rows), out_final, out_semantic,
                      out_depth, out_rel, out_conf, st);
}

int amdr_graph_destroy(amdr_graph_t* h) {
  if (!h) return AMDR_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  DevBuf* bufs[] = {&h->node_ptr, &h->edge_dst, &h->edge_rel, &h->conf_raw, &h->conf_eff, &h->evid,
                    &h->present,  &h->node_row, &h->row_node, &h->row_norm, &h->row_lang};
  for (DevBuf* b : bufs) b->release();
  for (auto& W : h->ws) {
    DevBuf* wb[] = {&W.f_edge, &W.f_parent, &W.f_depth, &W.f_count, &W.claims, &W.epoch,
                    &W.q,      &W.seeds,    &W.seed_count, &W.tables, &W.out};
    for (DevBuf* b : wb) b->release();
  }
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return AMDR_OK;
}

}  // extern "C"

"""Synthetic graph tables for the graph channel (csrc/graph.hip, amdr_graph_*), and numpy / Python models of its walk and
of its scoring and top-k.

The tables are built directly as the arrays _native.GraphIndex takes (no LawGraphStore, no files), so a test chooses what
the loader would never produce on its own: hubs of a given out-degree, duplicate and self edges, edges to ids that are
no stored node, two nodes on one chunk row, rows without a node, rows past the dense matrix.

  walk_oracle    LawGraphStore.walk (retrieval/graph_store.py) restated on the arrays: a FIFO breadth-first walk, one
                 `seen` set, the cut at `limit` — NOT the level-synchronous claim/compact form of graph_walk_kernel.
  score_oracle   the formula of include/amdretrieval.h, one numpy operation per rounding:
                     sem   = f32(dot) / (f32(f32(sqrt(f32(qq))) * norm) + f32(1e-9))
                     final = ((f64(sem) * decay[depth]) * weight[rel]) * conf_eff
                 valid = the node has a row, the row < n_dense, the language matches; order = final descending, stable
                 over the walk position, NaN behind every number (-inf included); padding past count = min(valid, k).

Two input families make "bit for bit" need no tolerance:
  exact   X and Q hold small integers (|v| <= 8), every query m^2 entries of +-1: the dot is exact in any summation
          order, <q, q> = m^2 and sqrtf is exact.  Rows come from a small pool, norms / decays / weights / confidences
          from small sets, so exact ties (and the near-tie 0.7 vs nextafter(0.7, 1)) are everywhere.
  float   unit-norm random rows, every query also stored as a row of X: dot and <q, q> are taken from
          DenseIndex.score_rows of the same handle (the header's "the dot as amdr_dense_score_rows"), the rest of the
          formula follows in numpy from those bits.

Not a test module (no test_ prefix): tests/test_graph_adversary.py checks the models and the case lists on the CPU,
tests/test_graph_adversary_gpu.py runs the cases on the device.
"""
from __future__ import annotations

import json
from collections import deque
from dataclasses import dataclass, field, replace
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

N_REL = 6
CONF_RAW = (0.0, 0.2, 0.5, 0.7, 0.9, 1.0)
NEAR = float(np.nextafter(0.7, 1.0))            # the near-tie partner of 0.7
NODE_CONF = (1.0, 1.0, 0.3, 0.8, 0.7, NEAR)     # conf_eff of an evidence-less edge: a property of the destination
NORMS = (1.0, 1.0, 2.0, 0.5, 3.0, 0.0, 1e-30)   # 0.0 and 1e-30: the division is by the 1e-9 term
WEIGHTS = (1.2, 1.15, 1.15, -0.5, 0.95, 1.0)    # two equal weights, one negative
MAX_K, MAX_LIMIT, MAX_SEEDS, LDS_NODES = 256, 4096, 1024, 12288

OUTS = ("count", "rows", "final", "semantic", "depth", "relation", "edge_conf")


# ---------------------------------------------------------------------------------------------------------------------
# the graphs of tests/test_graph_device_gpu.py (JSONL for LawGraphStore)

def random_graph(rng, n, path):
    rels = ["next", "prev", "cite", "defined_by", "ref", "amend", "neighbor", "x"]
    with open(path, "w", encoding="utf-8") as f:
        for i in range(n):
            nbs, dl = [], []
            for _ in range(rng.choice([0, 0, 1, 2, 3, 5, 8])):
                r = rng.random()
                if r < 0.08:
                    dst = str(i)                          # self edge
                elif r < 0.16:
                    dst = f"absent{rng.randrange(n)}"     # destination that is no stored node
                elif r < 0.22 and dl:
                    dst = rng.choice(dl)                  # duplicate edge
                else:
                    dst = str(rng.randrange(n))
                dl.append(dst)
                if rng.random() < 0.15:
                    nbs.append(dst)                      # bare string: relation "neighbor", conf 1.0
                else:
                    e = {"id": dst, "relation": rng.choice(rels), "conf": rng.choice([0, 0.2, 0.5, 0.7, 0.9, 1.0, None])}
                    if rng.random() < 0.3:
                        e["evidence"] = {"span": "ev"}
                    nbs.append(e)
            meta = {"_edge_conf": rng.choice([0.3, 0.8])} if rng.random() < 0.2 else {}
            f.write(json.dumps({"article_id": str(i), "neighbors": nbs, "meta": meta}) + "\n")


# ---------------------------------------------------------------------------------------------------------------------
# tables

@dataclass
class Tables:
    """The arrays of amdr_graph_create (field names as retrieval.graph_retriever.GraphTables)."""
    node_ptr: np.ndarray    # i64 [n + 1]
    edge_dst: np.ndarray    # i32 [E]
    edge_rel: np.ndarray    # i32 [E]
    conf_raw: np.ndarray    # f64 [E]
    conf_eff: np.ndarray    # f64 [E]
    evidence: np.ndarray    # i32 [E]
    present: np.ndarray     # i32 [n]
    node_row: np.ndarray    # i64 [n]
    row_node: np.ndarray    # i32 [rows]
    row_norm: np.ndarray    # f32 [rows]
    row_lang: Optional[np.ndarray]  # i32 [rows] or None
    n_rel: int
    hubs: Dict[int, int] = field(default_factory=dict)  # node -> out-degree of the hubs make_tables was asked for

    @property
    def n_nodes(self) -> int:
        return int(self.present.shape[0])

    @property
    def n_rows(self) -> int:
        return int(self.row_node.shape[0])

    def index(self, nat, device: int = 0):
        return nat.GraphIndex(self.node_ptr, self.edge_dst, self.edge_rel, self.conf_raw, self.conf_eff, self.evidence,
                              self.present, self.node_row, self.row_node, self.row_norm, self.row_lang, n_rel=self.n_rel,
                              device=device)

    def row_of(self, node: int) -> int:
        """A chunk row whose node is `node` (make_tables guarantees one for every hub)."""
        r = int(self.node_row[node])
        assert r >= 0 and int(self.row_node[r]) == node, node
        return r

    def with_isolated_node(self) -> "Tables":
        """The same graph with one more interned id: present, no edge, no row."""
        return replace(self, node_ptr=np.append(self.node_ptr, self.node_ptr[-1]), present=np.append(self.present, 1).astype(np.int32),
                       node_row=np.append(self.node_row, -1).astype(np.int64))


def check_tables(t) -> None:
    """What amdr_graph_create requires (graph.hip): nothing built here may depend on a rejected table being accepted."""
    n, E, rows = len(t.present), len(t.edge_dst), len(t.row_node)
    assert len(t.node_ptr) == n + 1 and t.node_ptr[0] == 0 and t.node_ptr[n] == E
    assert np.all(np.diff(t.node_ptr) >= 0)
    assert np.all((t.node_row >= -1) & (t.node_row < rows))
    assert E == 0 or (t.edge_dst.min() >= 0 and t.edge_dst.max() < n and t.edge_rel.min() >= 0 and t.edge_rel.max() < t.n_rel)
    assert np.all((t.row_node >= -1) & (t.row_node < n))
    assert len(t.row_norm) == rows and (t.row_lang is None or len(t.row_lang) == rows)
    assert all(len(x) == E for x in (t.edge_rel, t.conf_raw, t.conf_eff, t.evidence))
    assert np.all(np.diff(t.node_ptr)[t.present == 0] == 0), "an id that is no stored node has no adjacency list"


def make_tables(rng: np.random.Generator, n_nodes: int, *, degrees: Sequence[int] = (0, 0, 1, 2, 3, 5, 8),
                hubs: Optional[Dict[int, int]] = None, hub_dup: float = 0.0, hub_absent: float = 0.0,
                self_share: float = 0.06, dup_share: float = 0.06, absent_share: float = 0.08, n_rel: int = N_REL,
                conf_raw: Sequence[float] = CONF_RAW, evidence_share: float = 0.3, norow_share: float = 0.1,
                shared_rows: int = 4, extra_rows: int = 6, row_holes: float = 0.05, two_lang: bool = False,
                norms: Sequence[float] = NORMS) -> Tables:
    """Random tables over n_nodes interned ids.
    degrees       out-degree of an ordinary stored node, drawn uniformly from this list
    hubs          {node: out-degree}: stored nodes with a chunk row of their own whose list holds `degree` DISTINCT
                  stored non-hub destinations; then a share hub_dup of its entries repeats an earlier entry of the same
                  list and a share hub_absent points at ids that are no stored node
    self_share / dup_share     of the ordinary edges: src -> src, and a repeat of the previous edge's destination
    absent_share  of the ids are destinations only (present 0, no list): claimed by the walk, never emitted
    conf_raw, evidence_share   conf_eff = conf_raw on an edge with evidence, else a value of the DESTINATION (NODE_CONF)
    norow_share   of the ordinary nodes have node_row -1; shared_rows pairs of nodes sit on one row;
    extra_rows    rows beyond the nodes' (row_node -1); row_holes: share of the rows whose row_node is -1 although a
                  node points at them (a seed on such a row is dropped)
    two_lang      row_lang in {0, 1}, else None"""
    hubs = dict(hubs or {})
    n = int(n_nodes)
    is_hub = np.zeros(n, bool)
    is_hub[list(hubs)] = True
    present = (rng.random(n) >= absent_share) | is_hub
    deg = rng.choice(np.asarray(degrees), size=n)
    deg[~present] = 0
    for h, dg in hubs.items():
        deg[h] = dg
    node_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=node_ptr[1:])
    E = int(node_ptr[-1])
    src = np.repeat(np.arange(n), deg)
    dst = rng.integers(0, n, size=E)
    selfm = rng.random(E) < self_share
    dst[selfm] = src[selfm]
    dupm = (rng.random(E) < dup_share) & (np.arange(E) > 0)
    dupm[1:] &= src[1:] == src[:-1]
    if E:
        dupm[0] = False
    for e in np.nonzero(dupm)[0]:
        dst[e] = dst[e - 1]
    pool = np.nonzero(present & ~is_hub)[0]
    absent = np.nonzero(~present)[0]
    for h, dg in hubs.items():
        assert dg <= len(pool), "a hub's distinct destinations come from the stored non-hub nodes"
        lst = rng.permutation(pool)[:dg]
        for j in range(1, dg):
            r = rng.random()
            if r < hub_dup:
                lst[j] = lst[rng.integers(0, j)]
            elif r < hub_dup + hub_absent and len(absent):
                lst[j] = absent[rng.integers(0, len(absent))]
        dst[node_ptr[h]:node_ptr[h + 1]] = lst
    raw = rng.choice(np.asarray(conf_raw, np.float64), size=E)
    evid = (rng.random(E) < evidence_share).astype(np.int32)
    node_conf = rng.choice(np.asarray(NODE_CONF, np.float64), size=n)
    eff = np.where(evid != 0, raw, node_conf[dst] if E else raw)
    n_rows = n + int(extra_rows)
    node_row = rng.permutation(n_rows)[:n].astype(np.int64)
    node_row[(rng.random(n) < norow_share) & ~is_hub] = -1
    free = np.nonzero((node_row >= 0) & ~is_hub)[0]
    for _ in range(int(shared_rows)):
        a, b = rng.choice(free, size=2, replace=False)
        node_row[b] = node_row[a]
    row_node = np.full(n_rows, -1, np.int32)
    for i in range(n):  # the last node of a row wins, as the last chunk of an id does in build_graph_tables
        if node_row[i] >= 0 and not is_hub[i]:
            row_node[node_row[i]] = i
    holes = rng.random(n_rows) < row_holes
    row_node[holes] = -1
    for h in hubs:
        row_node[node_row[h]] = h
    t = Tables(node_ptr=node_ptr, edge_dst=dst.astype(np.int32), edge_rel=rng.integers(0, n_rel, size=E).astype(np.int32),
               conf_raw=raw, conf_eff=eff.astype(np.float64), evidence=evid, present=present.astype(np.int32),
               node_row=node_row, row_node=row_node, row_norm=rng.choice(np.asarray(norms, np.float32), size=n_rows),
               row_lang=rng.integers(0, 2, size=n_rows).astype(np.int32) if two_lang else None, n_rel=int(n_rel), hubs=hubs)
    check_tables(t)
    return t


def make_params(limit: int, *, default_depth: int = 2, min_conf: float = 0.0, rel_max_depth=None, rel_allowed=None,
                rel_weight=None, decay=None, lang: int = -1, n_rel: int = N_REL) -> Dict[str, Any]:
    """One call's amdr_graph_params_t as a dict (the keys of graph_retriever.graph_call_params, plus lang)."""
    limit = int(limit)
    if decay is None:  # not all 1, a zero (depth 4) and repeated values: ties across depths
        decay = np.array([(1.0, 0.5, 0.5, 0.25, 0.0, 0.75)[dd % 6] for dd in range(limit + 1)], np.float64)
    return {"limit": limit, "default_depth": int(default_depth), "min_conf": float(min_conf), "lang": int(lang),
            "rel_max_depth": np.asarray([default_depth] * n_rel if rel_max_depth is None else rel_max_depth, np.int32),
            "rel_allowed": np.asarray([1] * n_rel if rel_allowed is None else rel_allowed, np.int32),
            "rel_weight": np.asarray(WEIGHTS[:n_rel] if rel_weight is None else rel_weight, np.float64),
            "decay": np.asarray(decay, np.float64)}


def host_params(nat, p: Dict[str, Any]):
    return nat.GraphIndex.host_params(p["limit"], p["default_depth"], p["min_conf"], p["rel_max_depth"], p["rel_allowed"],
                                      p["rel_weight"], p["decay"], p["lang"])


# ---------------------------------------------------------------------------------------------------------------------
# the walk

Found = Tuple[int, int, int, int]  # (node, depth, parent, edge index)


def _lists(t):
    c = getattr(t, "_walk_lists", None)
    if c is None:
        c = (t.node_ptr.tolist(), t.edge_dst.tolist(), t.edge_rel.tolist(), t.conf_raw.tolist(), t.present.tolist())
        t._walk_lists = c
    return c


def seed_nodes(t, seeds: Sequence[int], seeds_are_nodes: bool) -> List[int]:
    """Seed entries -> node ids, order kept: node ids outside [0, n) drop out; chunk rows outside [0, n_rows) or whose
    row_node is -1 drop out."""
    n, rows, out = len(t.present), len(t.row_node), []
    for s in seeds:
        s = int(s)
        if seeds_are_nodes:
            if 0 <= s < n:
                out.append(s)
        elif 0 <= s < rows and int(t.row_node[s]) >= 0:
            out.append(int(t.row_node[s]))
    return out


def walk_oracle(t, seeds: Sequence[int], params: Dict[str, Any], seeds_are_nodes: bool) -> List[Found]:
    """LawGraphStore.walk on the arrays; `seeds` are the entries the call takes (the caller applies seed_n / seed_count).
    Seeds are claimed and never emitted; a destination that is no stored node is claimed and never emitted; a node
    reached by relation r expands while its depth < rel_max_depth[r] (seeds: default_depth); min_conf > 0 filters on
    conf_raw; rel_allowed; the cut at limit."""
    ptr, dst_l, rel_l, raw_l, present = _lists(t)
    limit, dd, min_conf = int(params["limit"]), int(params["default_depth"]), float(params["min_conf"])
    rmd, allowed = params["rel_max_depth"].tolist(), params["rel_allowed"].tolist()
    start = seed_nodes(t, seeds, seeds_are_nodes)
    seen = set(start)
    queue = deque((s, 0, -1) for s in start)
    found: List[Found] = []
    while queue and len(found) < limit:
        cur, dist, via = queue.popleft()
        if dist >= (dd if via < 0 else rmd[via]):
            continue
        for e in range(ptr[cur], ptr[cur + 1]):
            dst, rel = dst_l[e], rel_l[e]
            if (min_conf > 0 and raw_l[e] < min_conf) or not allowed[rel] or dst in seen:
                continue
            seen.add(dst)
            if not present[dst]:
                continue
            found.append((dst, dist + 1, cur, e))
            if len(found) >= limit:
                break
            queue.append((dst, dist + 1, rel))
    return found


def walk_tuples(t, found: Sequence[Found]):
    """The tuples _native.GraphIndex.walk returns: (node, depth, parent, relation, has_evidence, conf_raw)."""
    return [(n, dp, par, int(t.edge_rel[e]), bool(t.evidence[e]), float(t.conf_raw[e])) for n, dp, par, e in found]


# ---------------------------------------------------------------------------------------------------------------------
# scoring and top-k

def rank_order(final: np.ndarray) -> np.ndarray:
    """Positions by final descending, stable over the position; NaN behind every number (-inf included), NaN entries in
    position order; -0.0 == +0.0."""
    final = np.asarray(final, np.float64)
    nan = np.isnan(final)
    key = np.where(nan, 0.0, -final) + 0.0
    return np.lexsort((np.arange(len(final)), key, nan))


def score_all(t, X, q, found: Sequence[Found], params, n_dense: int, dots=None, qq=None):
    """(valid positions in rank order, per found position: row, sem f32, final f64).  dots f32 [F] / qq f32: the device's
    own dot bits (float family); default: the exact fp64 dot rounded to fp32 (exact family: no rounding happens)."""
    F = len(found)
    node = np.array([f[0] for f in found], np.int64)
    depth = np.array([f[1] for f in found], np.int64)
    edge = np.array([f[3] for f in found], np.int64)
    row = t.node_row[node] if F else np.zeros(0, np.int64)
    valid = (row >= 0) & (row < n_dense)
    lang = int(params.get("lang", -1))
    if lang >= 0 and t.row_lang is not None:
        valid &= t.row_lang[np.where(valid, row, 0)] == lang
    safe = np.where(valid, row, 0)
    q = np.asarray(q, np.float32)
    with np.errstate(all="ignore"):
        if dots is None:
            dots = (X[safe].astype(np.float64) @ q.astype(np.float64)).astype(np.float32) if F else np.zeros(0, np.float32)
        if qq is None:
            qq = np.float32(np.dot(q.astype(np.float64), q.astype(np.float64)))
        dots = np.asarray(dots, np.float32)
        qn = np.sqrt(np.float32(qq), dtype=np.float32)
        den = (qn * t.row_norm[safe].astype(np.float32)).astype(np.float32) + np.float32(1e-9)
        sem = (dots / den).astype(np.float32)
        final = sem.astype(np.float64) * params["decay"][depth]
        final = final * params["rel_weight"][t.edge_rel[edge]]
        final = final * t.conf_eff[edge]
    pos = np.nonzero(valid)[0]
    order = pos[rank_order(final[pos])]
    return order, row, sem, final


def score_oracle(t, X, q, found: Sequence[Found], params, k: int, n_dense: int, dots=None, qq=None) -> Dict[str, Any]:
    """One query's outputs of amdr_graph_search (count and the [k] arrays of OUTS), padding included."""
    order, row, sem, final = score_all(t, X, q, found, params, n_dense, dots, qq)
    return cut_to_k(t, found, order, row, sem, final, k)


def cut_to_k(t, found, order, row, sem, final, k: int) -> Dict[str, Any]:
    c = min(len(order), int(k))
    top = order[:c]
    edge = np.array([found[i][3] for i in top], np.int64)
    out = {"count": c, "rows": np.full(k, -1, np.int64), "final": np.zeros(k, np.float64),
           "semantic": np.zeros(k, np.float32), "depth": np.zeros(k, np.int32), "relation": np.full(k, -1, np.int32),
           "edge_conf": np.zeros(k, np.float64)}
    out["rows"][:c] = row[top]
    out["final"][:c] = final[top]
    out["semantic"][:c] = sem[top]
    out["depth"][:c] = [found[i][1] for i in top]
    out["relation"][:c] = t.edge_rel[edge]
    out["edge_conf"][:c] = t.conf_eff[edge]
    return out


BITS = {"final": np.uint64, "semantic": np.uint32, "edge_conf": np.uint64}


def assert_outputs_equal(got: Dict[str, np.ndarray], qi: int, exp: Dict[str, Any], what) -> None:
    """count / rows / depth / relation with ==, final / semantic / edge_conf by bit pattern, padding included."""
    assert int(got["count"][qi]) == exp["count"], (what, int(got["count"][qi]), exp["count"])
    for name in OUTS[1:]:
        g, e = np.ascontiguousarray(got[name][qi]), np.ascontiguousarray(exp[name])
        if name in BITS:
            g, e = g.view(BITS[name]), e.view(BITS[name])
        if not np.array_equal(g, e):
            j = int(np.nonzero(g != e)[0][0])
            raise AssertionError(f"{what}: {name}[{j}] = {got[name][qi][j]!r}, expected {exp[name][j]!r}")


# ---------------------------------------------------------------------------------------------------------------------
# the two input families

def exact_rows(rng: np.random.Generator, n: int, d: int, pool: int = 10) -> np.ndarray:
    """n rows drawn from `pool` integer vectors, |v| <= 8: identical rows are common."""
    P = rng.integers(-8, 9, size=(pool, d)).astype(np.float32)
    return np.ascontiguousarray(P[rng.integers(0, pool, size=n)])


def exact_queries(rng: np.random.Generator, nq: int, d: int) -> np.ndarray:
    """m^2 entries of +-1 each (<q, q> = m^2), one of them in the last float4 piece of the row."""
    Q = np.zeros((nq, d), np.float32)
    for i in range(nq):
        m = int(rng.choice([m for m in (1, 2, 3, 5) if m * m <= d]))
        cols = rng.permutation(d - 1)[:m * m - 1].tolist() + [d - 1]
        Q[i, cols] = rng.choice([-1.0, 1.0], size=m * m)
    return Q


def unit_rows(rng: np.random.Generator, n: int, d: int) -> np.ndarray:
    x = rng.standard_normal((n, d)).astype(np.float32)
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True))


# ---------------------------------------------------------------------------------------------------------------------
# the score cases (tests/test_graph_adversary_gpu.py runs them; tests/test_graph_adversary.py checks what they contain)

K_GRID = (1, 2, 10, 64, 255, 256)
LIMIT_GRID = (1, 2, 17, 511, 512, 513, 1024, 4095, 4096)
D_GRID = (4, 252, 256, 260, 1024)
F_GRID = tuple(sorted({0, 1, 511, 512, 513, 4096} | {max(0, k + o) for k in K_GRID for o in (-1, 0, 1)}))
SCORE_NODES = 6000


@dataclass
class ScoreCase:
    """One amdr_graph_search call: nq queries (rows of Q), their seed rows, the parameters; every k of K_GRID."""
    name: str
    params: Dict[str, Any]
    Q: np.ndarray            # f32 [nq, d]
    seeds: np.ndarray        # i64 [nq, ld]
    seed_count: np.ndarray   # i32 [nq]
    seed_n: int


@dataclass
class ScoreWorld:
    t: Tables
    X: np.ndarray
    n_dense: int
    cases: List[ScoreCase]


def score_world(d: int, seed: int = 0) -> ScoreWorld:
    """One graph of SCORE_NODES nodes, an exact-family matrix over fewer rows than the graph has, and the calls:
      F-*       depth-1 walks from a hub of out-degree F (distinct stored destinations): exactly F found nodes, for
                every F of F_GRID, limit 4096 — F below, at and above each k, the rank loop at 511 / 512 / 513
      limit-L   walks up to seven levels deep from random seed rows (query 0: four hubs among them, so that F reaches
                the limit), for every L of LIMIT_GRID; the language filter is on at L = 17 and 513"""
    rng = np.random.default_rng([seed, d])
    hubs = {10 + i: F for i, F in enumerate(F_GRID)}
    t = make_tables(rng, SCORE_NODES, hubs=hubs, two_lang=True, absent_share=0.05)
    n_dense = t.n_rows - 40  # rows past the dense matrix drop out
    X = exact_rows(rng, n_dense, d)
    cases: List[ScoreCase] = []
    hub_rows = np.array([[t.row_of(h)] for h in hubs], np.int64)
    cases.append(ScoreCase("F", make_params(MAX_LIMIT, default_depth=1, rel_max_depth=[1] * N_REL),
                           exact_queries(rng, len(hubs), d), hub_rows, np.ones(len(hubs), np.int32), 1))
    for L in LIMIT_GRID:
        nq, ld = 3, 12
        seeds = rng.integers(0, t.n_rows, size=(nq, ld)).astype(np.int64)
        seeds[0, 2:6] = [t.row_of(h) for h, F in hubs.items() if F in (254, 255, 256, 257)]  # query 0 reaches any limit
        p = make_params(L, default_depth=6, rel_max_depth=[6, 6, 5, 7, 1, 6], lang=1 if L in (17, 513) else -1)
        cases.append(ScoreCase(f"limit-{L}", p, exact_queries(rng, nq, d), seeds, np.array([ld, ld, 5], np.int32), ld))
    return ScoreWorld(t, X, n_dense, cases)


def case_walks(w: ScoreWorld, c: ScoreCase) -> List[List[Found]]:
    return [walk_oracle(w.t, c.seeds[q, :max(0, min(int(c.seed_count[q]), c.seed_n))], c.params, False)
            for q in range(len(c.seed_count))]


def case_expected(w: ScoreWorld, c: ScoreCase, ks: Sequence[int] = K_GRID):
    """{k: [per query outputs]} and the walks, each walk scored once."""
    walks = case_walks(w, c)
    scored = [score_all(w.t, w.X, c.Q[q], f, c.params, w.n_dense) for q, f in enumerate(walks)]
    return {k: [cut_to_k(w.t, f, *s, k) for f, s in zip(walks, scored)] for k in ks}, walks, scored


# ---------------------------------------------------------------------------------------------------------------------
# the walk cases

@dataclass
class WalkCase:
    name: str
    t: Tables
    params: Dict[str, Any]
    seeds: List[List[int]]   # node ids per query


def lds_boundary_tables(seed: int = 3) -> Tuple[Tables, Tables]:
    """A graph of exactly LDS_NODES interned ids (claim slots in LDS, the largest such launch) and the same graph with
    one isolated id more (claim slots in the workspace)."""
    t = make_tables(np.random.default_rng(seed), LDS_NODES, degrees=(1, 2, 3, 5, 8), absent_share=0.04)
    return t, t.with_isolated_node()


def lds_boundary_case(t: Tables, seed: int = 4) -> WalkCase:
    """limit 4096 and 1024 seeds (with duplicates): (2 * 4096 + 1024 + 12288) * 4 = 86 016 B of LDS at 12 288 ids."""
    rng = np.random.default_rng(seed)
    seeds = [rng.integers(0, LDS_NODES, size=MAX_SEEDS).tolist(), rng.integers(0, 40, size=MAX_SEEDS).tolist(),
             rng.integers(0, LDS_NODES, size=3).tolist()]
    return WalkCase(f"boundary-{t.n_nodes}", t, make_params(MAX_LIMIT, default_depth=6, rel_max_depth=[6, 5, 4, 6, 3, 6]), seeds)


def many_queries_case(t: Tables, seed: int, ng: int = 300) -> WalkCase:
    rng = np.random.default_rng(seed)
    seeds = [rng.integers(0, t.n_nodes, size=int(rng.choice([1, 2, 5]))).tolist() for _ in range(ng)]
    return WalkCase(f"ng{ng}-{seed}", t, make_params(64, default_depth=3, rel_max_depth=[3, 2, 3, 1, 3, 2]), seeds)


HUB, HUB_DEG = 0, 5000


def hub_tables(seed: int = 5) -> Tables:
    """Node 0: 5 000 edges.  The first 70 go to distinct stored nodes (a cut at limit L falls at entry L of the list);
    after them a fifth repeats an earlier destination and a twentieth is no stored node.  Node 1: the same list shape
    with the repeats from the start (the cut falls at a later entry than its limit)."""
    rng = np.random.default_rng(seed)
    t = make_tables(rng, 6000, hubs={HUB: HUB_DEG, 1: HUB_DEG}, degrees=(0, 1, 2), absent_share=0.05)
    e0 = int(t.node_ptr[HUB])
    lst = t.edge_dst[e0:e0 + HUB_DEG]
    absent = np.nonzero(t.present == 0)[0]
    for j in range(70, HUB_DEG):
        r = rng.random()
        if r < 0.2:
            lst[j] = lst[rng.integers(0, j)]
        elif r < 0.25:
            lst[j] = absent[rng.integers(0, len(absent))]
    e1 = int(t.node_ptr[1])
    lst1 = t.edge_dst[e1:e1 + HUB_DEG]
    for j in range(1, HUB_DEG):
        r = rng.random()
        if r < 0.3:
            lst1[j] = lst1[rng.integers(0, j)]
        elif r < 0.33:
            lst1[j] = HUB if r < 0.31 else 1  # an edge to the other hub / a self edge
    # a min_conf of 0.5 removes exactly the hub's first 64 entries
    t.conf_raw[e0:e0 + 64] = 0.2
    t.conf_raw[e0 + 64:e0 + HUB_DEG] = 0.9
    check_tables(t)
    return t


def hub_cases(t: Tables) -> List[WalkCase]:
    out = []
    for L in (63, 64, 65, 4096):
        out.append(WalkCase(f"hub-limit-{L}", t, make_params(L, default_depth=2), [[HUB], [1], [1, HUB]]))
    out.append(WalkCase("hub-min-conf", t, make_params(4096, default_depth=1, min_conf=0.5), [[HUB]]))
    out.append(WalkCase("hub-depth-0", t, make_params(4096, default_depth=0, rel_max_depth=[0] * N_REL), [[HUB], [1, 5, 9]]))
    out.append(WalkCase("hub-relations-stop", t, make_params(4096, default_depth=3, rel_max_depth=[0, 3, 0, 3, 0, 3],
                                                             rel_allowed=[1, 1, 0, 1, 1, 1]), [[HUB], [7, 8, 9, 1]]))
    return out


def fanout_tables(seed: int = 6, fan: int = 20) -> Tables:
    """Node 0 -> 20 nodes -> 20 each -> 3 each: the second frontier has 400 entries (the frontier prefix sums run over
    more than 256 of them), every one of which expands."""
    rng = np.random.default_rng(seed)
    n1, n2, n3 = fan, fan * fan, fan * fan * 3
    n = 1 + n1 + n2 + n3
    deg = np.zeros(n, np.int64)
    deg[0] = fan
    deg[1:1 + n1] = fan
    deg[1 + n1:1 + n1 + n2] = 3
    node_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=node_ptr[1:])
    dst = np.concatenate([np.arange(1, 1 + n1), np.arange(1 + n1, 1 + n1 + n2), np.arange(1 + n1 + n2, n)]).astype(np.int32)
    E = len(dst)
    raw = rng.choice(np.asarray(CONF_RAW[1:], np.float64), size=E)
    t = Tables(node_ptr=node_ptr, edge_dst=dst, edge_rel=rng.integers(0, N_REL, size=E).astype(np.int32), conf_raw=raw,
               conf_eff=raw.copy(), evidence=np.ones(E, np.int32), present=np.ones(n, np.int32),
               node_row=np.arange(n, dtype=np.int64), row_node=np.arange(n, dtype=np.int32),
               row_norm=np.ones(n, np.float32), row_lang=None, n_rel=N_REL)
    check_tables(t)
    return t


def fanout_case(t: Tables) -> WalkCase:
    return WalkCase("fan-out", t, make_params(4096, default_depth=3, rel_max_depth=[3] * N_REL), [[0], [0, 1, 2]])

"""Graph channel: walk the law graph from the seed hits, rescore the visited articles.

Mirror of legalrag/retrieval/graph_retriever.py (GraphRetriever :53-219, helpers :19-50)
and SURVEY.md §8f-2.  The reference re-EMBEDS the text of every visited article on every
query (up to graph_limit = 800 BERT forwards, graph_retriever.py:177-179) only to take its
cosine with the query vector.  Those articles are rows of the chunk matrix that is already
resident in HBM for the dense channel (row i <-> store.chunks[i], vector_store.py:95-128),
so here the step is one `amdr_dense_score_rows` call — a row gather + dot on the device —
plus the same scalar arithmetic:

    semantic = <q, x_row> / (|q| * |x_row| + 1e-9)                 (graph_retriever.py:19-21)
    final    = semantic * (1 + depth)^-gamma * max_r w(r) * conf   (:24-46, :186-191)

Row norms are computed once per loaded index.  An article without a row in the matrix
(never the case for an index built by build_faiss_index over the same corpus) falls back
to embedding its text, as the reference does.  Results agree with the reference to fp32
rounding of the dot product (tests/test_graph.py pins walk, hydration, scores and order
against vectors produced by the reference's own code).
"""
from __future__ import annotations

import copy
import math
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from ..schemas import LawChunk, RetrievalHit
from .graph_store import LawGraphStore, _clean
from .vector_store import VectorStore

_REL_WEIGHT = {"defined_by": 1.20, "defines_term": 1.10, "cite": 1.15, "cited": 1.15, "ref": 1.15, "amend": 1.10,
               "next": 0.95, "prev": 0.95, "neighbor": 1.00}


def _cosine_sim(a: np.ndarray, b: np.ndarray) -> float:
    return float(np.dot(a, b) / ((np.linalg.norm(a) * np.linalg.norm(b)) + 1e-9))


def _depth_decay(depth: int, gamma: float = 0.7) -> float:
    return float(1.0 / ((1.0 + max(1, int(depth or 1))) ** gamma))


def _relation_weight(relations: List[str]) -> float:
    rels = [str(r).lower() for r in (relations or [])]
    return float(max(_REL_WEIGHT.get(r, 1.0) for r in rels)) if rels else 1.0


def _article_key(obj: Any) -> Optional[str]:
    aid = getattr(obj, "article_id", None) or getattr(obj, "id", None)
    return str(aid) if aid else None


@dataclass
class GraphTables:
    """Host form of the device graph channel's tables (include/amdretrieval.h amdr_graph_create) over the interned
    article ids `names`: every stored node, every edge destination and every stripped chunk key."""
    names: List[str]
    rel_names: List[str]
    lang_names: List[str]
    node_ptr: np.ndarray      # i64 [n + 1]
    edge_dst: np.ndarray      # i32 [E]
    edge_rel: np.ndarray      # i32 [E]
    conf_raw: np.ndarray      # f64 [E]  float(conf or 1.0): the min_conf filter
    conf_eff: np.ndarray      # f64 [E]  the conf the score takes (the stored node's _edge_conf without evidence)
    evidence: np.ndarray      # i32 [E]
    present: np.ndarray       # i32 [n]  a stored node
    node_row: np.ndarray      # i64 [n]  chunk row of the article (last chunk wins), -1: none / empty text
    row_node: np.ndarray      # i32 [rows] node of the chunk's stripped key, -1: none
    row_lang: np.ndarray      # i32 [rows] index into lang_names


def build_graph_tables(graph: LawGraphStore, chunks: Sequence[LawChunk]) -> GraphTables:
    """The tables of amdr_graph_create from LawGraphStore.nodes / .adj and the store's chunks, by the expressions the
    host walk and GraphRetriever.search use (graph_store.py walk, _bind_rows, search's hydration)."""
    graph.load()
    index: Dict[str, int] = {}
    names: List[str] = []

    def intern(x: str) -> int:
        i = index.get(x)
        if i is None:
            i = index[x] = len(names)
            names.append(x)
        return i

    for aid in graph.nodes:
        intern(aid)
    for aid in list(graph.nodes):
        for dst, _rel, _conf, _ev in graph.adj.get(aid, []):
            intern(dst)
    row_node = np.full(len(chunks), -1, dtype=np.int32)
    row_of: Dict[str, int] = {}
    langs: Dict[str, int] = {}
    row_lang = np.zeros(len(chunks), dtype=np.int32)
    for row, c in enumerate(chunks):
        key = _article_key(c)
        if key:
            row_of[key] = row  # the last chunk of an id wins (_bind_rows)
            if _clean(key):
                row_node[row] = intern(_clean(key))  # seeds are stripped by walk()
        row_lang[row] = langs.setdefault((getattr(c, "lang", None) or "zh").strip().lower(), len(langs))
    n = len(names)
    rels: Dict[str, int] = {}
    node_ptr = np.zeros(n + 1, dtype=np.int64)
    dst_l, rel_l, raw_l, eff_l, ev_l = [], [], [], [], []
    for i, aid in enumerate(names):
        for dst, rel, conf, ev in graph.adj.get(aid, []) if aid in graph.nodes else []:
            dst_l.append(index[dst])
            rel_l.append(rels.setdefault(rel, len(rels)))
            raw_l.append(float(conf))
            if ev:
                eff_l.append(float(conf))
            else:
                stored = graph.nodes.get(dst)
                eff_l.append(float(((getattr(stored, "meta", {}) or {}).get("_edge_conf", 1.0)) or 1.0) if stored else 1.0)
            ev_l.append(1 if ev else 0)
        node_ptr[i + 1] = len(dst_l)
    node_row = np.full(n, -1, dtype=np.int64)
    for i, aid in enumerate(names):
        row = row_of.get(aid)
        if row is not None and (getattr(chunks[row], "text", "") or "").strip():
            node_row[i] = row
    return GraphTables(names=names, rel_names=list(rels), lang_names=list(langs), node_ptr=node_ptr,
                       edge_dst=np.asarray(dst_l, dtype=np.int32), edge_rel=np.asarray(rel_l, dtype=np.int32),
                       conf_raw=np.asarray(raw_l, dtype=np.float64), conf_eff=np.asarray(eff_l, dtype=np.float64),
                       evidence=np.asarray(ev_l, dtype=np.int32),
                       present=np.asarray([1 if a in graph.nodes else 0 for a in names], dtype=np.int32),
                       node_row=node_row, row_node=row_node, row_lang=row_lang)


def _rows_epoch(index: Any) -> int:
    """How often rows of `index` were removed or replaced in place (vector_store.FlatIPIndex.rows_epoch; 0 for an index
    without)."""
    return int(getattr(index, "rows_epoch", 0) or 0)


def _depth_bound(v: Any) -> int:
    """dist >= v for an integer dist, as an integer bound."""
    return int(max(-(2 ** 31), min(2 ** 31 - 1, math.ceil(float(v)))))


def graph_call_params(rcfg: Any, rel_names: Sequence[str], top_k: int) -> Dict[str, Any]:
    """Per-call parameters of the device channel from cfg.retrieval, resolved as GraphRetriever.search and
    LawGraphStore.walk resolve them: limit, default_depth, min_conf, gamma and the per-relation max_depth / allowed /
    weight tables, decay[depth] for depth 0 .. limit."""
    k = max(1, int(top_k))
    depths = rcfg.graph_walk_depths if hasattr(rcfg, "graph_walk_depths") else {"default": 2}
    limit = int(getattr(rcfg, "graph_limit", k * 8) if rcfg else k * 8)
    rel_types = getattr(rcfg, "graph_rel_types", None) if rcfg else None
    min_conf = float(getattr(rcfg, "graph_min_conf", 0.0) if rcfg else 0.0)
    gamma = float(getattr(rcfg, "graph_depth_gamma", 0.7) if rcfg else 0.7)
    if depths is None:
        depths = getattr(rcfg, "graph_walk_depths", None) or {"default": 2}
    default_depth = depths.get("default", 2)
    limit = max(1, int(limit))
    allowed = {str(r) for r in rel_types} if rel_types else None
    return {
        "limit": limit, "default_depth": _depth_bound(default_depth), "min_conf": float(min_conf or 0.0), "gamma": gamma,
        "rel_max_depth": np.asarray([_depth_bound(depths.get(r, default_depth) if r else default_depth)
                                     for r in rel_names] or [0], dtype=np.int32),
        "rel_allowed": np.asarray([1 if allowed is None or r in allowed else 0 for r in rel_names] or [0], dtype=np.int32),
        "rel_weight": np.asarray([_relation_weight([r]) for r in rel_names] or [1.0], dtype=np.float64),
        "decay": np.asarray([_depth_decay(d, gamma=gamma) for d in range(limit + 1)], dtype=np.float64),
    }


@dataclass
class GraphRetriever:
    cfg: Any
    graph: Optional[LawGraphStore] = None
    store: Optional[VectorStore] = None
    id2chunk: Optional[Dict[str, LawChunk]] = None

    def __post_init__(self) -> None:
        if self.graph is None:
            self.graph = LawGraphStore(self.cfg)
        if self.store is None:
            self.store = VectorStore.from_config(self.cfg)
        self.store.load()
        self._bind_rows()

    def _bind_rows(self) -> None:
        """article id -> chunk and -> row of the resident matrix; the LAST chunk of an id wins,
        as in the reference's dict build (:76-80)."""
        chunks = list(getattr(self.store, "chunks", []) or [])
        self.id2chunk, self._row_of = {}, {}
        for row, c in enumerate(chunks):
            key = _article_key(c)
            if key:
                self.id2chunk[key] = c
                self._row_of[key] = row
        self._norms: Optional[np.ndarray] = None
        self._bound_index = getattr(self.store, "index", None)
        self._bound_epoch = _rows_epoch(self._bound_index)

    def _row_norms(self) -> Optional[np.ndarray]:
        index = getattr(self.store, "index", None)
        if index is None or not hasattr(index, "native"):
            return None
        # store reloaded (mtime guard), or rows removed in place (FlatIPIndex.remove_ids renumbers the survivors): rows
        # may have moved.  The count of removals, not the row count: a removal followed by an add of equal size moves them too
        if index is not self._bound_index or _rows_epoch(index) != self._bound_epoch:
            self._bind_rows()
        if self._norms is None:
            # a row-sharded index (vector_store.ShardedFlatIPIndex) holds rows [r0, r1) only: the norms of the other
            # rows stay -inf here and come from their own rank in _semantic's all-reduce
            r0, r1 = (index.row_offset, index.row_end) if hasattr(index, "spec") else (0, int(index.ntotal))
            norms = np.full(int(index.ntotal), -np.inf, dtype=np.float32)
            for lo in range(r0, r1, 65536):
                norms[lo:min(lo + 65536, r1)] = np.linalg.norm(index.reconstruct_n(lo, min(65536, r1 - lo)), axis=1)
            self._norms = norms
        return self._norms

    # ------------------------------------------------------------- device channel
    def device_graph(self):
        """(GraphIndex, GraphTables) of the graph channel on the device, built once per loaded index (rebuilt when the
        store reloads).  ValueError for a row-sharded index (no device walk there) or a store without a device matrix."""
        from .. import _native
        norms = self._row_norms()  # rebinds the rows when the store reloaded
        index = getattr(self.store, "index", None)
        if norms is None:
            raise ValueError("graph_channel='device' needs the store's chunk matrix on the device (a native index)")
        if hasattr(index, "spec"):
            raise ValueError("graph_channel='device' does not run on a row-sharded index (cfg.retrieval.shard); "
                             "use graph_channel='host'")
        cached = self.__dict__.get("_dev_graph")
        if cached is not None and cached[0] is index and cached[3] == _rows_epoch(index):
            return cached[1], cached[2]
        t = build_graph_tables(self.graph, list(getattr(self.store, "chunks", []) or []))
        if len(t.row_node) != int(index.ntotal):
            raise ValueError(f"graph_channel='device': {len(t.row_node)} chunks but {int(index.ntotal)} matrix rows")
        g = _native.GraphIndex(t.node_ptr, t.edge_dst, t.edge_rel, t.conf_raw, t.conf_eff, t.evidence, t.present,
                               t.node_row, t.row_node, norms, t.row_lang, n_rel=len(t.rel_names),
                               device=int(getattr(index, "_device", getattr(self.cfg.retrieval, "device", 0)) or 0))
        self.__dict__["_dev_graph"] = (index, g, t, _rows_epoch(index))
        return g, t

    def device_params(self, top_k: int, lang: Optional[str] = None):
        """(graph_call_params dict, lang id) for a call: the limits of the device channel are checked here."""
        from .. import _native
        _g, t = self.device_graph()
        p = graph_call_params(getattr(self.cfg, "retrieval", None), t.rel_names, top_k)
        if p["limit"] > _native.GRAPH_MAX_LIMIT:
            raise ValueError(f"graph_channel='device': graph_limit {p['limit']} exceeds the device limit of "
                             f"{_native.GRAPH_MAX_LIMIT}")
        lang_id = -1 if not lang else (t.lang_names.index(lang) if lang in t.lang_names else len(t.lang_names))
        return p, lang_id

    def hits_from_device(self, out: Dict[str, np.ndarray], qi: int, params: Dict[str, Any]) -> List[RetrievalHit]:
        """RetrievalHits of query qi of a device call, with GraphRetriever.search's fields and score_breakdown keys."""
        _g, t = self.device_graph()
        chunks = self.store.chunks
        hits: List[RetrievalHit] = []
        for r in range(int(out["count"][qi])):
            cc = copy.copy(chunks[int(out["rows"][qi, r])])
            cc.source = "graph"
            depth, rel = int(out["depth"][qi, r]), int(out["relation"][qi, r])
            s, final, conf = float(out["semantic"][qi, r]), float(out["final"][qi, r]), float(out["edge_conf"][qi, r])
            hits.append(RetrievalHit(chunk=cc, score=final, rank=r + 1, source="graph", score_breakdown={
                "channel": "graph", "semantic": s, "depth_decay": float(params["decay"][depth]),
                "relation_weight": float(params["rel_weight"][rel]), "edge_conf": conf, "final": final,
                "graph_depth": depth, "relations": [t.rel_names[rel]]}))
        return hits

    def search_device(self, q_vecs: np.ndarray, seed_rows: np.ndarray, seed_count: np.ndarray, *, top_k: int = 10,
                      lang: Optional[str] = None) -> List[List[RetrievalHit]]:
        """GraphRetriever.search for a batch in one device call (host pointers): q_vecs [nq, d] (the NON-query
        embeddings, as store._embed(question)), seed_rows [nq, ld] chunk rows of the seeds, seed_count [nq]."""
        from .. import _native
        g, _t = self.device_graph()
        p, lang_id = self.device_params(top_k, lang)
        seed_rows = np.asarray(seed_rows, dtype=np.int64).reshape(len(seed_count), -1)
        hp, keep = _native.GraphIndex.host_params(p["limit"], p["default_depth"], p["min_conf"], p["rel_max_depth"],
                                                  p["rel_allowed"], p["rel_weight"], p["decay"], lang_id)
        k = max(1, int(top_k))
        out = g.search(self.store.index.native, q_vecs, seed_rows, seed_count, min(seed_rows.shape[1], _native.GRAPH_MAX_SEEDS),
                       k, hp)
        del keep
        return [self.hits_from_device(out, qi, p) for qi in range(len(seed_count))]

    def _semantic(self, question: str, chunks: List[LawChunk], keys: List[str]) -> List[float]:
        qvec = np.asarray(self.store._embed(question), dtype=np.float32).reshape(-1)
        qn = float(np.linalg.norm(qvec))
        norms = self._row_norms()
        rows = np.array([self._row_of.get(k, -1) if norms is not None else -1 for k in keys], dtype=np.int64)
        sem = [0.0] * len(chunks)
        on_dev = np.nonzero(rows >= 0)[0]
        if on_dev.size:
            index = self.store.index
            if hasattr(index, "spec"):
                # row-sharded: every candidate row lives on exactly one rank — score the local ones, -inf for the
                # rest, ONE all-reduce(max) of (dots, norms) over the ranks; identical on every rank afterwards
                from . import sharding
                g = rows[on_dev]
                mine = (g >= index.row_offset) & (g < index.row_end)
                both = np.full((2, g.size), -np.inf, dtype=np.float32)
                if mine.any():
                    both[0, mine] = index.native.score_rows(qvec, g[mine] - index.row_offset)[0]
                    both[1, mine] = norms[g[mine]]
                both = sharding.allreduce_max_numpy(both, index._device, group=index.spec.group)
                dots, row_norms = both[0], both[1]
            else:
                dots = index.native.score_rows(qvec, rows[on_dev])[0]
                row_norms = norms[rows[on_dev]]
            for j, dot, rn in zip(on_dev, dots, row_norms):
                sem[j] = float(np.float32(dot) / np.float32(np.float32(qn * rn) + np.float32(1e-9)))
        rest = [j for j in range(len(chunks)) if rows[j] < 0]
        if rest:
            vecs = self.store._embed([chunks[j].text for j in rest])
            for j, v in zip(rest, vecs):
                sem[j] = _cosine_sim(qvec, v)
        return sem

    def search(self, question: str, seeds: List[Any], *, decision: Any = None, lang: Optional[str] = None,
               top_k: int = 10) -> List[RetrievalHit]:
        rcfg = getattr(self.cfg, "retrieval", None)
        k = max(1, int(top_k))
        depths = rcfg.graph_walk_depths if hasattr(rcfg, "graph_walk_depths") else {"default": 2}
        limit = int(getattr(rcfg, "graph_limit", k * 8) if rcfg else k * 8)
        rel_types = getattr(rcfg, "graph_rel_types", None) if rcfg else None
        min_conf = float(getattr(rcfg, "graph_min_conf", 0.0) if rcfg else 0.0)
        gamma = float(getattr(rcfg, "graph_depth_gamma", 0.7) if rcfg else 0.7)

        seed_ids = [key for key in (_article_key(getattr(h, "chunk", None)) for h in seeds or []) if key]
        if not seed_ids:
            return []
        nodes = self.graph.walk(start_ids=seed_ids, relation_max_depth=depths, limit=limit, rel_types=rel_types,
                                min_conf=min_conf)
        if not nodes:
            return []

        chunks: List[LawChunk] = []
        keys: List[str] = []
        meta: List[Dict[str, Any]] = []
        taken = set()
        for n in nodes:  # first visit of an article wins; articles without text / of another language drop out
            aid = str(getattr(n, "article_id", "") or "").strip()
            if not aid or aid in taken:
                continue
            taken.add(aid)
            c = self.id2chunk.get(aid)
            if not c or not (getattr(c, "text", "") or "").strip():
                continue
            if lang and (getattr(c, "lang", None) or "zh").strip().lower() != lang:
                continue
            cc = copy.copy(c)
            cc.source = "graph"
            chunks.append(cc)
            keys.append(aid)
            meta.append({"graph_depth": int(getattr(n, "graph_depth", 1) or 1),
                         "relations": list(getattr(n, "relations", []) or []),
                         "edge_conf": float(((getattr(n, "meta", {}) or {}).get("_edge_conf", 1.0)) or 1.0)})
        if not chunks:
            return []

        sem = self._semantic(question, chunks, keys)
        hits: List[RetrievalHit] = []
        for pos, (c, s, m) in enumerate(zip(chunks, sem, meta), start=1):
            dd, rw, conf = _depth_decay(m["graph_depth"], gamma=gamma), _relation_weight(m["relations"]), m["edge_conf"]
            final = float(s) * float(dd) * float(rw) * float(conf)
            hits.append(RetrievalHit(chunk=c, score=final, rank=pos, source="graph", score_breakdown={
                "channel": "graph", "semantic": float(s), "depth_decay": float(dd), "relation_weight": float(rw),
                "edge_conf": float(conf), "final": final, "graph_depth": m["graph_depth"], "relations": m["relations"]}))
        hits.sort(key=lambda h: float(h.score or 0.0), reverse=True)
        for r, h in enumerate(hits, start=1):
            h.rank = r
        return hits[:k]

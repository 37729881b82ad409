"""Hybrid orchestrator: dense + BM25 (+ ColBERT) -> fusion -> filter -> rerank.

Drop-in for legalrag/retrieval/hybrid_retriever.py:136-551 — same constructor
(`HybridRetriever(cfg)`, attributes `.cfg .dense .bm25 .colbert .graph`), same
methods (`search`, `search_dense/_bm25/_colbert/_graph`, `_fuse`), same
RetrievalHit / score_breakdown keys, same per-stage timing log line.  The
arithmetic of every stage runs in libamdretrieval kernels:
    channels      dense_retriever / bm25_retriever / colbert_retriever
    _fuse         amdr_fuse       (minmax, RRF, weighted blend, stable rank)
    filter        amdr_fuse's min_final_score count
    rerank blend  amdr_rerank_blend (minmax of CE scores, (1-b)s + b*norm, re-rank)
Host Python only moves ids/scores in and out and builds the hit objects.
`search_batch` is the throughput form (whole query batches stay in HBM).

Differences from the reference, all deliberate:
  * exactly tied fused scores keep first-appearance order (dense list, then
    bm25, then colbert) instead of Python set-iteration order
    (hybrid_retriever.py:460,484,526 — PYTHONHASHSEED dependent there);
  * the graph channel (graph_retriever.py) rescores the walked articles with a row
    gather + dot on the resident chunk matrix instead of re-embedding their text.
"""
from __future__ import annotations

import logging
import math
import threading
import time
import traceback
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Set

import numpy as np

from .. import _native
from ..config import graph_channel_mode, query_tokenizer_mode
from ..schemas import RetrievalHit
from .bm25_retriever import BM25Retriever
from .colbert_retriever import ColBERTRetriever
from .dense_retriever import DenseRetriever
from .diversity import Diversity, resolve as _resolve_diversity
from .facets import FacetCounts, Facets, build as _build_facets
from .graph_retriever import GraphRetriever
from .highlight import Highlight, HitHighlight, build as _build_highlight, pack_tables as _pack_slot_tables
from .highlight import slot_table as _slot_table
from .rerankers import RerankerFactory, _to_doc_text
from .scope import Scope, resolver_for
from .terms import Fuzzy, Near, NearOf, Phrase, PhraseOf, Prefix, Terms, Wildcard, Within, pack as _pack_terms  # noqa: F401 (NearOf, PhraseOf, Wildcard: re-exported)
from .vocab_match import Suggestion, collect_patterns as _collect_patterns  # noqa: F401 (Suggestion: re-exported)

logger = logging.getLogger("legalrag.retrieval.hybrid_retriever")

class HitText(str):
    """str(hit) as ONE string that also remembers its two parts: `head` ("chunk=<repr of the LawChunk>", the same str
    object for every hit of that chunk — nearly all of the text) and `tail` (the hit's own fields).  A scorer that
    tokenises its documents may cache per head; any other consumer sees a plain str."""
    __slots__ = ("head", "tail")

    def __new__(cls, head: str, tail: str):
        self = super().__new__(cls, head + tail)
        self.head, self.tail = head, tail
        return self


_CHUNK_REPR: Dict[int, Any] = {}  # id(LawChunk) -> (the chunk, repr(chunk)): see HybridRetriever._hit_text

CHANNELS = ("dense", "bm25", "colbert")
_HIT_FIELDS_SET = {"chunk", "score", "rank", "source", "score_breakdown"}


def _minmax(scores: Sequence[float]) -> List[float]:
    """hybrid_retriever.py:24-30 (host utility; the fused path uses the kernel)."""
    if not scores:
        return []
    lo, hi = min(scores), max(scores)
    if hi - lo < 1e-12:
        return [0.0 for _ in scores]
    return [(float(s) - lo) / (hi - lo) for s in scores]


def _as_channel_list(x: Any) -> List[str]:
    if x is None:
        return []
    if isinstance(x, (list, set, tuple)):
        return [str(i) for i in x]
    return [str(x)]


def _dedup_keep_best(hits: List[RetrievalHit]) -> List[RetrievalHit]:
    """Best-scoring hit per chunk.id, provenance unioned (hybrid_retriever.py:71-130).
    Channel unions are built in first-seen order (the reference goes through a set)."""
    best: Dict[str, RetrievalHit] = {}
    for h in hits:
        cid = h.chunk.id
        sb = h.score_breakdown or {}
        if cid not in best:
            if "channel" in sb:
                sb["channel"] = _as_channel_list(sb.get("channel"))
                h.score_breakdown = sb
            best[cid] = h
            continue
        cur = best[cid]
        sb_cur = cur.score_breakdown or {}
        merged: List[str] = []
        for c in _as_channel_list(sb_cur.get("channel")) + _as_channel_list(sb.get("channel")):
            if c not in merged:
                merged.append(c)
        contrib: Dict[str, float] = {}
        for src in (sb_cur.get("channel_contrib", {}) or {}, sb.get("channel_contrib", {}) or {}):
            for k, v in src.items():
                contrib[str(k)] = contrib.get(str(k), 0.0) + float(v)
        if float(h.score) > float(cur.score):
            best[cid] = h
        rep = best[cid]
        sb_rep = rep.score_breakdown or {}
        if contrib:
            merged.sort(key=lambda c: float(contrib.get(c, 0.0)), reverse=True)
            sb_rep["channel_contrib"] = contrib
        else:
            merged.sort()
        sb_rep["channel"] = merged
        rep.score_breakdown = sb_rep
    out = list(best.values())
    out.sort(key=lambda x: float(x.score), reverse=True)
    for i, h in enumerate(out, start=1):
        h.rank = i
    return out


def _is_graph_mode(mode: Any) -> bool:
    return bool(mode) and (str(mode).upper().endswith("GRAPH_AUGMENTED") or str(mode) == "RoutingMode.GRAPH_AUGMENTED")


class _NativeStage:
    """State of a retriever's device-resident stage: the compatibility key of the loaded indexes and its verdict
    (_native_channels), the engines by "with ColBERT" (rebuilt when the key changes) and the lock of one batch at a time."""

    def __init__(self) -> None:
        self.key, self.ok, self.engines, self.lock = None, False, {}, threading.Lock()


@dataclass
class _Prepared:
    """One batch ready for the device (HybridRetriever._prepare)."""
    native: Any    # (dense store, BM25 retriever, ColBERT retriever | None: channel off or its query encoder failed)
    q_emb: Any     # f32 [n, d] query embeddings on the device
    csr: Any       # the BM25 side as (q_terms i32, q_ptr i64) numpy arrays, or None when `text` is set
    text: Any      # ... or the UTF-8 views of a text batch (BM25Retriever.device_text_batch)
    exact: Any     # bool [n]: tokenised exactly (zh_exact)
    q_tok: Any     # the ColBERT query tokens (device tensor or numpy batch), or None
    stamps: Any    # (t_after_dense_prep, t_after_bm25_prep, t_after_colbert_prep) for search()'s log line


def _fetch_full(eng, res):  # ONE synchronise and ONE device-to-host copy (the four outputs share an allocation)
    return res.to_host()


# The columns of search_batch_arrays: (name, dtype, fill where a question or a hit has no result, shape of one hit's entry
# | None: one entry per question).  Whatever allocates a column (_column: the graph columns, the scatter of a split batch)
# reads this table.
COLUMNS = (
    ("rows", np.int64, -1, ()), ("scores", np.float64, 0.0, ()), ("count", np.int32, 0, None),
    ("channel_mask", np.int32, 0, ()), ("zh_exact", np.bool_, True, None), ("values", np.float64, 0.0, (_native.FUSE_NVALS,)),
    ("graph_rows", np.int64, -1, ()), ("graph_scores", np.float64, 0.0, ()), ("graph_semantic", np.float32, 0.0, ()),
    ("graph_depth", np.int32, 0, ()), ("graph_relation", np.int32, -1, ()), ("graph_edge_conf", np.float64, 0.0, ()),
    ("graph_count", np.int32, 0, None))


# ... and the two more of a diversified call with values=True (diversity=): per selected hit the winning MMR value and its
# largest cosine to the hits selected before it.
MMR_COLUMNS = (("mmr", np.float64, 0.0, ()), ("mmr_max_sim", np.float64, 0.0, ()))


def _column(n: int, top_k: int, dtype, fill, hit) -> np.ndarray:
    return np.full((n,) if hit is None else (n, top_k) + hit, fill, dtype=dtype)


@dataclass
class HybridRetriever:
    cfg: Any

    def __post_init__(self) -> None:
        self.dense = DenseRetriever(self.cfg)
        self.bm25 = BM25Retriever(self.cfg)
        self.colbert = None
        if getattr(self.cfg.retrieval, "enable_colbert", False):
            try:
                self.colbert = ColBERTRetriever.from_config(self.cfg)
            except Exception as e:  # noqa: BLE001 - channel-level swallow, as the reference (:163-169)
                print("[HybridRetriever] ColBERT init failed:", repr(e))
                traceback.print_exc()
                self.colbert = None
        self.graph = None
        if getattr(self.cfg.retrieval, "enable_graph", False):
            try:
                self.graph = GraphRetriever(self.cfg)
            except Exception:  # noqa: BLE001 - no graph file / no index: channel off, as the reference (:171-177)
                self.graph = None

    # ------------------------------------------------------------------ knobs
    def _knobs(self) -> Dict[str, Any]:
        r = self.cfg.retrieval
        return {
            "method": str(getattr(r, "fusion_method", "rrf_norm_blend")).lower(),
            "rrf_k": int(getattr(r, "rrf_k", 60)),
            "alpha": float(getattr(r, "rrf_alpha", 0.50)),
            "weights": {"dense": float(getattr(r, "dense_weight", 0.55)), "bm25": float(getattr(r, "bm25_weight", 0.35)),
                        "colbert": float(getattr(r, "colbert_weight", 0.25))},
        }

    def _params(self, kn: Dict[str, Any], min_final: float = -math.inf) -> "_native.FuseParams":
        w = kn["weights"]
        return _native.make_fuse_params(method=kn["method"], rrf_k=kn["rrf_k"], alpha=kn["alpha"], w_dense=w["dense"],
                                        w_bm25=w["bm25"], w_colbert=w["colbert"], min_final_score=min_final)

    # ------------------------------------------------------- per-channel APIs
    def _scope_workspace(self, device: int) -> "_native.ScopeWorkspace":
        """The workspace of the per-channel scoped searches (host-pointer calls: serialised inside the handle)."""
        held = self.__dict__.setdefault("_scope_ws", {})
        ws = held.get(int(device))
        if ws is None:
            ws = held[int(device)] = _native.ScopeWorkspace(device=int(device))
        return ws

    def _term_rows(self, who: str, chunks, scope: Optional[Scope], terms: Terms) -> np.ndarray:
        """The ascending rows of `chunks` that satisfy `terms` inside `scope` (None: the whole list), resolved on the GPU from
        the BM25 index's resident postings (amdr_term_scope, the host twin).  `chunks` must be the BM25 index's own chunk
        list or one with the same ids in the same order — a BM25 document id is then a row of it — and the index unsharded:
        ValueError otherwise, before any launch."""
        bm = self.bm25
        if not isinstance(bm, BM25Retriever):
            raise ValueError(f"{who}(terms=): term constraints need this package's own BM25 retriever")
        bm.load()
        if getattr(bm, "shard", None) is not None:
            raise ValueError(f"{who}(terms=): term constraints do not run on a row-sharded index")
        if chunks is not bm.chunks and not (len(chunks) == len(bm.chunks) and all(
                a is not None and a.id == b.id for a, b in zip(chunks, bm.chunks))):
            raise ValueError(f"{who}(terms=): this channel's chunk list is not the BM25 index's (a BM25 document id must "
                             f"be a row of the channel)")
        model = bm.bm25
        tt = _pack_terms([(scope, terms)], model.vocab(), model._doc_frequencies(), int(model.corpus_size),
                         resolver_for(bm.chunks).rows, model.sorted_vocab() if terms.has_union or terms.has_class_span or terms.has_within else None,
                         self._expansions(bm, [terms]))
        if tt.cand_max == 0:
            return np.zeros(0, dtype=np.int64)
        def check(status, name) -> None:
            """RuntimeError naming the first item whose status word is non-zero (name(i): the item; None: the constraint)."""
            if status.any():
                i = int(np.flatnonzero(status)[0])
                what = f"{name(i)!r}" if name is not None else "the term constraint"
                raise RuntimeError(f"{who}(terms=): {what} overflowed its bound (status {int(status[i])}); the "
                                   f"host model and the resident BM25 index disagree")

        def behind(lists, lp, docs):
            """The lists (lp, docs) of a step appended behind the array `lists` (None: they start it)."""
            if lists is None:
                return lp, docs
            return np.concatenate([lists[0], lists[0][-1] + lp[1:]]), np.concatenate([lists[1], docs])

        lists = None
        if tt.n_near:  # phrases and Nears in one span step, into one array of document lists
            bm.ensure_token_stream()
            lp, docs, p_status = bm.gpu_index().span_lists(*tt.span_ops, tt.span_cand_max, tt.span_rows_cap)
            check(p_status, tt.span_item)
            lists = behind(lists, lp, docs)
        elif tt.n_phr:  # the phrases first, into their own document lists: the virtual terms of the constraint
            bm.ensure_token_stream()
            lp, docs, p_status = bm.gpu_index().phrase_lists(tt.phr_ops[0], tt.phr_ops[1], tt.phr_cand_max, tt.phr_rows_cap)
            check(p_status, lambda p: tt.phrases[p])
            lists = behind(lists, lp, docs)
        if tt.n_union:  # the unions behind them, in the same arrays
            u_lp, u_docs, u_status = bm.gpu_index().union_lists(*tt.union_ops, tt.union_rows_cap)
            check(u_status, lambda u: tt.unions[u])
            lists = behind(lists, u_lp, u_docs)
        if tt.n_cspan:  # the class spans behind the unions: the twin resolves the classes it needs itself, in its own array
            bm.ensure_token_stream()
            c_ptr, c_slots, c_kind, c_dist = tt.cspan_ops
            first = len(model.vocab()) + tt.n_phr + tt.n_near  # union u is the twin's class u
            c_lp, c_docs, c_status = bm.gpu_index().class_spans(c_ptr, np.where(c_slots >= first, c_slots - (tt.n_phr + tt.n_near),
                                                                                 c_slots), c_kind, c_dist, *tt.union_ops,
                                                                 tt.cspan_cand_max, tt.cspan_rows_cap)
            check(c_status, lambda c: tt.cspans[c])
            lists = behind(lists, c_lp, c_docs)
        if tt.n_unit:  # the Withins behind the class spans: the twin resolves the classes it needs itself, as the class step's
            bm.ensure_breaks()
            w_ptr, w_slots, w_kind = tt.unit_ops
            first = len(model.vocab()) + tt.n_phr + tt.n_near  # union u is the twin's class u
            w_lp, w_docs, w_status = bm.gpu_index().unit_spans(w_ptr, np.where(w_slots >= first, w_slots - (tt.n_phr + tt.n_near),
                                                                               w_slots), w_kind, *tt.union_ops,
                                                               tt.unit_cand_max, tt.unit_rows_cap)
            check(w_status, lambda w: tt.units[w])
            lists = behind(lists, w_lp, w_docs)
        _, rows, status = bm.gpu_index().term_scope(tt.ops, tt.cand_max, tt.rows_cap, lists=lists)
        check(status[:1], None)
        return rows

    @staticmethod
    def _expansions(bm, terms: Sequence[Optional[Terms]]):
        """What terms.pack and highlight.slot_table take as `expansions`: the tokens each distinct Wildcard / Fuzzy of these
        Terms names, resolved on the GPU against the live vocabulary in one native call (BM25Retriever.vocab_matcher); None
        when they hold no pattern — nothing is launched then."""
        members = _collect_patterns(terms)
        return bm.vocab_matcher().expand(members) if members else None

    def phrase(self, text_: str) -> Phrase:
        """The Phrase of a string, cut by the BM25 index's DOCUMENT-side tokeniser (an English index lower-cases):
        retriever.phrase("Security Interest") == Phrase("security", "interest").  ValueError for a string without a token,
        with more than 16, or on an index that records no tokeniser."""
        bm = self.bm25
        if not isinstance(bm, BM25Retriever):
            raise ValueError("phrase(): phrases need this package's own BM25 retriever")
        toks = bm.document_tokens(text_)
        if not toks:
            raise ValueError(f"phrase(): {text_!r} holds no token")
        return Phrase(*toks)

    def near(self, text_: str, distance: int, ordered: bool = False) -> Near:
        """The Near of a string, cut by the BM25 index's DOCUMENT-side tokeniser as phrase() cuts it:
        retriever.near("Buyer Seller", distance=5) == Near("buyer", "seller", distance=5).  ValueError for a string with
        fewer than 2 or more than 8 tokens, a distance outside 1 .. 255, or on an index that records no tokeniser."""
        bm = self.bm25
        if not isinstance(bm, BM25Retriever):
            raise ValueError("near(): proximity constraints need this package's own BM25 retriever")
        return Near(*bm.document_tokens(text_), distance=distance, ordered=ordered)

    def within(self, text_: str, unit: str = "sentence", ordered: bool = False) -> Within:
        """The Within of a string, cut by the BM25 index's DOCUMENT-side tokeniser as near() cuts it:
        retriever.within("Buyer Seller", unit="sentence") == Within("buyer", "seller", unit="sentence").  ValueError for a
        string with fewer than 2 or more than 8 tokens, an unknown unit, or on an index that records no tokeniser."""
        bm = self.bm25
        if not isinstance(bm, BM25Retriever):
            raise ValueError("within(): sentence and paragraph connectors need this package's own BM25 retriever")
        return Within(*bm.document_tokens(text_), unit=unit, ordered=ordered)

    def prefix(self, text_: str) -> Prefix:
        """The Prefix of a string, cut by the BM25 index's DOCUMENT-side tokeniser as phrase() cuts it:
        retriever.prefix("Sell") == Prefix("sell").  ValueError unless the string yields exactly one token, or on an index
        that records no tokeniser."""
        bm = self.bm25
        if not isinstance(bm, BM25Retriever):
            raise ValueError("prefix(): root expanders need this package's own BM25 retriever")
        toks = bm.document_tokens(text_)
        if len(toks) != 1:
            raise ValueError(f"prefix(): {text_!r} holds {len(toks)} tokens; a stem is exactly one")
        return Prefix(toks[0])

    def fuzzy(self, text_: str, edits: int = 1) -> Fuzzy:
        """The Fuzzy of a string, cut by the BM25 index's DOCUMENT-side tokeniser as prefix() cuts it:
        retriever.fuzzy("Warrenty", edits=1) == Fuzzy("warrenty", edits=1).  ValueError unless the string yields exactly
        one token, or on an index that records no tokeniser.  (There is no wildcard(): a tokeniser would cut at '?'.)"""
        bm = self.bm25
        if not isinstance(bm, BM25Retriever):
            raise ValueError("fuzzy(): vocabulary patterns need this package's own BM25 retriever")
        toks = bm.document_tokens(text_)
        if len(toks) != 1:
            raise ValueError(f"fuzzy(): {text_!r} holds {len(toks)} tokens; a Fuzzy is exactly one")
        return Fuzzy(toks[0], edits=edits)

    def suggest_batch(self, words: Sequence[str], edits: int = 2, top: int = 5) -> List[tuple]:
        """"Did you mean": per word a tuple of Suggestion(token, distance, doc_freq) — the vocabulary tokens within `edits`
        of the word as fuzzy() cuts it, by (distance ascending, document frequency descending, token ascending); the word
        itself comes first, at distance 0, when the vocabulary holds it.  A word no longer than `edits` takes len(word) - 1
        edits (one character: only itself), so a short word never fails the batch.  Document frequencies are the host
        model's; ONE native call serves the batch.  Preconditions as search_*(terms=): this package's own BM25 retriever
        on an unsharded index (ValueError before any launch)."""
        bm = self.bm25
        if not isinstance(bm, BM25Retriever):
            raise ValueError("suggest(): vocabulary patterns need this package's own BM25 retriever")
        bm.load()
        if getattr(bm, "shard", None) is not None:
            raise ValueError("suggest(): vocabulary patterns do not run on a row-sharded index")
        words = list(words)
        if not words:
            return []
        cut = []
        for w in words:
            toks = bm.document_tokens(w)
            if len(toks) != 1:
                raise ValueError(f"suggest(): {w!r} holds {len(toks)} tokens; a word is exactly one")
            cut.append(toks[0])
        return list(bm.vocab_matcher().suggest_batch(cut, bm.bm25._doc_frequencies(), edits=edits, top=top))

    def suggest(self, word: str, edits: int = 2, top: int = 5) -> tuple:
        """The one-word form of suggest_batch."""
        return self.suggest_batch([word], edits=edits, top=top)[0]

    # ------------------------------------------------------------------ facets
    def _facet_engine(self, bm):
        """The engine of the facet calls: the BM25 index alone (the constraints are resolved on its postings, the table and
        the code columns are rows of its chunk list).  Made again when the index is reloaded or updated in place."""
        from .engine import HybridEngine
        gpu = bm.gpu_index()
        key = (id(gpu), id(bm.bm25), getattr(bm, "appends", 0))
        held = self.__dict__.get("_facet_eng")
        if held is None or held[0] != key:
            held = self.__dict__["_facet_eng"] = (key, HybridEngine(None, gpu, None,
                                                                    device=int(getattr(self.cfg.retrieval, "device", 0))))
        return held[1]

    def facets_batch(self, *, terms: Optional[Sequence[Optional[Terms]]] = None, scopes: Optional[Sequence[Optional[Scope]]] = None,
                     spec: Facets = Facets(), _who: str = "facets_batch") -> List[FacetCounts]:
        """One FacetCounts per (scope, terms) pair: how many chunks of the BM25 index's chunk list lie in scopes[i] (None:
        all) and satisfy terms[i] (None: no constraint), and how they spread over the fields of `spec`.  The constraints are
        resolved on the GPU (HybridEngine.term_scopes; without any `terms` the scopes' own rows are uploaded), counted there
        (HybridEngine.facet_counts) and only the counts come back; equal pairs of a batch are resolved once.  With `terms`
        the preconditions and errors are those of search_*(terms=): this package's own BM25 retriever on an unsharded index
        (ValueError before any launch), RuntimeError for a non-zero status word."""
        if not isinstance(spec, Facets):
            raise TypeError(f"{_who}: spec must be a Facets, got {type(spec).__name__}")
        if terms is None and scopes is None:
            raise ValueError(f"{_who}: give terms, scopes or both (one entry per pair)")
        n = len(terms) if terms is not None else len(scopes)
        if scopes is not None and len(scopes) != n:
            raise ValueError(f"{_who}: scopes must have one entry per pair")
        for i, s in enumerate(scopes if scopes is not None else ()):
            if s is not None and not isinstance(s, Scope):
                raise TypeError(f"{_who}: scopes[{i}] is not a Scope")
        no_terms = self._no_terms(terms, _who)
        bm = self.bm25
        if not isinstance(bm, BM25Retriever):
            raise ValueError(f"{_who}(terms=): term constraints need this package's own BM25 retriever")
        bm.load()
        if getattr(bm, "shard", None) is not None:
            raise ValueError(f"{_who}(terms=): term constraints do not run on a row-sharded index")
        if n == 0:
            return []
        resolver = resolver_for(bm.chunks)
        cols, values = resolver.code_columns(spec.by)
        pairs = [(scopes[i] if scopes is not None else None, (terms[i] if terms is not None else None) or Terms())
                 for i in range(n)]
        tt = None
        if no_terms:
            sp, rows, qscope, _ = resolver.table([s if s is not None else Scope() for s, _ in pairs])
        else:
            model = bm.bm25
            tt = _pack_terms(pairs, model.vocab(), model._doc_frequencies(), int(model.corpus_size), resolver.rows,
                             model.sorted_vocab() if any(t.has_union or t.has_class_span or t.has_within for _, t in pairs) else None,
                             self._expansions(bm, [t for _, t in pairs]))
            if tt.n_phr or tt.n_near or tt.n_cspan:
                bm.ensure_token_stream()
            if tt.n_unit:
                bm.ensure_breaks()
            qscope = np.asarray(tt.qscope)
        import torch
        with self._stage().lock:
            eng = self._facet_engine(bm)
            eng.check_facets()
            with torch.cuda.device(eng.tdev):
                if tt is None:
                    table, pin = eng.upload_scopes(sp, rows, qscope, channel=1), None
                else:
                    table, st = eng.term_scopes(tt)
                    pin = eng._pinned("fcst", 4 * max(int(st.numel()), 1))[:4 * int(st.numel())]
                    pin.copy_(st.view(torch.uint8), non_blocking=True)
                got = eng.facet_counts(table, cols, [len(v) for v in values], spec.top)()
            if pin is not None:  # (fetch has waited for an event recorded behind the copy)
                status = pin.numpy().view(np.int32)
                if status.any():
                    i = int(np.flatnonzero(status)[0])
                    what = "the term constraint" if i < int(tt.n_cons) else f"{tt.list_item(i - int(tt.n_cons))!r}"
                    raise RuntimeError(f"{_who}(terms=): {what} overflowed its bound (status {int(status[i])}); the "
                                       f"host model and the resident BM25 index disagree")
        per_cons = _build_facets(spec, values, *got)
        return [per_cons[int(j)] for j in qscope]

    def facets(self, *, terms: Optional[Terms] = None, scope: Optional[Scope] = None, spec: Facets = Facets()) -> FacetCounts:
        """The one-pair form of facets_batch."""
        return self.facets_batch(terms=[terms], scopes=[scope], spec=spec, _who="facets")[0]

    def count_batch(self, *, terms: Optional[Sequence[Optional[Terms]]] = None,
                    scopes: Optional[Sequence[Optional[Scope]]] = None) -> List[int]:
        """How many chunks each (scope, terms) pair matches: the totals of facets_batch."""
        return [f.total for f in self.facets_batch(terms=terms, scopes=scopes, spec=Facets(by=("law_name",), top=1),
                                                   _who="count_batch")]

    def count(self, *, terms: Optional[Terms] = None, scope: Optional[Scope] = None) -> int:
        """How many chunks lie in `scope` (None: all) and satisfy `terms` (None: no constraint)."""
        return self.facets_batch(terms=[terms], scopes=[scope], spec=Facets(by=("law_name",), top=1), _who="count")[0].total

    # ------------------------------------------------------------- highlighting
    def highlight(self, question: str, hits: Sequence[Any], *, terms: Optional[Terms] = None,
                  spec: Highlight = Highlight()) -> List[Optional[HitHighlight]]:
        """The one-question form of highlight_batch: one HitHighlight (or None) per hit."""
        return self.highlight_batch([question], [hits], terms=None if terms is None else [terms], spec=spec)[0]

    def highlight_batch(self, questions: Sequence[str], hits_lists: Sequence[Sequence[Any]],
                        terms: Optional[Sequence[Optional[Terms]]] = None,
                        spec: Highlight = Highlight()) -> List[List[Optional[HitHighlight]]]:
        """Marks and the best passage of every hit (retrieval/highlight.py): for question i and each hit of hits_lists[i]
        — a RetrievalHit, or anything with a `.chunk` — the tokens of the chunk that the question and terms[i] name and the
        window of spec.window tokens that holds the most of them, resolved on the GPU from the BM25 index's resident token
        stream in ONE native call for the batch (amdr_bm25_marks).  A chunk the BM25 index does not hold gets None.  The
        chunk text is the index's own (after a live replace: the new text).  ValueError on a row-sharded index or a
        foreign BM25 retriever, as phrase()."""
        bm = self.bm25
        if not isinstance(bm, BM25Retriever):
            raise ValueError("highlight(): highlighting needs this package's own BM25 retriever")
        if not isinstance(spec, Highlight):
            raise TypeError(f"highlight(): spec is a Highlight, got {type(spec).__name__}")
        questions, hits_lists = list(questions), [list(h) for h in hits_lists]
        if len(hits_lists) != len(questions) or (terms is not None and len(terms) != len(questions)):
            raise ValueError("highlight_batch(): one hit list (and one Terms or None) per question")
        bm.load()
        if getattr(bm, "shard", None) is not None:
            raise ValueError("highlight(): highlighting does not run on a row-sharded index")
        bm.ensure_token_stream()
        model = bm.bm25
        vocab = model.vocab()
        held = self.__dict__.get("_highlight_rows")
        if held is None or held[0] is not bm.chunks or held[1] != (len(bm.chunks), bm.appends):
            held = self.__dict__["_highlight_rows"] = (bm.chunks, (len(bm.chunks), bm.appends),
                                                       {c.id: r for r, c in enumerate(bm.chunks)})
        row_of = held[2]
        sorted_vocab = None
        expansions = None if terms is None else self._expansions(bm, terms)
        tables = []
        for i, q in enumerate(questions):
            t = None if terms is None else terms[i]
            if t is not None and sorted_vocab is None and (t.has_union or t.has_class_span or t.has_within):
                sorted_vocab = model.sorted_vocab()
            tables.append(_slot_table(bm.document_tokens(q) if spec.question else [], t, vocab, model.idf, sorted_vocab or (),
                                      expansions))
        k = max((len(h) for h in hits_lists), default=0)
        out: List[List[Optional[HitHighlight]]] = [[None] * len(h) for h in hits_lists]
        if not questions or k == 0:
            return out
        docs = np.full((len(questions), k), -1, dtype=np.int64)
        for i, hits in enumerate(hits_lists):
            for j, h in enumerate(hits):
                chunk = getattr(h, "chunk", None)
                docs[i, j] = row_of.get(getattr(chunk, "id", None), -1)
        g = bm.gpu_index()
        win, score, slots, marks, status = g.marks(docs, *_pack_slot_tables(tables), spec.window, spec.marks)
        lowered = bm.index_tokenizer == "en_regex"
        cut: Dict[int, Any] = {}
        for i, hits in enumerate(hits_lists):
            for j in range(len(hits)):
                r = int(docs[i, j])
                if r < 0:
                    continue
                if r not in cut:
                    txt = bm.chunks[r].text
                    cut[r] = (txt, bm.document_tokens(txt))
                txt, toks = cut[r]
                out[i][j] = _build_highlight(tables[i], spec, win[i, j], score[i, j], slots[i, j], marks[i, j], int(status[i, j]),
                                             txt, toks, lowered, int(model.doc_len[r]))
        return out

    def _highlight_stage(self, questions: Sequence[str], outs: List[List[RetrievalHit]], terms, spec: Highlight) -> None:
        """search(highlight=) / search_batch(highlight=): behind every ranking stage, each hit's HitHighlight.as_dict() (or
        None) at hit.score_breakdown["highlight"]."""
        for hits, hls in zip(outs, self.highlight_batch(questions, outs, terms=terms, spec=spec)):
            for h, hl in zip(hits, hls):
                h.score_breakdown["highlight"] = None if hl is None else hl.as_dict()

    def _search_scoped(self, who: str, chunks, scope: Optional[Scope], top_k: int, refusal: Optional[str], device, twin: str,
                       operands, terms: Optional[Terms] = None):
        """The common sequence of the per-channel scoped searches: [(chunk, score)] of the channel's top_k among the rows of
        `chunks` the scope names.  A scope that matches nothing returns [] without a launch, even where the index would be
        refused; `refusal`: the channel's error text when its index cannot take a scope, else None; `twin`: the channel's
        host twin (a ScopeWorkspace method), called on a one-scope table with what `operands()` returns: (index, queries).
        `terms`: the rows are those of `scope` (None: all) that satisfy the term constraint (_term_rows)."""
        rows = resolver_for(chunks).rows(scope) if terms is None else self._term_rows(who, chunks, scope, terms)
        if rows.size == 0:
            return []
        if refusal is not None:
            raise ValueError(refusal)
        if top_k > _native.MAX_K:
            raise ValueError(f"{who}: a scoped search ranks at most {_native.MAX_K} hits per channel, got top_k={top_k}")
        scores, ids = getattr(self._scope_workspace(device), twin)(*operands(), [0, rows.size], rows, [0], top_k)
        return [(chunks[r], float(s)) for r, s in zip(ids[0].tolist(), scores[0].tolist()) if r >= 0 and chunks[r] is not None]

    def _search_dense_scoped(self, question: str, top_k: int, scope: Optional[Scope],
                             terms: Optional[Terms] = None) -> List[RetrievalHit]:
        store = self.dense.store
        store.load()
        index = getattr(store.index, "native", None)
        pairs = self._search_scoped(
            "search_dense", store.chunks, scope, top_k,
            "search_dense(scope=): needs this package's own, unsharded dense index"
            if index is None or getattr(store.index, "spec", None) is not None else None,
            getattr(index, "device", 0), "dense_search", lambda: (index, store._embed([question], is_query=True)), terms)
        return [RetrievalHit(chunk=c, score=s, rank=j, source="retriever", semantic_score=s)
                for j, (c, s) in enumerate(pairs, start=1)]

    def search_dense(self, question: str, top_k: int = 10, *, scope: Optional[Scope] = None,
                     terms: Optional[Terms] = None) -> List[RetrievalHit]:
        """`scope`: rank only that part of the corpus (retrieval/scope.py); None: the whole corpus.  `terms`: rank only the
        chunks that satisfy the term constraint (retrieval/terms.py), inside `scope` if both are given."""
        top_k = max(1, int(top_k))
        terms = None if self._no_terms(None if terms is None else [terms], "search_dense") else terms
        hits = (self.dense.search(question, top_k) if scope is None and terms is None
                else self._search_dense_scoped(question, top_k, scope, terms))
        hits.sort(key=lambda h: float(h.score), reverse=True)
        for i, h in enumerate(hits, start=1):
            h.rank = i
            h.source = "retriever"
            h.score_breakdown = {"channel": ["dense"], "dense_raw": float(h.score)}
        return hits

    def _search_bm25_scoped(self, question: str, top_k: int, tokens: Optional[Sequence[str]], scope: Optional[Scope],
                            terms: Optional[Terms] = None):
        bm = self.bm25
        bm.load()

        def operands():
            if tokens is not None:
                terms = list(tokens)
                bm._tls.exact = True
            else:
                terms = bm.tokenize_query(question)
            return bm.gpu_index(), [bm.bm25.term_ids(terms)]
        return self._search_scoped(
            "search_bm25", bm.chunks, scope, top_k,
            "search_bm25(scope=): scoped search does not run on a row-sharded index" if getattr(bm, "shard", None) is not None
            else None, bm.device_index, "bm25_search", operands, terms)

    def search_bm25(self, question: str, top_k: int = 10, tokens: Optional[Sequence[str]] = None, *,
                    scope: Optional[Scope] = None, terms: Optional[Terms] = None) -> List[RetrievalHit]:
        """`tokens`: the caller's own segmentation of `question` (exact path without jieba).  `scope`: rank only that
        part of the corpus (idf and avgdl stay those of the whole index).  `terms`: rank only the chunks that satisfy the
        term constraint (retrieval/terms.py), inside `scope` if both are given; the scores do not change."""
        top_k = max(1, int(top_k))
        terms = None if self._no_terms(None if terms is None else [terms], "search_bm25") else terms
        # (a duck-typed retriever with the reference's two-argument search() is still accepted)
        if scope is not None or terms is not None:
            pairs = self._search_bm25_scoped(question, top_k, tokens, scope, terms)
        else:
            pairs = self.bm25.search(question, top_k, tokens=tokens) if tokens is not None else self.bm25.search(question, top_k)
        hits = [RetrievalHit(chunk=c, score=float(s), rank=i, source="retriever",
                             score_breakdown={"channel": ["bm25"], "bm25_raw": float(s)})
                for i, (c, s) in enumerate(pairs, start=1)]
        hits.sort(key=lambda h: float(h.score), reverse=True)
        inexact = not getattr(self.bm25, "zh_exact", True)  # stand-in tokenizer ran: never unmarked (text.py)
        for i, h in enumerate(hits, start=1):
            h.rank = i
            if inexact:
                h.score_breakdown["zh_exact"] = False
        return hits

    def _search_colbert_scoped(self, question: str, top_k: int, scope: Optional[Scope], terms: Optional[Terms] = None):
        col = self.colbert
        if not col.enabled:
            return []
        col._load_meta_and_collection()
        question = (question or "").strip()
        if not question:
            return []
        held = self.__dict__.get("_colbert_chunks")
        if held is None or held[0] is not col._pid2chunk:  # the ColBERT row space as a list: pid -> chunk (None: no such pid)
            held = self.__dict__["_colbert_chunks"] = (col._pid2chunk,
                                                       [col._pid2chunk.get(i) for i in range(max(col._pid2chunk) + 1)])
        return self._search_scoped(
            "search_colbert", held[1], scope, top_k,
            "search_colbert(scope=): scoped search does not run on a row-sharded index" if getattr(col, "shard", None) is not None
            else None, col.device_index, "maxsim_search",
            lambda: (col._searcher, np.asarray(col._encoder.encode_query(question), dtype=np.float32)[None]), terms)

    def search_colbert(self, question: str, top_k: int = 10, *, scope: Optional[Scope] = None,
                       terms: Optional[Terms] = None) -> List[RetrievalHit]:
        top_k = max(1, int(top_k))
        terms = None if self._no_terms(None if terms is None else [terms], "search_colbert") else terms
        if self.colbert is None:
            return []
        try:
            hits: List[RetrievalHit] = []
            for item in (self.colbert.search(question, top_k) if scope is None and terms is None
                         else self._search_colbert_scoped(question, top_k, scope, terms)):
                if isinstance(item, RetrievalHit):
                    hits.append(item)
                else:
                    c, s = item
                    hits.append(RetrievalHit(chunk=c, score=float(s), rank=0, source="retriever",
                                             score_breakdown={"channel": ["colbert"], "colbert_raw": float(s)}))
            hits.sort(key=lambda h: float(h.score), reverse=True)
            for i, h in enumerate(hits, start=1):
                h.rank = i
                h.source = "retriever"
                sb = h.score_breakdown or {}
                sb["channel"] = _as_channel_list(sb.get("channel")) or ["colbert"]
                sb.setdefault("colbert_raw", float(h.score))
                h.score_breakdown = sb
            return hits
        except Exception:  # noqa: BLE001 - reference swallows channel errors (:244-245)
            return []

    def search_graph(self, question: str, top_k: int = 10, *, decision: Any = None,
                     seeds: Optional[List[RetrievalHit]] = None) -> List[RetrievalHit]:
        """Graph hits for the seeds (hybrid_retriever.py:247-277): without seeds, the three
        channels' own top graph_seed_k each; hits come back re-sorted, renumbered, relabelled
        source="retriever" with channel ["graph"]; any failure -> []."""
        top_k = max(1, int(top_k))
        if self.graph is None:
            return []
        if seeds is None:
            seed_n = int(getattr(self.cfg.retrieval, "graph_seed_k", max(10, top_k * 3)))
            seeds = (self.search_dense(question, seed_n)[:seed_n] + self.search_bm25(question, seed_n)[:seed_n]
                     + self.search_colbert(question, seed_n)[:seed_n])
        try:
            hits = self.graph.search(question, seeds, decision=decision, top_k=top_k)
            hits.sort(key=lambda h: float(h.score), reverse=True)
            for i, h in enumerate(hits, start=1):
                h.rank = i
                h.source = "retriever"
                sb = h.score_breakdown or {}
                sb["channel"] = _as_channel_list(sb.get("channel")) or ["graph"]
                h.score_breakdown = sb
            return hits
        except Exception:  # noqa: BLE001
            return []

    # -------------------------------------------------------------- fusion
    def _fuse(self, *, dense_hits: List[RetrievalHit], bm25_hits: List[RetrievalHit],
              colbert_hits: List[RetrievalHit]) -> List[RetrievalHit]:
        return self._fuse_kept(dense_hits, bm25_hits, colbert_hits, -math.inf)[0]

    def _fuse_kept(self, dense_hits: List[RetrievalHit], bm25_hits: List[RetrievalHit],
                   colbert_hits: List[RetrievalHit], min_final: float):
        """(every fused hit, how many of them score >= min_final: the list is sorted, so they are a prefix)."""
        kn = self._knobs()
        lists = {"dense": dense_hits, "bm25": bm25_hits, "colbert": colbert_hits}
        for name, hs in lists.items():
            if len(hs) > _native.MAX_K:  # never truncated silently: the fused list would change
                raise ValueError(f"_fuse: {len(hs)} {name} hits exceed the fusion kernel's limit of {_native.MAX_K} per "
                                 f"channel (cfg.retrieval.top_k / top_k too deep)")
            hs.sort(key=lambda h: float(h.score), reverse=True)
        # corpus-wide integer uid per chunk.id for this call; chunk lookup prefers
        # dense -> bm25 -> colbert (setdefault order, hybrid_retriever.py:426-429)
        uid_of: Dict[str, int] = {}
        chunk_of: List[Any] = []
        for h in dense_hits + bm25_hits + colbert_hits:
            if h.chunk.id not in uid_of:
                uid_of[h.chunk.id] = len(chunk_of)
                chunk_of.append(h.chunk)
        if not chunk_of:
            return [], 0

        def arr(hs: List[RetrievalHit]):
            # a repeated id inside one channel keeps its first (best-ranked) entry
            seen: Set[int] = set()
            ids, sc = [], []
            for h in hs:
                u = uid_of[h.chunk.id]
                if u in seen:
                    continue
                seen.add(u)
                ids.append(u)
                sc.append(float(h.score))
            if not ids:
                return None
            return np.asarray([ids], dtype=np.int64), np.asarray([sc], dtype=np.float64)

        ids, vals, mask, count = _native.fuse(self._params(kn, min_final), 1, arr(dense_hits), arr(bm25_hits),
                                              arr(colbert_hits))
        hits = self._hits_from_native(ids[0], vals[0], mask[0], ids.shape[1], kn, chunk_of)
        if any((h.score_breakdown or {}).get("zh_exact") is False for h in bm25_hits):
            for h in hits:  # the stand-in tokenizer's mark survives fusion (text.py)
                h.score_breakdown["zh_exact"] = False
        return hits, int(count[0])

    @staticmethod
    def _hits_from_native(ids, vals, mask, n, kn, chunk_of) -> List[RetrievalHit]:
        out: List[RetrievalHit] = []
        n = int(n)
        # one conversion of the rows to Python scalars (per-element float(np.float64) was a third of this function)
        idl, vl, ml = ids[:n].tolist(), vals[:n].tolist(), mask[:n].tolist()
        method, rrf_k, alpha, weights = kn["method"], int(kn["rrf_k"]), float(kn["alpha"]), kn["weights"]
        fv = _native.FV
        i_s, i_rn, i_ws = fv["score"], fv["rrf_norm"], fv["weighted_sum"]
        i_n = (fv["dense_norm"], fv["bm25_norm"], fv["colbert_norm"])
        i_c = (fv["contrib_dense"], fv["contrib_bm25"], fv["contrib_colbert"])
        for r in range(n):
            i = idl[r]
            if i < 0:
                break
            v, m = vl[r], ml[r]
            contrib = {"dense": v[i_c[0]], "bm25": v[i_c[1]], "colbert": v[i_c[2]]}
            members = [ch for c, ch in enumerate(CHANNELS) if m & (1 << c)]
            if len(members) > 1:
                members.sort(key=lambda c: (contrib[c], c), reverse=True)
            sb = {
                "fusion_method": method, "rrf_k": rrf_k, "alpha": alpha, "channel_weights": dict(weights),
                "channel": members, "channel_contrib": contrib, "rrf_norm": v[i_rn], "weighted_sum": v[i_ws],
                "dense_norm": v[i_n[0]], "bm25_norm": v[i_n[1]], "colbert_norm": v[i_n[2]],
            }
            # model_construct: the fields come straight from the kernels' typed outputs and the store's own LawChunk
            # objects — the validating constructor was a third of a batch's host time (validate_python per hit)
            # (every field named: model_construct otherwise resolves each missing default per hit; _fields_set = the
            # five the validating constructor would have been given)
            out.append(RetrievalHit.model_construct(_HIT_FIELDS_SET, chunk=chunk_of[i], score=v[i_s], rank=r + 1,
                                                    source="retriever", semantic_score=None, graph_depth=None,
                                                    relations=None, seed_article_id=None, score_breakdown=sb))
        return out

    def _eff_depth(self, top_k: int, who: str) -> int:
        """Per-channel depth max(cfg.retrieval.top_k, top_k) (hybrid_retriever.py:289-292).  Beyond the fusion
        kernel's limit search(), search_batch() and search_batch_arrays() all refuse with ONE clear error — no
        NativeError from one channel, fallback in another and silent clamp in a third, and no host-side fuse
        (the product has no CPU path); the per-channel searches themselves accept any depth."""
        rcfg = self.cfg.retrieval
        eff = int(getattr(rcfg, "top_k", top_k * 8) or (top_k * 8))
        eff = max(eff, top_k)
        if eff > _native.MAX_K:
            raise ValueError(f"HybridRetriever.{who}: per-channel depth {eff} (max(cfg.retrieval.top_k, top_k)) "
                             f"exceeds the fusion kernel's limit of {_native.MAX_K} hits per channel")
        return eff

    # ---------------------------------------------------------- main search
    def search(self, question: str, llm: Any = None, top_k: int = 10, decision: Any = None, *,
               scope: Optional[Scope] = None, diversity: Any = None, terms: Optional[Terms] = None,
               highlight: Optional[Highlight] = None) -> List[RetrievalHit]:
        """`scope` (retrieval/scope.py): every channel ranks only that part of the corpus and the fusion normalises over
        those lists — the one-question form of search_batch(scopes=).  None: the whole corpus.
        `terms` (retrieval/terms.py): every channel ranks only the chunks whose text holds the required and none of the
        excluded tokens, inside `scope` if both are given — the one-question form of search_batch(terms=).
        `diversity` (retrieval/diversity.py): a Diversity makes MMR selection the last stage, None takes the configured
        default (cfg.retrieval.diversity_lambda), False switches it off.
        `highlight` (retrieval/highlight.py): a Highlight marks the query's words in every returned hit and picks its best
        passage, behind every ranking stage; the result is hit.score_breakdown["highlight"].  None: nothing changes."""
        if highlight is not None and not isinstance(highlight, Highlight):
            raise TypeError(f"search(highlight=) is a Highlight or None, got {type(highlight).__name__}")
        if scope is not None or (terms is not None and not self._no_terms([terms], "search")):
            return self.search_batch([question], top_k=top_k, llm=llm, decisions=None if decision is None else [decision],
                                     scopes=None if scope is None else [scope], diversity=diversity,
                                     terms=None if terms is None else [terms], highlight=highlight)[0]
        rcfg = self.cfg.retrieval
        top_k = max(1, int(top_k))
        mmr = self._diversity(diversity, top_k, "search")
        has_gpu = _native.device_count() > 0
        t_start = time.time()
        eff_top_k = self._eff_depth(top_k, "search")

        min_final = float(getattr(rcfg, "min_final_score", 0.0))
        native = self._native_channels(eff_top_k)
        if native is not None:
            # device-resident form: query vectors up, dense / BM25 / MaxSim top-k -> fuse -> filter on ONE
            # stream, ONE synchronise, one set of copies back (the kernels and results are those of the
            # per-channel path below; tests pin the two against each other)
            t0 = time.time()
            parts, _ = self._partition([question], None, None, native[0].chunks, native[2] is not None, "search")
            outs, (t1, t2, t3), _ = self._hit_lists([question], parts, eff_top_k, native, min_final)
            fused = outs[0]
            t4 = time.time()
        else:
            t0 = time.time()
            dense_hits = self.search_dense(question, eff_top_k)
            t1 = time.time()
            bm25_hits = self.search_bm25(question, eff_top_k)
            t2 = time.time()
            colbert_hits = self.search_colbert(question, eff_top_k)
            t3 = time.time()

            all_fused, kept = self._fuse_kept(dense_hits, bm25_hits, colbert_hits, min_final)
            fused = all_fused[:kept]  # hits with score >= min_final_score
            t4 = time.time()

        t_graph = None
        if getattr(rcfg, "enable_graph", False) and _is_graph_mode(getattr(decision, "mode", None)):
            # the fused list is cut to the seeds even when the graph channel is off (:317-320)
            seed_n = int(getattr(rcfg, "graph_seed_k", max(10, top_k * 3)))
            seeds = fused[:seed_n]
            fused = seeds + self.search_graph(question, eff_top_k, decision=decision, seeds=seeds)
            t_graph = time.time()

        t_rerank = None
        if getattr(rcfg, "enable_rerank", False):
            fused = self._rerank_stage([question], [fused], llm, top_k)[0]
            t_rerank = time.time()

        fused = _dedup_keep_best(fused)
        if mmr is not None:
            fused = self._mmr_stage([fused], top_k, *mmr)[0]
        t_end = time.time()

        def ms(a, b):
            return int((b - a) * 1000)
        logger.info(
            "[retrieval] dense=%dms bm25=%dms colbert=%dms fuse=%dms graph=%dms rerank=%dms total=%dms "
            "enabled(graph=%s,colbert=%s, has_gpu=%s)",
            ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t4, t_graph) if t_graph else 0,
            ms((t_graph or t4), t_rerank) if t_rerank else 0, ms(t_start, t_end),
            int(bool(getattr(rcfg, "enable_graph", False))), int(self.colbert is not None), int(has_gpu))
        fused = fused[:top_k]
        if highlight is not None:
            self._highlight_stage([question], [fused], None, highlight)
        return fused

    # ------------------------------------------------------- diversification
    def _diversity(self, diversity: Any, top_k: int, who: str):
        """(Diversity, pool) of a call, or None when the stage is off — and every refusal, before anything is launched:
        top_k beyond the kernel's pool, a row-sharded index, no dense index of this package's own on the GPU."""
        div = _resolve_diversity(diversity, self.cfg.retrieval)
        if div is None:
            return None
        try:
            pool = div.pool_for(top_k)
        except ValueError as e:
            raise ValueError(f"HybridRetriever.{who}: {e}") from None
        index = None
        store = getattr(self.dense, "store", None)
        if store is not None:
            try:
                store.load()
                index = getattr(store, "index", None)
            except Exception:  # noqa: BLE001 - reported as "no index" below
                index = None
        if index is not None and getattr(index, "spec", None) is not None:
            raise ValueError(f"HybridRetriever.{who}: diversity (MMR selection) does not run on a row-sharded index "
                             f"(the candidate rows are global)")
        if index is None or getattr(index, "native", None) is None:
            raise ValueError(f"HybridRetriever.{who}: diversity (MMR selection) needs this package's own dense index "
                             f"resident on the GPU: the cosine is taken between its rows, and there is no CPU path")
        return div, pool

    def _mmr_stage(self, lists: List[List[RetrievalHit]], top_k: int, div: Diversity, pool: int) -> List[List[RetrievalHit]]:
        """The last stage of the hit-object paths, behind _dedup_keep_best (which re-sorts by score): MMR selection over the
        first `pool` hits of every list in ONE batched call (amdr_mmr).  relevance = hit.score, candidate row = the chunk's
        row of the dense store (-1: a chunk the store does not hold has no vector and is similar to nothing).  Returns the
        selected hits in selection order, cut to top_k: rank renumbered, score untouched, score_breakdown gains "mmr" and
        "mmr_max_sim"."""
        nq = len(lists)
        if nq == 0:
            return lists
        store = self.dense.store
        row_of = resolver_for(store.chunks).row_of
        rows = np.full((nq, pool), -1, dtype=np.int64)
        rel = np.zeros((nq, pool), dtype=np.float64)
        count = np.zeros(nq, dtype=np.int32)
        for q, hits in enumerate(lists):
            m = count[q] = min(len(hits), pool)
            rows[q, :m] = [row_of(h.chunk.id) for h in hits[:m]]
            rel[q, :m] = [float(h.score) for h in hits[:m]]
        pos, val, sim, cnt = store.index.native.mmr(rows, rel, count, pool, min(top_k, pool), div.lam)
        outs = []
        for q, hits in enumerate(lists):
            out = []
            for j in range(int(cnt[q])):
                h = hits[int(pos[q, j])]
                sb = h.score_breakdown or {}
                sb["mmr"], sb["mmr_max_sim"] = float(val[q, j]), float(sim[q, j])
                h.score_breakdown, h.rank = sb, j + 1
                out.append(h)
            outs.append(out)
        return outs

    @staticmethod
    def _hit_text(h: Any) -> str:
        """str(hit) — what the reference's rerank stage hands to the cross-encoder (hybrid_retriever.py:343 passes the hit
        objects, rerankers.py:78-86 stringifies them) — without pydantic walking the whole model per hit: the chunk's
        repr (nearly all of the string: the law text) is cached per LawChunk object, the rest formatted field by field in
        the schema's order.  Identical to str(h) (tests/test_host_logic.py; the reference-generated strings of
        search_golden.json pin it end to end)."""
        if type(h) is not RetrievalHit:
            return _to_doc_text(h)
        ck = h.chunk
        ent = _CHUNK_REPR.get(id(ck))
        if ent is None or ent[0] is not ck:
            if len(_CHUNK_REPR) > 500_000:
                _CHUNK_REPR.clear()
            ent = _CHUNK_REPR[id(ck)] = (ck, "chunk=" + repr(ck))
        tail = (f" score={h.score!r} rank={h.rank!r} source={h.source!r} "
                f"semantic_score={h.semantic_score!r} graph_depth={h.graph_depth!r} relations={h.relations!r} "
                f"seed_article_id={h.seed_article_id!r} score_breakdown={h.score_breakdown!r}")
        return HitText(ent[1], tail)

    def _rerank_stage(self, questions: Sequence[str], fused_lists: List[List[RetrievalHit]], llm: Any,
                      top_k: int) -> List[List[RetrievalHit]]:
        """hybrid_retriever.py:324-356 for one or many queries: the first rerank_top_n fused hits of each query are
        scored by the reranker (cross-encoder unless an LLM judge is configured and the list is short,
        rerankers.py:301-312), the scores normalised, blended and the lists re-ranked — the scoring of ALL queries'
        candidates goes through the model in full batches (`score_pairs`), the blend of all queries is ONE
        amdr_rerank_blend launch."""
        rcfg = self.cfg.retrieval
        use_llm_rerank = bool(getattr(rcfg, "rerank_use_llm", False))
        dev = getattr(rcfg, "device", None)
        factory = RerankerFactory(llm=llm if use_llm_rerank else None, cross_model=rcfg.rerank_ce_model,
                                  llm_threshold=30, use_cache=True,
                                  device=None if dev is None else (dev if isinstance(dev, str) else f"cuda:{int(dev)}"),
                                  fp16=bool(getattr(rcfg, "rerank_fp16", False)))
        rerank_top_n = int(getattr(rcfg, "rerank_top_n", min(40, max(10, top_k * 4))))
        beta = float(getattr(rcfg, "rerank_beta", 0.35))
        # the reference hands the hit objects to rerank_candidates, whose _to_doc_text turns them into str(hit)
        # (rerankers.py:78-86) — kept.
        jobs = []  # (query index, reranker, docs)
        for qi, fused in enumerate(fused_lists):
            cand = fused[:rerank_top_n]
            if cand:
                jobs.append((qi, factory.create(top_k=len(cand)), [self._hit_text(h) for h in cand]))
        raws: Dict[int, List[float]] = {}
        by_model: Dict[int, List[int]] = {}
        for j, (_, rr, _) in enumerate(jobs):
            by_model.setdefault(id(rr), []).append(j)
        for group in by_model.values():
            rr = jobs[group[0]][1]
            if len(group) > 1 and hasattr(rr, "score_pairs"):
                pairs = [(questions[jobs[j][0]], d) for j in group for d in jobs[j][2]]
                flat = [float(x) for x in rr.score_pairs(pairs)]
                at = 0
                for j in group:
                    n = len(jobs[j][2])
                    raws[jobs[j][0]] = flat[at:at + n]
                    at += n
            else:
                for j in group:
                    qi, _, docs = jobs[j]
                    raws[qi] = [float(x) for x in rr.score_batch(questions[qi], docs)]
        todo = [qi for qi in range(len(fused_lists)) if qi in raws]
        if todo:
            blended = self._rerank_blend_many([fused_lists[qi] for qi in todo], [raws[qi] for qi in todo], beta)
            fused_lists = list(fused_lists)
            for qi, hits in zip(todo, blended):
                fused_lists[qi] = hits
        return fused_lists

    @staticmethod
    def _rerank_blend(fused: List[RetrievalHit], raw: List[float], beta: float) -> List[RetrievalHit]:
        return HybridRetriever._rerank_blend_many([fused], [raw], beta)[0]

    @staticmethod
    def _rerank_blend_many(lists: List[List[RetrievalHit]], raws: List[List[float]], beta: float) -> List[List[RetrievalHit]]:
        """hybrid_retriever.py:343-355 on the GPU for a batch of queries in one launch: normalise the cross-encoder
        scores, blend, re-rank.  `raws[q][j]` belongs to lists[q][j]."""
        nq = len(lists)
        n = max(len(f) for f in lists)
        top_n = max(len(r) for r in raws)
        ids = np.full((nq, n), -1, dtype=np.int64)
        vals = np.zeros((nq, n, _native.FUSE_NVALS), dtype=np.float64)
        mask = np.zeros((nq, n), dtype=np.int32)
        count = np.zeros(nq, dtype=np.int32)
        ce = np.zeros((nq, top_n), dtype=np.float64)
        for q, (fused, raw) in enumerate(zip(lists, raws)):
            m = len(fused)
            ids[q, :m] = np.arange(m)
            vals[q, :m, 0] = [float(h.score) for h in fused]
            count[q] = m
            ce[q, :len(raw)] = raw
        rr = _native.rerank_blend(count, ids, vals, mask, ce, float(beta))
        outs: List[List[RetrievalHit]] = []
        for q, fused in enumerate(lists):
            out: List[RetrievalHit] = []
            for r in range(len(fused)):
                h = fused[int(ids[q, r])]
                h.score = float(vals[q, r, 0])
                h.rank = r + 1
                if not math.isnan(rr[q, r, 0]):
                    h.score_breakdown = h.score_breakdown or {}
                    h.score_breakdown.update({"rerank_raw": float(rr[q, r, 0]), "rerank_norm": float(rr[q, r, 1]),
                                              "rerank_beta": beta})
                    h.source = "rerank"
                out.append(h)
            outs.append(out)
        return outs

    # ------------------------------------------------- device-resident stage
    def _stage(self) -> "_NativeStage":
        """The ONE home of the native stage's state, made on first use (retrievers built with __new__ have no
        __post_init__; setdefault: two threads' first calls agree on one object)."""
        return self.__dict__.get("_native_stage") or self.__dict__.setdefault("_native_stage", _NativeStage())

    def native_engine(self, with_colbert: bool = False):
        """The HybridEngine of the device-resident stage with / without the ColBERT channel; None until a search has
        built it (and again after the indexes were reloaded)."""
        return self._stage().engines.get(bool(with_colbert))

    def _native_channels(self, eff: int):
        """(dense store, bm25 retriever, colbert retriever | None) when every channel is this
        package's own retriever over the SAME chunk list, so that one row number means one chunk in
        all of them and the whole stage can stay in HBM; None -> the per-channel path (duck-typed
        retrievers, indexes built over different chunk lists, depth beyond the kernels' limit,
        AMDR_SEARCH_NATIVE=0)."""
        import os
        if os.environ.get("AMDR_SEARCH_NATIVE") == "0" or eff > _native.MAX_K:
            return None
        if not isinstance(self.dense, DenseRetriever) or not isinstance(self.bm25, BM25Retriever):
            return None
        if self.colbert is not None and not isinstance(self.colbert, ColBERTRetriever):
            return None
        try:
            self.dense.store.load()
            self.bm25.load()
            col = self.colbert if (self.colbert is not None and self.colbert.enabled) else None
            if col is not None:
                col._load_meta_and_collection()
        except Exception:  # noqa: BLE001 - the per-channel path raises the reference's own errors
            return None
        store = self.dense.store
        # (the BM25 retriever's Han mode: an engine's device tokeniser is a copy of the host tokeniser in that mode)
        # (appends counts in-place mutations: an in-place BM25 append or removal keeps the object and changes n_docs and
        # the term ids: engines and reserves are made again)
        # (rows_epoch counts the dense index's in-place removals and replacements, FlatIPIndex.remove_ids / replace_rows: the
        # object stays, its rows move or change)
        key = (id(store.index), getattr(store.index, "rows_epoch", 0), id(self.bm25.bm25), getattr(self.bm25, "appends", 0),
               id(col._searcher) if col is not None else None, id(col._pid2chunk) if col is not None else None,
               self.bm25.han_key())
        st = self._stage()
        if st.key != key:
            a, b = store.chunks, self.bm25.chunks
            same = len(a) == len(b) and all(x.id == y.id for x, y in zip(a, b))
            if same and col is not None:
                same = len(col._pid2chunk) == len(a) and all(
                    (col._pid2chunk.get(i) is not None and col._pid2chunk[i].id == c.id) for i, c in enumerate(a))
            st.key, st.ok, st.engines = key, bool(same) and getattr(store.index, "native", None) is not None, {}
        return (store, self.bm25, col) if st.ok else None

    @staticmethod
    def _make_engine(store, bm, col, dev: int):
        """The device pipeline over the three retrievers' own indexes.  In a row-sharded deployment
        (cfg.retrieval.shard = "rows") every index holds this rank's row block and the engine exchanges the
        per-shard top-k once per batch (engine.HybridEngine, sharding.exchange_topk); the three blocks must be the
        same rows, which contiguous blocks of one chunk list are."""
        from .engine import HybridEngine
        shard = getattr(store.index, "spec", None)
        offset = None
        if shard is not None:
            offset = int(store.index.row_offset)
            if getattr(bm, "shard", None) is None or (col is not None and (col.shard is None or col.row_offset != offset)):
                raise RuntimeError("row-sharded search: the dense, BM25 and ColBERT channels must all be sharded "
                                   "(load them under the same cfg.retrieval.shard and process group)")
        return HybridEngine(store.index.native, bm.gpu_index(), col._searcher if col is not None else None,
                            device=dev, shard_offset=offset, shard_group=shard.group if shard is not None else None)

    def _engine(self, store, bm, col):
        """The stage's engine with / without ColBERT, built on first use (caller holds the stage lock)."""
        engines = self._stage().engines
        eng = engines.get(col is not None)
        if eng is None:
            eng = engines[col is not None] = self._make_engine(store, bm, col, int(getattr(self.cfg.retrieval, "device", 0)))
        return eng

    def _prepare(self, questions: Sequence[str], native, q_emb=None, device_tok: bool = False) -> "_Prepared":
        """Step 1, outside the lock: embed / tokenise / encode the batch on the host side.
        device_tok (cfg.retrieval.query_tokenizer = "device"): a batch the device rule decides
        (BM25Retriever.device_text_batch) goes up as UTF-8 text and is tokenised on the GPU (_run); any other batch
        takes the host tokeniser."""
        import torch
        store, bm, col = native
        tdev = torch.device("cuda", int(getattr(self.cfg.retrieval, "device", 0)))
        if q_emb is None:
            q_emb = store.embed_device(list(questions), is_query=True)  # encoder output stays in HBM
        else:  # the caller's own encoder output (numpy or a device tensor), one row per question
            q_emb = (torch.from_numpy(np.ascontiguousarray(q_emb, dtype=np.float32)) if isinstance(q_emb, np.ndarray)
                     else q_emb).to(tdev, dtype=torch.float32, non_blocking=True).contiguous()
            if q_emb.shape != (len(questions), store.index.d):
                raise ValueError(f"q_emb must be [{len(questions)}, {store.index.d}], got {tuple(q_emb.shape)}")
        t1 = time.time()
        csr, txt = None, bm.device_text_batch(questions) if device_tok else None
        if txt is None:
            qt, qp, exact = bm.term_ids_batch(questions)  # native batched tokeniser + vocabulary lookup
            if qt.size == 0:
                qt = np.zeros(1, dtype=np.int32)  # pack_queries' convention for "no term at all"
            csr = (qt, qp)
        else:
            exact = txt[4]  # False where a stand-in cuts a Han query (BM25Retriever.device_text_batch)
        t2 = time.time()
        q_tok = None
        if col is not None:
            try:
                # the ColBERT query side of the whole batch in ONE encoder call: a device tensor when the encoder can hand
                # one over (TransformersColBERT: one BERT forward, nothing comes back to the host), else one numpy batch
                stripped = [(q or "").strip() for q in questions]
                enc = col._encoder
                if hasattr(enc, "encode_queries_tensor"):
                    q_tok = enc.encode_queries_tensor(stripped)
                elif hasattr(enc, "encode_queries"):
                    q_tok = np.ascontiguousarray(enc.encode_queries(stripped), dtype=np.float32)
                else:
                    q_tok = np.stack([np.asarray(enc.encode_query(q), dtype=np.float32) for q in stripped])
            except Exception:  # noqa: BLE001 - the reference swallows ColBERT channel errors (:244-245)
                if getattr(store.index, "spec", None) is not None:
                    # row-sharded: dropping the channel is a rank-LOCAL decision inside an SPMD exchange — the other ranks
                    # would all-gather three packed channels against this rank's two (hang, or garbage).  Fail loudly.
                    raise
                col, q_tok = None, None
        return _Prepared((store, bm, col), q_emb, csr, txt, np.asarray(exact, dtype=bool), q_tok, (t1, t2, time.time()))

    def _run(self, prep: "_Prepared", params: "_native.FuseParams", eff: int, fetch, after=None, scope_table=None, mmr=None,
             term_table=None):
        """Step 2, under the stage lock (one batch at a time through the handles' "_device" workspace,
        include/amdretrieval.h): engine, upload, eng.search_batch on torch's current stream, the ColBERT fallback,
        `after(engine, result)` (the device graph stage), then `fetch(engine, result)` — the ONE synchronise and
        device-to-host copy of the form the caller decodes.  Returns (what fetch returned, what after returned).
        scope_table (ScopeResolver.table of the batch): the scoped step — the three channels share one chunk list here
        (_native_channels), so one table serves them all.  mmr = (k_sel, lam, pool): the result is diversified on the device
        (HybridEngine.diversify) behind `after`, whose seeds are the fused list as ranked, and in front of `fetch`.
        term_table (retrieval/terms.py pack of the batch) instead of scope_table: the table is resolved on the device from
        the term constraints (HybridEngine.term_scopes) in the same stream; its status words ride a pinned copy enqueued
        behind it and are read after fetch's synchronise — a non-zero one raises RuntimeError naming the constraint."""
        import torch
        (store, bm, col), tdev = prep.native, prep.q_emb.device
        with self._stage().lock:
            eng = self._engine(store, bm, col)
            if prep.text is None:
                # BM25 query CSR in ONE host-to-device copy through pinned staging: q_ptr (i64) then q_terms (i32)
                q_ptr_d, q_terms_d = eng.upload_csr(np.ascontiguousarray(prep.csr[1], dtype=np.int64),
                                                    np.ascontiguousarray(prep.csr[0], dtype=np.int32))
            else:
                # the query texts in ONE host-to-device copy (packed into pinned staging), the CSR made on the device
                if eng.tokenizer is None:  # (a reloaded BM25 index changes the compatibility key: new engines)
                    eng.tokenizer = bm.device_tokenizer()
                blob_d, offs_d = eng.upload_text(*prep.text[:3])
                q_terms_d, q_ptr_d, _ = eng.tokenize_device(blob_d, offs_d)
            q_tok = prep.q_tok
            if q_tok is not None:
                q_tok = (q_tok.to(tdev, dtype=torch.float32).contiguous() if torch.is_tensor(q_tok)
                         else torch.from_numpy(q_tok).to(tdev, non_blocking=True))

            status = []

            def scoped(e, with_col):
                if term_table is not None:
                    tb, st = e.term_scopes(term_table)
                    pin = e._pinned("tsst", 4 * max(int(st.numel()), 1))[:4 * int(st.numel())]
                    pin.copy_(st.view(torch.uint8), non_blocking=True)
                    status[:] = [pin]
                elif scope_table is None:
                    return {}
                else:
                    tb = e.upload_scopes(*scope_table[:3])
                return {"scopes": (tb, tb, tb if with_col else None)}
            try:
                res = eng.search_batch(params, eff, q_emb=prep.q_emb, q_terms=q_terms_d, q_ptr=q_ptr_d, q_tok=q_tok,
                                       **scoped(eng, q_tok is not None))
            except _native.NativeError:
                if col is None or eng.shard_offset is not None:
                    raise  # (row-sharded: a rank must not leave the common exchange on its own, see _prepare)
                # a failing ColBERT stage (e.g. out of memory) empties that channel, it does not fail the query
                # (hybrid_retriever.py:244-245, colbert_retriever.py:171-181); a dense / BM25 failure raises again here
                eng = self._engine(store, bm, None)
                res = eng.search_batch(params, eff, q_emb=prep.q_emb, q_terms=q_terms_d, q_ptr=q_ptr_d, **scoped(eng, False))
            extra = after(eng, res) if after is not None else None
            if mmr is not None:
                res = eng.diversify(res, *mmr)
            host = fetch(eng, res)
            if status:  # (fetch has synchronised the stream the copy was enqueued on)
                bad = np.flatnonzero(status[0].numpy().view(np.int32))
                if bad.size and int(bad[0]) >= int(term_table.n_cons):  # the phrases' words stand behind the constraints'
                    p = int(bad[0]) - int(term_table.n_cons)
                    raise RuntimeError(f"{term_table.list_item(p)!r} of the batch overflowed its bound (status "
                                       f"{int(status[0].numpy().view(np.int32)[bad[0]])}: 1 = candidates beyond cand_max, "
                                       f"2 = documents beyond rows_cap); the host model and the resident BM25 index disagree")
                if bad.size:
                    c = int(bad[0])
                    raise RuntimeError(f"term constraint {c} of the batch overflowed its bound (status "
                                       f"{int(status[0].numpy().view(np.int32)[c])}: 1 = candidates beyond cand_max, 2 = rows "
                                       f"beyond rows_cap); the host model and the resident BM25 index disagree")
            return host, extra

    # Step 3, the decoders: host arrays of ONE fetch -> the caller's form.
    def _decode_hits(self, host, exact, kn, chunks) -> List[List[RetrievalHit]]:
        ids, vals, mask, cnt = host
        out = []
        for qi in range(len(cnt)):
            # only the hits that survive min_final_score are ever used (hybrid_retriever.py:309-310)
            hits = self._hits_from_native(ids[qi], vals[qi], mask[qi], int(cnt[qi]), kn, chunks)
            if not exact[qi]:
                for h in hits:
                    h.score_breakdown["zh_exact"] = False
            out.append(hits)
        return out

    @staticmethod
    def _decode_columns(host, exact, top_k: int, chunks) -> Dict[str, Any]:
        """The full columnar dict from BatchResult.to_host(): the first top_k columns and every fused value."""
        ids, vals, mask, cnt = host
        w = min(top_k, ids.shape[1])
        keep = np.arange(w)[None, :] < np.minimum(cnt, w)[:, None]
        return {"rows": np.where(keep, ids[:, :w], -1), "scores": np.where(keep, vals[:, :w, _native.FV["score"]], 0.0),
                "count": np.minimum(cnt, w).astype(np.int32), "channel_mask": np.where(keep, mask[:, :w], 0),
                "values": vals[:, :w], "value_names": dict(_native.FV), "zh_exact": exact, "chunks": chunks}

    @staticmethod
    def _decode_lean(host, exact, chunks) -> Dict[str, Any]:
        """The lean columnar dict from HybridEngine.compact_to_host(result, top_k): rows / scores / count / channel_mask
        only, cut to top_k on the device — 20 bytes per hit over PCIe instead of the full fused record (9 doubles for
        every candidate of every channel: 1.6 KB per query)."""
        rows, scores, cmask, cnt = host
        return {"rows": rows, "scores": scores, "count": cnt, "channel_mask": cmask, "zh_exact": exact, "chunks": chunks}

    # ----------------------------------------------------------- batch form
    @staticmethod
    def _no_terms(terms, who: str) -> bool:
        """Whether `terms` (None, or one Terms | None per question) restricts no question; TypeError for anything else."""
        if terms is None:
            return True
        for i, t in enumerate(terms):
            if t is not None and not isinstance(t, Terms):
                raise TypeError(f"{who}: terms[{i}] is not a Terms")
        return all(t is None or t.unrestricted for t in terms)

    @staticmethod
    def _check_terms(terms, native, who: str) -> None:
        """The refusal of term constraints on a row-sharded index, before anything is launched (the engine refuses too)."""
        if terms is None:
            return
        store, bm, col = native
        if (getattr(store.index, "spec", None) is not None or getattr(bm, "shard", None) is not None
                or (col is not None and getattr(col, "shard", None) is not None)):
            raise ValueError(f"{who}(terms=): term constraints do not run on a row-sharded index (base rows and the "
                             f"table are global)")

    @staticmethod
    def _partition(questions: Sequence[str], scopes, decisions, chunks, colbert: bool, who: str, terms=None):
        """(parts, empty) of a batch; needs neither device nor torch.  A part is (indices, scoped, ColBERT on): questions
        that share one engine run.  The order is fixed — plain-blank, plain, scoped-blank, scoped — and a part without an
        index is left out.  A blank question switches the ColBERT channel off for itself (colbert_retriever.py:147-149), so
        with the channel on (`colbert`) the blank ones run apart, without it; with the channel off nothing is split.
        `empty`: the questions whose scope names no row of `chunks` (no launch is made for them).  A graph-mode decision
        together with a scope raises: the graph channel follows cross-references out of any scope by design.
        `terms` (one Terms or None per question): a question with a Terms joins the scoped part — whether it matches
        anything is known only on the device — and refuses a graph-mode decision as a scope does."""
        n = len(questions)
        if terms is not None and len(terms) != n:
            raise ValueError(f"{who}: terms must have one entry per question")
        if scopes is not None and len(scopes) != n:
            raise ValueError(f"{who}: scopes must have one entry per question")
        if decisions is not None and len(decisions) != n:
            raise ValueError(f"{who}: decisions must have one entry per question")
        plain, scoped, empty = range(n), [], []
        for i, s in enumerate(scopes if scopes is not None else ()):
            if s is None:
                continue
            if not isinstance(s, Scope):
                raise TypeError(f"{who}: scopes[{i}] is not a Scope")
            if decisions is not None and _is_graph_mode(getattr(decisions[i], "mode", None)):
                raise ValueError(f"{who}: question {i} has a graph-mode decision and a scope; the graph channel follows "
                                 f"cross-references out of any scope")
            (scoped if resolver_for(chunks).rows(s).size else empty).append(i)
        for i, t in enumerate(terms if terms is not None else ()):
            if t is None:
                continue
            if not isinstance(t, Terms):
                raise TypeError(f"{who}: terms[{i}] is not a Terms")
            if t.unrestricted:
                continue
            if decisions is not None and _is_graph_mode(getattr(decisions[i], "mode", None)):
                raise ValueError(f"{who}: question {i} has a graph-mode decision and term constraints; the graph channel "
                                 f"follows cross-references to articles that do not hold the terms")
            if i not in scoped and i not in empty:
                scoped.append(i)
        scoped.sort()
        if scoped or empty:
            out = set(scoped).union(empty)
            plain = [i for i in plain if i not in out]
        parts = []
        for idxs, sc in ((plain, False), (scoped, True)):
            blank = [i for i in idxs if not (questions[i] or "").strip()] if colbert else []
            if blank:
                parts.append((blank, sc, False))
                drop = set(blank)
                idxs = [i for i in idxs if i not in drop]
            parts.append((idxs, sc, colbert))
        return [p for p in parts if len(p[0])], empty

    def _split_scopes(self, n: int, scopes, decisions, chunks, who: str):
        """(plain, scoped, empty) of _partition with the ColBERT channel left aside."""
        parts, empty = self._partition([None] * n, scopes, decisions, chunks, False, who)
        by = {sc: list(idxs) for idxs, sc, _ in parts}
        return by.get(False, []), by.get(True, []), empty

    def _run_part(self, part, questions, scopes, q_emb, native, device_tok: bool, params, eff: int, fetch, decode, graph=None,
                  mmr=None, terms=None):
        """One part of a batch in one engine run: _prepare -> the scope table of a scoped part -> _run -> `decode(host
        arrays, exact)`; `graph` (what _graph_device_stage returned) rides the part it names.  Returns (what decode
        returned, the _Prepared's time stamps, what the graph stage returned).  A part that is the whole batch takes the
        caller's questions and q_emb as they are."""
        idxs, scoped, with_col = part
        store, bm, col = native
        after = graph[2] if graph is not None and part is graph[0] else None
        if len(idxs) < len(questions):
            questions = [questions[i] for i in idxs]
            q_emb = None if q_emb is None else q_emb[idxs]
        prep = self._prepare(questions, (store, bm, col if with_col else None), q_emb, device_tok)
        table = term_table = None
        if scoped and terms is not None and any(terms[i] is not None and not terms[i].unrestricted for i in idxs):
            # one table for the part: a question with a Scope alone is the constraint without a group over that base
            model = bm.bm25  # (looked up per call: an in-place update renumbers the vocabulary)
            term_table = _pack_terms([(scopes[i] if scopes is not None else None, terms[i] or Terms()) for i in idxs],
                                     model.vocab(), model._doc_frequencies(), int(model.corpus_size),
                                     resolver_for(store.chunks).rows,
                                     model.sorted_vocab() if any(terms[i] is not None and (
                                         terms[i].has_union or terms[i].has_class_span or terms[i].has_within)
                                                              for i in idxs) else None,
                                     self._expansions(bm, [terms[i] for i in idxs]))
            if term_table.n_phr or term_table.n_near or term_table.n_cspan:
                bm.ensure_token_stream()  # (made lazily: on the first phrase or Near, and again after a live update)
            if term_table.n_unit:
                bm.ensure_breaks()  # (the break flags beside it: only a batch with a Within pays for them)
        elif scoped:
            table = resolver_for(store.chunks).table([scopes[i] for i in idxs])
        host, extra = self._run(prep, params, eff, fetch, after, table, mmr, term_table)
        return decode(host, prep.exact), prep.stamps, extra

    def _hit_lists(self, questions: Sequence[str], parts, eff: int, native, min_final: float, q_emb=None,
                   device_tok: bool = False, scopes=None, graph=None, terms=None):
        """The parts of a batch as hit lists: ([fused hits with score >= min_final per question; [] for a question no part
        holds: its scope matches nothing], (t_after_dense_prep, t_after_bm25_prep, t_after_colbert_prep) of the last part,
        what the graph stage `graph` (_graph_device_stage) returned)."""
        kn = self._knobs()
        params = self._params(kn, min_final)
        chunks = native[0].chunks
        outs, stamps, gout = [[] for _ in questions], (time.time(),) * 3, None
        for part in parts:
            lists, stamps, g = self._run_part(part, questions, scopes, q_emb, native, device_tok, params, eff, _fetch_full,
                                              lambda host, exact: self._decode_hits(host, exact, kn, chunks), graph,
                                              terms=terms)
            gout = gout if g is None else g
            for i, hits in zip(part[0], lists):
                outs[i] = hits
        return outs, stamps, gout

    def _graph_selection(self, decisions, top_k: int):
        """(sel, seed_n): the questions whose decision asks for the graph channel (none unless cfg.retrieval.enable_graph)
        and how many fused hits seed the walk."""
        rcfg = self.cfg.retrieval
        on = decisions is not None and getattr(rcfg, "enable_graph", False)
        sel = [i for i, dec in enumerate(decisions) if _is_graph_mode(getattr(dec, "mode", None))] if on else []
        return sel, int(getattr(rcfg, "graph_seed_k", max(10, top_k * 3)))

    def search_batch(self, questions: Sequence[str], top_k: int = 10, llm: Any = None,
                     decisions: Optional[Sequence[Any]] = None, q_emb=None, *,
                     scopes: Optional[Sequence[Optional[Scope]]] = None, diversity: Any = None,
                     terms: Optional[Sequence[Optional[Terms]]] = None,
                     highlight: Optional[Highlight] = None) -> List[List[RetrievalHit]]:
        """Throughput form: `search_batch(qs)[i]` == `search(qs[i])` for every stage the configuration enables
        (hybrid_retriever.py:282-384) — one kernel pipeline for the whole batch (dense + BM25 (+ ColBERT) -> fuse
        -> filter), the graph stage per query whose `decisions[i]` asks for it, the rerank stage with the
        cross-encoder fed in full batches over all queries' candidates and ONE blend launch, dedup, cut.
        `scopes` (one Scope or None per question, retrieval/scope.py): a scoped question's channels rank only its part of
        the corpus and its fusion normalises over those lists; the questions with None run as one part through the
        unscoped step, the scoped ones as another; a scope that matches nothing yields [].  A graph-mode decision with a
        scope raises ValueError.
        `terms` (one Terms or None per question, retrieval/terms.py): a question with a Terms joins the scoped part; its
        constraint — inside its Scope, if it has one — is resolved on the GPU from the resident BM25 postings into the
        part's scope table (HybridEngine.term_scopes), so every channel ranks only the qualifying chunks; a constraint that
        matches nothing yields [].  ValueError, before any launch, with a graph-mode decision, on a row-sharded index, or
        when the channels do not share one chunk list.
        `diversity`: as search — MMR selection as the last stage, ONE batched call for all questions.
        `highlight`: as search — behind every ranking stage, ONE native call for the hits of all questions."""
        if highlight is not None and not isinstance(highlight, Highlight):
            raise TypeError(f"search_batch(highlight=) is a Highlight or None, got {type(highlight).__name__}")
        rcfg = self.cfg.retrieval
        top_k = max(1, int(top_k))
        questions = list(questions)
        if self._no_terms(terms, "search_batch"):
            terms = None
        mmr = self._diversity(diversity, top_k, "search_batch")
        eff = self._eff_depth(top_k, "search_batch")
        native = self._native_channels(eff)
        if native is None:
            if terms is not None:
                raise ValueError("search_batch(terms=): term constraints need this package's own dense / BM25 (/ ColBERT) "
                                 "retrievers built over one chunk list (a BM25 document id must be a dense row)")
            raise RuntimeError("search_batch requires this package's own dense / BM25 (/ ColBERT) retrievers built "
                               "over the same chunk list")
        self._check_terms(terms, native, "search_batch")
        parts, _ = self._partition(questions, scopes, decisions, native[0].chunks, native[2] is not None, "search_batch",
                                   terms)
        sel, seed_n = self._graph_selection(decisions, top_k)
        # The graph walks at the per-channel depth `eff`.  With the device channel off or no graph loaded the stage
        # falls back to the host search_graph per query (which, without a graph, still cuts the list to the seeds).
        graph = None
        if sel and self.graph is not None and graph_channel_mode(self.cfg) == "device":
            graph = self._graph_device_stage(parts, questions, sel, eff, seed_n, native)
        outs, _, gout = self._hit_lists(questions, parts, eff, native, float(getattr(rcfg, "min_final_score", 0.0)), q_emb,
                                        query_tokenizer_mode(self.cfg) == "device", scopes, graph, terms)
        for j, i in enumerate(sel):
            seeds = outs[i][:seed_n]
            if graph is not None:
                # one device call served every graph-mode query; the same relabelling as search_graph
                hits = self.graph.hits_from_device(gout, j, graph[3])
                for h in hits:
                    h.source = "retriever"
                    h.score_breakdown["channel"] = ["graph"]
            else:
                hits = self.search_graph(questions[i], eff, decision=decisions[i], seeds=seeds)
            outs[i] = seeds + hits
        # rerank, dedup and cut run once, over the whole batch (a question whose scope matches nothing has no candidate)
        if getattr(rcfg, "enable_rerank", False):
            outs = self._rerank_stage(questions, outs, llm, top_k)
        outs = [_dedup_keep_best(hits) for hits in outs]
        if mmr is not None:
            outs = self._mmr_stage(outs, top_k, *mmr)
        outs = [hits[:top_k] for hits in outs]
        if highlight is not None:
            self._highlight_stage(questions, outs, terms, highlight)
        return outs

    def _graph_device_stage(self, parts, questions: Sequence[str], sel: Sequence[int], k: int, seed_n: int, native,
                            lang: Optional[str] = None):
        """The graph channel of a batch on the device (graph_channel = "device"): the graph-mode questions `sel` embedded
        once (non-query form, as GraphRetriever's store._embed(question)), then ONE amdr_graph_search_device call over the
        fused lists of their part, seeds = the first graph_seed_k fused hits.  _partition has refused graph mode with a
        scope, so `sel` lies in the plain questions; they must share one engine run.  Returns (that part, sel as indices
        inside it, after, params): `after(engine, BatchResult)` is the stage for _run (its outputs as host arrays, one row
        per question of sel), params what hits_from_device takes.  Row-sharded indexes and parameters outside the kernel's
        limits raise ValueError (no silent host path)."""
        import torch
        store = native[0]
        plain = [p for p in parts if not p[1]]
        if len(plain) != 1 or plain[0][2] != (native[2] is not None):
            raise ValueError("graph_channel='device': empty questions are not supported with the ColBERT channel on")
        if getattr(store.index, "spec", None) is not None:
            raise ValueError("graph_channel='device' does not run on a row-sharded index (cfg.retrieval.shard); "
                             "use graph_channel='host'")
        g, _t = self.graph.device_graph()
        params, lang_id = self.graph.device_params(k, lang)
        if k > _native.MAX_K:
            raise ValueError(f"graph_channel='device': depth {k} exceeds {_native.MAX_K}")
        emb = store.embed_device([questions[i] for i in sel], is_query=False)
        at = {i: j for j, i in enumerate(plain[0][0])} if len(plain[0][0]) < len(questions) else None
        sel = list(sel) if at is None else [at[i] for i in sel]

        def after(eng, res):
            eng.set_graph(g, params, lang_id)
            nq = int(res.ids.shape[0])
            q_full = eng._buf("gq", (nq, int(emb.shape[1])), torch.float32)
            qsel = torch.tensor(sel, dtype=torch.int32).to(eng.tdev, non_blocking=True)
            q_full.index_copy_(0, qsel.long(), emb.to(eng.tdev, dtype=torch.float32))
            eng.graph.reserve(len(sel), k, eng.graph_limit)
            outs = eng.graph_topk(res.ids, res.count, q_full, k, seed_n, qsel=qsel)
            return {n: v.cpu().numpy() for n, v in outs.items()}
        return plain[0], sel, after, params

    def _graph_columns(self, cols: Dict[str, Any], g, sel: Sequence[int], top_k: int) -> None:
        """The graph_* columns of a part's columnar dict: what the device stage returned (`g`, one row per question of
        `sel`; None: no graph-mode question) at the rows `sel`, the schema's fill everywhere else."""
        n = len(cols["count"])
        for name, dt, fill, hit in COLUMNS:
            if name.startswith("graph_"):
                cols[name] = _column(n, top_k, dt, fill, hit)
                if g is not None:
                    cols[name][sel] = g["final" if name == "graph_scores" else name[len("graph_"):]]
        cols["graph_relation_names"] = list(self.graph.device_graph()[1].rel_names)

    @staticmethod
    def _scatter_columns(n: int, top_k: int, values: bool, chunks, parts) -> Dict[str, Any]:
        """The columnar dict of n questions from the decoded parts [(indices, columnar dict)].  A part's rows land at its
        indices; a question no part holds (its scope matches nothing) and a column a part does not carry (graph_* beside
        a scoped part) keep the schema's fill.  What is no column (value_names, chunks, graph_relation_names) passes
        through.  ONE part holding every question is returned as it is."""
        if len(parts) == 1 and len(parts[0][0]) == n:
            return parts[0][1]
        out: Dict[str, Any] = {"chunks": chunks}
        if values:
            out["value_names"] = dict(_native.FV)
        for name, dt, fill, hit in COLUMNS + MMR_COLUMNS:
            if any(name in cols for _, cols in parts) or not (name.startswith(("graph_", "mmr")) or
                                                              (name == "values" and not values)):
                out[name] = _column(n, top_k, dt, fill, hit)
                for idxs, cols in parts:
                    if name in cols:
                        out[name][idxs] = cols[name]
        for _, cols in parts:
            for key, val in cols.items():
                out.setdefault(key, val)
        return out

    def search_batch_arrays(self, questions: Sequence[str], top_k: int = 10, q_emb=None, values: bool = True,
                            decisions: Optional[Sequence[Any]] = None, *,
                            scopes: Optional[Sequence[Optional[Scope]]] = None, diversity: Any = None,
                            terms: Optional[Sequence[Optional[Terms]]] = None) -> Dict[str, Any]:
        """`search_batch` without building RetrievalHit objects (pydantic construction, not the GPU, bounds
        `search_batch` at a few thousand queries/s): columnar results for bulk callers (evaluation sweeps,
        offline scoring).  rows[q, j] indexes `self.dense.store.chunks`; entries j >= count[q] are -1 / 0.
        `q_emb` ([n, d] numpy array or device tensor): query embeddings the caller's encoder already produced
        (a deployment batches its BERT forward itself); default: this store's encoder.
        `values=False`: rows / scores / count / channel_mask only (_decode_lean) instead of the full record.
        The rows of one index are distinct chunks, so the dedup step of search() has nothing to merge.
        `decisions` (one per question): the graph channel runs on the device for the GRAPH_AUGMENTED ones (when
        cfg.retrieval.enable_graph and a graph is loaded) and the result gains graph_rows / graph_scores (final) /
        graph_semantic / graph_depth / graph_relation (index into graph_relation_names) / graph_edge_conf [n, top_k] and
        graph_count [n] (0 for the other queries).
        `scopes`: as search_batch — one Scope or None per question; a scope that matches nothing gives count 0.
        `terms`: as search_batch — one Terms or None per question; a constraint that matches nothing gives count 0.
        `diversity`: as search — the selection runs on the device inside the stage (HybridEngine.diversify) over the
        fused list of every part, scoped ones included; the columns hold the selected hits in selection order and, with
        values=True, `mmr` and `mmr_max_sim` [n, top_k] beside them (MMR_COLUMNS).
        COLUMNS holds every column's dtype and the fill of a question or hit without a result."""
        rcfg = self.cfg.retrieval
        top_k = max(1, int(top_k))
        mmr = self._diversity(diversity, top_k, "search_batch_arrays")
        mmr = None if mmr is None else (top_k, mmr[0].lam, mmr[1])
        eff = self._eff_depth(top_k, "search_batch_arrays")
        native = self._native_channels(eff)
        if self._no_terms(terms, "search_batch_arrays"):
            terms = None
        if native is None:
            if terms is not None:
                raise ValueError("search_batch_arrays(terms=): term constraints need this package's own retrievers built "
                                 "over one chunk list (a BM25 document id must be a dense row)")
            raise RuntimeError("search_batch_arrays requires this package's own retrievers built over the same chunk list")
        self._check_terms(terms, native, "search_batch_arrays")
        questions, chunks = list(questions), native[0].chunks
        parts, _ = self._partition(questions, scopes, decisions, chunks, native[2] is not None, "search_batch_arrays",
                                   terms)
        if native[2] is not None and not all(with_col for _, _, with_col in parts):
            raise ValueError("search_batch_arrays: empty questions are not supported in the columnar form")
        sel, seed_n = self._graph_selection(decisions, top_k)
        # The graph walks at depth `top_k`, always on the device; with no graph loaded `decisions` are ignored.
        graph_on = decisions is not None and getattr(rcfg, "enable_graph", False) and self.graph is not None
        graph = self._graph_device_stage(parts, questions, sel, top_k, seed_n, native) if graph_on and sel else None
        params = self._params(self._knobs(), float(getattr(rcfg, "min_final_score", 0.0)))
        if values and mmr is not None:
            def fetch(eng, res):
                return res.to_host(), res.mmr.cpu().numpy(), res.mmr_max_sim.cpu().numpy()

            def decode(host, exact):
                cols = self._decode_columns(host[0], exact, top_k, chunks)
                cols["mmr"], cols["mmr_max_sim"] = host[1], host[2]
                return cols
        elif values:
            fetch, decode = _fetch_full, lambda host, exact: self._decode_columns(host, exact, top_k, chunks)
        else:
            fetch, decode = (lambda eng, res: eng.compact_to_host(res, top_k),
                             lambda host, exact: self._decode_lean(host, exact, chunks))
        done = []
        for part in parts:
            cols, _, g = self._run_part(part, questions, scopes, q_emb, native, query_tokenizer_mode(self.cfg) == "device",
                                        params, eff, fetch, decode, graph, mmr, terms)
            if graph_on and not part[1]:
                self._graph_columns(cols, g, graph[1] if graph is not None else [], top_k)
            done.append((part[0], cols))
        return self._scatter_columns(len(questions), top_k, values, chunks, done)

"""Batched, device-resident hybrid pipeline (the throughput path).

The reference answers one query per `HybridRetriever.search` call
(hybrid_retriever.py:282-384).  This engine runs the same stages — dense top-k,
BM25 top-k, optional MaxSim top-k, `_fuse`, the min_final_score filter and the
optional rerank blend — for a whole batch of queries without leaving HBM:
every stage is a libamdretrieval kernel launched on the caller's stream, and
the buffers between stages are plain device allocations (torch tensors are
used only as the allocator / stream provider).  `HybridRetriever.search_batch`
and bench.py sit on top of it; the single-query API uses the same kernels.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import _native

NV = _native.FUSE_NVALS


def packed_layout(nq: int, w: int, nvals: int = NV):
    """Byte offsets (o1, o2, o3, total) of a packed fused record: ids i64 [nq, w] | vals f64 [nq, w, nvals] | mask i32
    [nq, w] | count i32 [nq].  nvals = FUSE_NVALS: the full record (fuse); nvals = 1: the lean one of one score per hit
    (compact_to_host).  The ONE place the layout is computed."""
    o1 = nq * w * 8
    o2 = o1 + nq * w * nvals * 8
    o3 = o2 + nq * w * 4
    return o1, o2, o3, o3 + nq * 4


def packed_views(h: np.ndarray, nq: int, w: int, nvals: int = NV):
    """(ids, vals, mask, count) as numpy views of a packed record on the host (u8 array of at least `total` bytes);
    the lean record's vals are [nq, w]."""
    o1, o2, o3, tot = packed_layout(nq, w, nvals)
    return (h[:o1].view("int64").reshape(nq, w), h[o1:o2].view("float64").reshape((nq, w, nvals) if nvals > 1 else (nq, w)),
            h[o2:o3].view("int32").reshape(nq, w), h[o3:tot].view("int32"))


# The forms of one hybrid step (step_form):
ONE_LAUNCH = "one_launch"            # both channels and the fusion in one launch (_hybrid_small)
BM25_THEN_FUSED = "bm25_then_fused"  # BM25, the dense channel and the fusion as one native call (amdr_hybrid_batch_device)
CHANNELS = "channels"                # the channels one after the other on the caller's stream, then the fusion
CHANNELS_SIDE = "channels_side"      # dense / BM25 on the side stream beside MaxSim, then the fusion
SCOPED = "scoped"                    # every channel ranks each query's own rows (search_batch(scopes=)), then the fusion
# The one-launch form is asked for up to this many queries and fused candidates per query (the serving call).
# amdr_hybrid_small_device decides again natively (corpus size, AMDR_HYBRID_SMALL) and falls back by itself to the
# launches of BM25_THEN_FUSED, so this test only has to be no narrower than the native one.
SMALL_NQ, SMALL_CANDS = 4, 32


def step_form(has_dense: bool, has_bm25: bool, has_colbert: bool, sharded: bool, nq: int, k: int, overlap: bool):
    """(form, exchange) of a step: which channels have an index AND an operand, whether the indexes are row shards,
    the batch, the depth and whether the side stream is allowed (AMDR_ENGINE_OVERLAP).  exchange: the per-shard lists
    are all-gathered and merged before the fusion.  Pure: search_batch switches on it."""
    if has_dense and has_bm25 and not has_colbert and not sharded:
        # dense + BM25 on one GPU, the serving hybrid without ColBERT
        return (ONE_LAUNCH if nq <= SMALL_NQ and 2 * k <= SMALL_CANDS else BM25_THEN_FUSED), False
    # The dense and BM25 channels of a batch are a few short launches that do not fill the chip; MaxSim's first pass is
    # ~0.8 ms on the matrix pipe.  They depend on nothing of each other until the fusion.
    side = has_colbert and overlap and (has_dense or has_bm25)
    return (CHANNELS_SIDE if side else CHANNELS), bool(sharded)


def _check_emb(q_emb: torch.Tensor) -> None:
    assert q_emb.is_cuda and q_emb.dtype == torch.float32 and q_emb.is_contiguous(), "q_emb: contiguous f32 on the device"


def _check_tok(q_tok: torch.Tensor) -> None:
    assert q_tok.is_cuda and q_tok.dtype == torch.float32 and q_tok.is_contiguous(), "q_tok: contiguous f32 on the device"


def _check_csr(q_terms: torch.Tensor, q_ptr: torch.Tensor) -> None:
    assert q_terms.dtype == torch.int32 and q_ptr.dtype == torch.int64 and q_terms.is_cuda and q_ptr.is_cuda, "BM25 CSR"


@dataclass
class BatchResult:
    ids: torch.Tensor     # i64 [nq, max_out]  fused rank order, -1 padded
    vals: torch.Tensor    # f64 [nq, max_out, 9]  (_native.FV layout)
    mask: torch.Tensor    # i32 [nq, max_out]  channel membership bits
    count: torch.Tensor   # i32 [nq]  hits surviving min_final_score
    dense_ids: Optional[torch.Tensor] = None
    dense_scores: Optional[torch.Tensor] = None
    bm25_ids: Optional[torch.Tensor] = None
    bm25_scores: Optional[torch.Tensor] = None
    colbert_ids: Optional[torch.Tensor] = None
    colbert_scores: Optional[torch.Tensor] = None
    rerank: Optional[torch.Tensor] = None  # f64 [nq, max_out, 2] (raw, norm) after rerank_blend
    packed: Optional[torch.Tensor] = None  # u8: ids | vals | mask | count in ONE allocation (one D2H for the host API)
    needs_segmenter: Optional[torch.Tensor] = None  # i32 [nq] of a text-in step (q_text): 1 = Han query, no BM25 terms
    graph: Optional[dict] = None  # graph_topk outputs of a captured step that ends with the graph stage
    # after diversify(): per selected hit its position in the fused list it was picked from, the winning MMR value and
    # its largest cosine to the hits picked before it (i32 / f64 / f64 [nq, k_sel])
    mmr_pos: Optional[torch.Tensor] = None
    mmr: Optional[torch.Tensor] = None
    mmr_max_sim: Optional[torch.Tensor] = None

    def to_host(self):
        """(ids, vals, mask, count) as numpy arrays through ONE device-to-host copy (the first `.cpu()` of a result
        waits for the kernels; three more copies of a single query's few hundred bytes cost ~10 us each)."""
        if self.packed is None:
            return (self.ids.cpu().numpy(), self.vals.cpu().numpy(), self.mask.cpu().numpy(), self.count.cpu().numpy())
        return packed_views(self.packed.cpu().numpy(), *self.ids.shape)


def _stream() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


class HybridEngine:
    def __init__(self, dense: Optional[_native.DenseIndex], bm25: Optional[_native.BM25Index],
                 maxsim: Optional[_native.MaxSimIndex] = None, *, device: int = 0,
                 dense_row2uid: Optional[torch.Tensor] = None, bm25_row2uid: Optional[torch.Tensor] = None,
                 colbert_row2uid: Optional[torch.Tensor] = None, shard_offset: Optional[int] = None,
                 shard_group=None, tokenizer: Optional[_native.DeviceTokenizer] = None):
        if not torch.cuda.is_available():
            raise RuntimeError("HybridEngine needs a GPU (no CPU fallback)")
        self.dense, self.bm25, self.maxsim = dense, bm25, maxsim
        self.device = int(device)
        self.tdev = torch.device("cuda", self.device)
        self.maps = (dense_row2uid, bm25_row2uid, colbert_row2uid)
        self._bufs = {}
        self._xcache = {}  # argument blocks of the shard exchange (sharding.exchange_topk_native)
        # Row-sharded corpus (retrieval/sharding.py): the three indexes hold this rank's row block (local ids
        # 0 .. n_r - 1 = global ids shard_offset ..); search_batch then all-gathers the packed per-channel lists
        # ONCE per batch, merges W*k -> k per channel (merge_parts_kernel) and fuses the GLOBAL lists — the
        # result is identical on every rank.  None: one index holds everything, nothing is exchanged.
        self.shard_offset, self.shard_group = shard_offset, shard_group
        # the BM25 query side on the device (text-in steps, q_text=): a copy of the BM25 vocabulary's host tokeniser
        self.tokenizer = tokenizer
        # the graph channel (graph_topk): a GraphIndex over the dense matrix's rows and its per-call parameters
        self.graph: Optional[_native.GraphIndex] = None
        self.graph_params: Optional[_native.GraphParams] = None
        self.graph_limit = 0
        self._graph_key = None
        self._side_stream: Optional[torch.cuda.Stream] = None  # made by the first CHANNELS_SIDE step
        self.scope: Optional[_native.ScopeWorkspace] = None  # made by the first scoped call / reserve(rows_max=)

    def _buf(self, name, shape, dtype):
        key = (name, tuple(shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=self.tdev)
            self._bufs[key] = t
        return t

    def _pinned(self, name, nbytes: int):
        """A page-locked host buffer of at least nbytes (grown geometrically, reused): staging for the one H2D copy of a
        batch's BM25 query CSR and the one D2H copy of its results — copies from / to pageable memory go through the
        driver's own bounce buffer synchronously."""
        key = ("pin", name)
        t = self._bufs.get(key)
        if t is None or t.numel() < nbytes:
            t = torch.empty((max(int(nbytes), 2 * (t.numel() if t is not None else 0), 4096),), dtype=torch.uint8).pin_memory()
            self._bufs[key] = t
        return t

    def _staging(self, name: str, nbytes: int):
        """The next of TWO (pinned host, device) staging pairs of `name`, each of at least nbytes.  Uploads alternate
        between the pairs, and before a pair's pinned half is refilled the host waits on the event recorded behind the
        copy it carried two uploads ago: bytes the GPU has not read yet are never overwritten, however far ahead of the
        stream the caller enqueues.  Returns (host, dev, event to record behind the new copy)."""
        slot = self._bufs.get(("slot", name), 1) ^ 1
        self._bufs[("slot", name)] = slot
        ev = self._bufs.get(("ev", name, slot))
        if ev is None:
            ev = torch.cuda.Event()
            self._bufs[("ev", name, slot)] = ev
        ev.synchronize()  # (an event never recorded: returns at once)
        host = self._pinned(f"{name}{slot}", nbytes)
        dev = self._bufs.get(("dev", name, slot))
        if dev is None or dev.numel() < nbytes:
            dev = torch.empty((host.numel(),), dtype=torch.uint8, device=self.tdev)
            self._bufs[("dev", name, slot)] = dev
        return host, dev, ev

    def _send(self, host, dev, ev, nbytes: int):
        dev[:nbytes].copy_(host[:nbytes], non_blocking=True)
        ev.record(torch.cuda.current_stream(self.tdev))

    def upload_csr(self, q_ptr, q_terms):
        """BM25 query CSR (numpy int64 [n+1], int32 [total]) -> device tensors through ONE pinned staging copy, enqueued
        on the current stream.  Back-to-back batches may be enqueued without synchronising: the staging is a ring of two
        (pinned, device) pairs fenced by events (_staging), so the returned tensors hold this batch's CSR until two more
        upload_csr calls have been made; work that reads them must be enqueued before then on the same stream."""
        qp8, qt8 = q_ptr.view(np.uint8), q_terms.view(np.uint8)
        n1, n2 = qp8.size, qt8.size
        host, dev, ev = self._staging("csr", n1 + n2)
        hv = host.numpy()
        hv[:n1] = qp8
        hv[n1:n1 + n2] = qt8
        self._send(host, dev, ev, n1 + n2)
        return dev[:n1].view(torch.int64), dev[n1:n1 + n2].view(torch.int32)

    def upload_scopes(self, scope_ptr, rows, qscope, channel: int = 0):
        """A scope table (numpy: scope_ptr int64 [n_scopes + 1], rows int64, qscope int32 [nq]; retrieval/scope.py
        ScopeResolver.table) -> the device table the scoped channels take, (scope_ptr, rows, qscope, n_scopes, rows_max),
        through ONE pinned staging copy enqueued on the current stream.  The same contract as upload_csr: a ring of two
        staging pairs fenced by events, so the table holds until two more upload_scopes calls of the same `channel`; work
        that reads it must be enqueued before then on the same stream.  channel (0 dense, 1 BM25, 2 ColBERT): one ring
        each, so that the three tables of a step whose channels have different row spaces are live together."""
        scope_ptr, rows, qscope, rows_max = _native.check_scope_table(scope_ptr, rows, qscope)
        sp8, rw8, qs8 = scope_ptr.view(np.uint8), rows.view(np.uint8), qscope.view(np.uint8)
        n1, n2, n3 = sp8.size, rw8.size, qs8.size
        host, dev, ev = self._staging(f"scp{int(channel)}_", n1 + n2 + n3)
        hv = host.numpy()
        hv[:n1] = sp8
        hv[n1:n1 + n2] = rw8
        hv[n1 + n2:n1 + n2 + n3] = qs8
        self._send(host, dev, ev, n1 + n2 + n3)
        return (dev[:n1].view(torch.int64), dev[n1:n1 + n2].view(torch.int64), dev[n1 + n2:n1 + n2 + n3].view(torch.int32),
                int(scope_ptr.size) - 1, rows_max)

    def _grown(self, name: str, nbytes: int) -> torch.Tensor:
        """A device byte buffer of at least nbytes under `name` (grown geometrically, reused)."""
        t = self._bufs.get(("grow", name))
        if t is None or t.numel() < nbytes:
            t = torch.empty((max(int(nbytes), 2 * (t.numel() if t is not None else 0), 4096),), dtype=torch.uint8,
                            device=self.tdev)
            self._bufs[("grow", name)] = t
        return t

    def check_term_scopes(self) -> None:
        """ValueError unless term_scopes() can run on this engine; launches nothing."""
        if self.shard_offset is not None:
            raise ValueError("term constraints do not run on a row-sharded engine (base rows and the table are global)")
        if self.bm25 is None:
            raise ValueError("term constraints need the BM25 index (they are resolved on its resident postings)")

    def term_scopes(self, table):
        """Term constraints -> the scope table of the scoped channels, on the device, on the current stream, without a host
        synchronise.  table: retrieval/terms.py pack() — the operand arrays, each question's constraint and the host bounds.
        The operands go up through ONE pinned staging copy (the ring of upload_scopes: they hold until two more term_scopes
        calls).  Returns ((scope_ptr, rows, qscope, n_scopes, rows_max), status): the 5-tuple upload_scopes returns —
        n_scopes = the constraint count, rows_max = cand_max — which search_batch(scopes=) and capture take as they take an
        uploaded table (the channels must share the BM25 index's chunk list), and the status tensor i32 (0; 1 / 2: cand_max
        / rows_cap exceeded — never with pack()'s bounds on the index they were computed from).  The outputs are this
        engine's buffers: they hold until the next term_scopes call.
        The chain: the table's LIST STEPS, each three launches, write the lists of its phrases and Nears, its unions (a
        Prefix or a OneOf) and its class spans (a PhraseOf or a NearOf) back to back into ONE list array, in that order —
        the first step present starts the array, every later one continues it behind the n_before lists written so far —
        and the term step (amdr_term_scope_device; with lists amdr_term_scope_lists_device) reads list x as the term
        n_terms + x.  The steps, each only when the table has its items:
          span    amdr_span_lists_device over the phrases (kind 0) and then the Nears; a table without a Near takes
                  amdr_phrase_lists_device over its phrases instead.  Needs the token stream (BM25Index.set_tokens).
          union   amdr_union_lists_device; needs no token stream.
          class   amdr_class_spans_device; its classes are the unions (cls_first = the span step's lists) and it reads
                  their lists where the union step wrote them.  Needs the token stream.
          unit    amdr_unit_spans_device over the Withins, behind the class spans, with the same classes.  Needs the token
                  stream and its break flags (BM25Index.set_breaks).
        The array is sized for the steps' row bounds together, and the status tensor holds the constraints' words and then
        each step's, in list order: i32 [n_cons + n_phr + n_near + n_union + n_cspan + n_unit]."""
        self.check_term_scopes()
        n_cons, cand_max, rows_cap = int(table.n_cons), int(table.cand_max), int(table.rows_cap)
        n_phr = int(getattr(table, "n_phr", 0))
        n_near = int(getattr(table, "n_near", 0))
        n_union = int(getattr(table, "n_union", 0))
        n_cspan = int(getattr(table, "n_cspan", 0))
        n_unit = int(getattr(table, "n_unit", 0))
        n_span = n_phr + n_near
        n_x = n_span + n_union + n_cspan + n_unit  # the virtual lists of the term step
        span_cap = (int(table.span_rows_cap) if n_near else int(table.phr_rows_cap)) if n_x else 0
        list_cap = (span_cap + int(getattr(table, "union_rows_cap", 0)) + (int(table.cspan_rows_cap) if n_cspan else 0)
                    + (int(table.unit_rows_cap) if n_unit else 0))
        # The list steps in call order: (name, operands: item_ptr i64 and then i32 arrays, item count, n_before, the key of
        # its grown workspace, plan() -> bytes, call(operand pointers, at, the output and workspace arguments)).
        steps = []
        if n_near:
            p_max = int(table.span_cand_max)
            steps.append(("span", table.span_ops, n_span, 0, "phw", lambda: _native.span_lists_plan(n_span, p_max),
                          lambda ops, at, out: self.bm25.span_lists_device(*ops, n_span, p_max, span_cap, *out)))
        elif n_phr:
            p_max = int(table.phr_cand_max)
            steps.append(("span", table.phr_ops, n_phr, 0, "phw", lambda: _native.phrase_lists_plan(n_phr, p_max),
                          lambda ops, at, out: self.bm25.phrase_lists_device(*ops, n_phr, p_max, span_cap, *out)))
        if n_union:
            steps.append(("union", table.union_ops, n_union, n_span, "unw",
                          lambda: _native.union_lists_plan(n_union, int(self.bm25.n_docs)),
                          lambda ops, at, out: self.bm25.union_lists_device(*ops, n_union, n_span, list_cap, *out)))
        if n_cspan:
            c_max = int(table.cspan_cand_max)
            steps.append(("class", table.cspan_ops, n_cspan, n_span + n_union, "csw",
                          lambda: _native.class_spans_plan(n_cspan, c_max),
                          lambda ops, at, out: self.bm25.class_spans_device(
                              *ops, n_cspan, *((at["union0"], at["union1"]) if n_union else (0, 0)), n_union, n_span,
                              n_span + n_union, c_max, list_cap, *out)))
        if n_unit:
            w_max = int(table.unit_cand_max)
            steps.append(("unit", table.unit_ops, n_unit, n_span + n_union + n_cspan, "usw",
                          lambda: _native.unit_spans_plan(n_unit, w_max),
                          lambda ops, at, out: self.bm25.unit_spans_device(
                              *ops, n_unit, *((at["union0"], at["union1"]) if n_union else (0, 0)), n_union, n_span,
                              n_span + n_union + n_cspan, w_max, list_cap, *out)))
        # Staging, the i64 arrays first (every array starts on a multiple of its item size): the term step's, the steps'
        # item_ptr (the last step's first); then the i32 arrays: the term step's, each step's in call order, qscope.
        term_names = ("grp_ptr", "grp_kind", "grp_term_ptr", "grp_terms", "base_ptr", "base_rows", "cons_base")
        term = {n: np.ascontiguousarray(a, dtype=t) for n, a, t in zip(term_names, table.ops, _native.BM25Index.TERM_OPS)}
        wide = [(n, term[n]) for n in ("grp_ptr", "grp_term_ptr", "base_ptr", "base_rows")]
        wide += [(f"{name}0", np.ascontiguousarray(ops[0], dtype=np.int64)) for name, ops, *_ in reversed(steps)]
        narrow = [(n, term[n]) for n in ("grp_kind", "grp_terms", "cons_base")]
        narrow += [(f"{name}{j}", np.ascontiguousarray(ops[j], dtype=np.int32)) for name, ops, *_ in steps
                   for j in range(1, len(ops))]
        narrow.append(("qscope", np.ascontiguousarray(table.qscope, dtype=np.int32)))
        parts = [(n, a.view(np.uint8)) for n, a in wide + narrow]
        total = sum(p.size for _, p in parts)
        host, dev, ev = self._staging("tsc", max(total, 8))
        hv, off, at = host.numpy(), 0, {}
        base = dev.data_ptr()
        for n, p in parts:
            hv[off:off + p.size] = p
            at[n] = base + off
            off += p.size
        self._send(host, dev, ev, max(total, 8))
        o_rows, o_status = 8 * (n_cons + 1), 8 * (n_cons + 1) + 8 * rows_cap
        out = self._grown("tso", o_status + 4 * (n_cons + n_x) + 8)
        lists = None
        if n_x:  # ONE list array: the first step begins it, the later ones continue it
            o_docs = 8 * (n_x + 1)
            pout = self._grown("pho", o_docs + 4 * list_cap + 8)
            x_ptr, x_doc, x_status = pout.data_ptr(), pout.data_ptr() + o_docs, out.data_ptr() + o_status + 4 * n_cons
            for name, ops, _, n_before, key, plan, call in steps:
                w_bytes = plan()
                work = self._grown(key, w_bytes)
                call([at[f"{name}{j}"] for j in range(len(ops))], at,
                     (x_ptr, x_doc, x_status + 4 * n_before, work.data_ptr(), w_bytes, _stream()))
            lists = (x_ptr, x_doc, n_x)
        work_bytes = _native.term_scope_plan(n_cons, cand_max)
        work = self._grown("tsw", work_bytes)
        self.bm25.term_scope_device([at[n] for n in term_names], int(table.n_base), n_cons, int(table.n_groups), cand_max,
                                    rows_cap, out.data_ptr(), out.data_ptr() + o_rows, out.data_ptr() + o_status,
                                    work.data_ptr(), work_bytes, _stream(), lists=lists)
        q0 = at["qscope"] - base
        qn = parts[-1][1].size
        return ((out[:o_rows].view(torch.int64), out[o_rows:o_status].view(torch.int64), dev[q0:q0 + qn].view(torch.int32),
                 n_cons, cand_max), out[o_status:o_status + 4 * (n_cons + n_x)].view(torch.int32))

    def check_facets(self) -> None:
        """ValueError unless facet_counts() can run on this engine; launches nothing."""
        if self.shard_offset is not None:
            raise ValueError("facet counts do not run on a row-sharded engine (base rows and the table are global)")

    def _facet_columns(self, columns: np.ndarray) -> torch.Tensor:
        """The code columns i32 [n_fields, n_rows] on the device: uploaded once per array object (ScopeResolver.code_columns
        hands out one array per resolver and field tuple, read-only) and kept resident with it."""
        held = self._bufs.setdefault(("fcol",), {})
        ent = held.get(id(columns))
        if ent is None or ent[0] is not columns:
            if len(held) >= 8:  # (resolvers of chunk lists that live updates have replaced)
                held.clear()
            # (a writable host copy: torch does not wrap a read-only array)
            ent = held[id(columns)] = (columns, torch.from_numpy(np.array(columns, dtype=np.int32, order="C")).to(self.tdev))
        return ent[1]

    def facet_counts(self, table, columns, n_codes, top: int):
        """Facet counts of a scope table on the device (amdr_facet_counts_device; the rule is in include/amdretrieval.h).
        table: the 5-tuple term_scopes or upload_scopes returned — every constraint of it is counted.  columns: the code
        columns, numpy i32 [n_fields, n_rows] (kept resident, uploaded once per array) or a device tensor of that shape;
        n_codes: the fields' value counts.  The call is enqueued on the current stream behind whatever wrote the table,
        without a host synchronise, and its outputs ride ONE copy into pinned memory enqueued behind it.  Returns fetch():
        it waits for that copy and returns (total i64 [n_cons], missing i64 [n_cons, F], distinct i32 [n_cons, F], code i32
        [n_cons, F, top], count i64 [n_cons, F, top]) as numpy arrays of the caller's own.  The outputs are this engine's
        buffers: they hold until the next facet_counts call."""
        self.check_facets()
        sp, rw, _, n_cons, rows_max = table
        n_cons, top = int(n_cons), int(top)
        cols = columns if torch.is_tensor(columns) else self._facet_columns(columns)
        assert cols.is_cuda and cols.dtype == torch.int32 and cols.dim() == 2 and cols.is_contiguous()
        n_fields, n_rows = int(cols.shape[0]), int(cols.shape[1])
        n_codes = [int(x) for x in n_codes]
        if len(n_codes) != n_fields:
            raise ValueError("facet_counts: one n_codes entry per code column")
        cf = n_cons * n_fields
        # i64 first: total [n_cons] | missing [cf] | count [cf, top]; then i32: distinct [cf] | code [cf, top]
        o_missing, o_count = 8 * n_cons, 8 * (n_cons + cf)
        o_distinct = o_count + 8 * cf * top
        o_code, nbytes = o_distinct + 4 * cf, o_distinct + 4 * cf + 4 * cf * top
        out = self._grown("fco", nbytes + 8)
        work_bytes = _native.facet_plan(n_cons, n_codes)
        work = self._grown("fcw", work_bytes + 8)
        base = out.data_ptr()
        with torch.cuda.device(self.tdev):
            _native.facet_counts_device(sp.data_ptr(), rw.data_ptr(), n_cons, int(rows_max), cols.data_ptr(), n_rows, n_codes,
                                        top, base, base + o_missing, base + o_distinct, base + o_code, base + o_count,
                                        work.data_ptr(), work_bytes, _stream())
        host = self._pinned("fcoh", max(nbytes, 8))
        host[:nbytes].copy_(out[:nbytes], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.tdev))

        def fetch():
            ev.synchronize()
            h = host.numpy()
            return (h[:o_missing].view(np.int64).copy(), h[o_missing:o_count].view(np.int64).reshape(n_cons, n_fields).copy(),
                    h[o_distinct:o_code].view(np.int32).reshape(n_cons, n_fields).copy(),
                    h[o_code:nbytes].view(np.int32).reshape(n_cons, n_fields, top).copy(),
                    h[o_count:o_distinct].view(np.int64).reshape(n_cons, n_fields, top).copy())
        return fetch

    def upload_text(self, ptrs, lens, total: int):
        """Query texts (UTF-8 pointer / length arrays, _native.utf8_views) -> (blob u8 [total], offs i64 [n + 1]) on the
        device: packed straight into pinned staging (amdr_tokenizer_pack: offsets first, then the bytes) and sent up
        by ONE host-to-device copy on the current stream.  The same contract as upload_csr: back-to-back batches need no
        synchronisation, the returned tensors hold this batch's text until two more upload_text calls."""
        n = int(ptrs.shape[0])
        n1 = (n + 1) * 8
        nbytes = n1 + int(total)
        host, dev, ev = self._staging("txt", nbytes)
        base = host.data_ptr()
        _native.pack_utf8(ptrs, lens, base + n1, int(total), base)
        self._send(host, dev, ev, nbytes)
        return dev[n1:nbytes], dev[:n1].view(torch.int64)

    def tokenize_device(self, blob: torch.Tensor, offs: torch.Tensor):
        """BM25 query side of a text-in step on the device: (q_terms i32, q_ptr i64 [nq + 1], needs_segmenter i32 [nq])
        from the UTF-8 blob and its offsets (device tensors; nq = offs.numel() - 1, n_bytes = blob.numel()).  q_terms
        is the whole term buffer (sized from the reserve: tokens <= bytes); q_ptr says which part is used.  A query that
        holds a Han character gets needs_segmenter = 1 and no terms (the caller decides what to do with it) — unless the
        tokeniser is a copy of a host tokeniser in a Han mode (_native.Tokenizer(han=)), which cuts it: flag 0, terms."""
        if self.tokenizer is None:
            raise RuntimeError("tokenize_device: this engine has no device tokeniser (HybridEngine(..., tokenizer=))")
        assert blob.is_cuda and blob.element_size() == 1 and offs.is_cuda and offs.dtype == torch.int64
        nq, n_bytes = int(offs.numel()) - 1, int(blob.numel())
        tok = self.tokenizer
        if nq > tok.nq_max or n_bytes > tok.bytes_max:
            tok.reserve(max(nq, tok.nq_max), max(n_bytes, tok.bytes_max))  # eager first use (capture() reserves first)
        tt = self._buf("tkt", (max(tok.bytes_max, 1),), torch.int32)
        tp = self._buf("tkp", (nq + 1,), torch.int64)
        tf = self._buf("tkf", (max(nq, 1),), torch.int32)
        tok.encode_device(blob, offs.contiguous(), tt, tp, tf[:nq], nq=nq, n_bytes=n_bytes, stream=_stream())
        return tt, tp, tf[:nq]

    def compact_to_host(self, res: "BatchResult", w: int):
        """(rows i64 [nq, w], scores f64 [nq, w], channel mask i32 [nq, w], count i32 [nq]) of a fused result on the host:
        compacted by ONE kernel (amdr_fuse_compact_device), ONE copy into pinned memory, one synchronise."""
        nq, mo = res.ids.shape
        w = max(1, min(int(w), int(mo)))
        o1, o2, o3, tot = packed_layout(nq, w, 1)
        pk = self._buf("cpk", (tot,), torch.uint8)
        base = pk.data_ptr()
        _native.fuse_compact_device(nq, mo, w, res.ids.data_ptr(), res.vals.data_ptr(), res.mask.data_ptr(),
                                    res.count.data_ptr(), base, base + o1, base + o2, base + o3, device=self.device,
                                    stream=_stream())
        host = self._pinned("cpkh", tot)
        host[:tot].copy_(pk, non_blocking=True)
        torch.cuda.current_stream(self.tdev).synchronize()
        return tuple(v.copy() for v in packed_views(host.numpy(), nq, w, 1))

    def reserve(self, nq: int, k: int, total_terms: int = 0, bytes_max: int = 0, rows_max: int = 0) -> None:
        """bytes_max > 0: text-in steps of up to that many bytes of query text (q_text); BM25 then takes up to bytes_max
        terms (tokens <= bytes).  rows_max > 0: scoped steps (search_batch(scopes=)) whose longest scope has up to that
        many rows."""
        if rows_max > 0:
            self._scope_reserve(nq, k, rows_max)
        if bytes_max > 0 and self.tokenizer is not None:
            self.tokenizer.reserve(nq, bytes_max)
            total_terms = max(total_terms, bytes_max)
        if self.dense is not None:
            self.dense.reserve(nq, k)
        if self.bm25 is not None:
            self.bm25.reserve(nq, k, max(total_terms, 1))
        if self.maxsim is not None:
            self.maxsim.reserve(nq, k)
        if self.graph is not None and self.graph_limit > 0:
            self.graph.reserve(nq, k, self.graph_limit)

    # -- graph channel ------------------------------------------------------------
    def set_graph(self, graph: _native.GraphIndex, params: dict, lang: int = -1) -> None:
        """The graph channel of this engine: the GraphIndex and one call's parameters (graph_retriever.graph_call_params);
        the parameter tables go up to the device once per distinct parameter set."""
        key = (id(graph), int(params["limit"]), int(params["default_depth"]), float(params["min_conf"]), int(lang),
               params["rel_max_depth"].tobytes(), params["rel_allowed"].tobytes(), params["rel_weight"].tobytes(),
               params["decay"].tobytes())
        if self.graph is graph and self._graph_key == key:
            return
        tabs = tuple(torch.from_numpy(np.ascontiguousarray(params[n])).to(self.tdev)
                     for n in ("rel_max_depth", "rel_allowed", "rel_weight", "decay"))
        torch.cuda.current_stream(self.tdev).synchronize()
        self.graph, self._graph_tabs, self._graph_key = graph, tabs, key
        self.graph_limit = int(params["limit"])
        self.graph_params = _native.GraphParams(int(params["limit"]), int(params["default_depth"]), int(lang), 0,
                                                float(params["min_conf"]), *(t.data_ptr() for t in tabs))

    def graph_topk(self, seeds: torch.Tensor, seed_count: torch.Tensor, q_emb: torch.Tensor, k: int, seed_n: int,
                   qsel: Optional[torch.Tensor] = None) -> dict:
        """The graph stage on the current stream (amdr_graph_search_device): for g < ng the query q = qsel[g] (default
        g) walks from the first min(seed_n, seed_count[q]) chunk rows of seeds[q] (the fused list: BatchResult ids /
        count) and re-scores the walked articles against q_emb[q] (the non-query embedding of the question).
        Returns the outputs (_native.GraphIndex.OUTS), indexed by g.  Capturable after reserve()."""
        if self.graph is None or self.graph_params is None:
            raise RuntimeError("graph_topk: this engine has no graph channel (set_graph)")
        assert seeds.is_cuda and seeds.dtype == torch.int64 and seeds.is_contiguous() and seed_count.dtype == torch.int32
        _check_emb(q_emb)
        ld = int(seeds.shape[1])
        ng = int(qsel.numel()) if qsel is not None else int(seeds.shape[0])
        if qsel is not None:
            assert qsel.is_cuda and qsel.dtype == torch.int32 and qsel.is_contiguous()
        k = int(k)
        outs = {n: self._buf("g_" + n, (ng,) if n == "count" else (ng, k), getattr(torch, np.dtype(t).name))
                for n, t in zip(_native.GraphIndex.OUTS, _native.GraphIndex._OUT_T)}
        self.graph.search_device(self.dense, q_emb.data_ptr(), qsel.data_ptr() if qsel is not None else 0,
                                 seeds.data_ptr(), seed_count.data_ptr(), ld, min(int(seed_n), ld, _native.GRAPH_MAX_SEEDS),
                                 ng, k, self.graph_params, [outs[n].data_ptr() for n in _native.GraphIndex.OUTS], _stream())
        return outs

    # -- channels (device in, device out) -----------------------------------
    def dense_topk(self, q_emb: torch.Tensor, k: int):
        nq = q_emb.shape[0]
        _check_emb(q_emb)
        s = self._buf("ds", (nq, k), torch.float32)
        i = self._buf("di", (nq, k), torch.int64)
        self.dense.search_device(q_emb.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), _stream())
        return s, i

    def bm25_topk(self, q_terms: torch.Tensor, q_ptr: torch.Tensor, k: int):
        nq = q_ptr.shape[0] - 1
        _check_csr(q_terms, q_ptr)
        s = self._buf("bs", (nq, k), torch.float64)
        i = self._buf("bi", (nq, k), torch.int64)
        self.bm25.search_device(q_terms.data_ptr(), q_ptr.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), _stream())
        return s, i

    def colbert_topk(self, q_tok: torch.Tensor, k: int):
        nq, q_len = q_tok.shape[0], q_tok.shape[1]
        _check_tok(q_tok)
        s = self._buf("cs", (nq, k), torch.float32)
        i = self._buf("ci", (nq, k), torch.int64)
        self.maxsim.search_device(q_tok.data_ptr(), nq, q_len, k, s.data_ptr(), i.data_ptr(), _stream())
        return s, i

    # -- scoped channels: each query's top-k among its OWN rows (table: upload_scopes) ---------------------------------
    def _scope_ws(self) -> "_native.ScopeWorkspace":
        if self.shard_offset is not None:
            raise ValueError("scoped search does not run on a row-sharded index (a scope's rows are global)")
        if self.scope is None:
            self.scope = _native.ScopeWorkspace(device=self.device)
        return self.scope

    def _scope_reserve(self, nq: int, k: int, rows_max: int) -> "_native.ScopeWorkspace":
        """The workspace with a reserve that covers (nq, k, rows_max) and everything reserved before (never shrinks)."""
        ws = self._scope_ws()
        if nq > ws.nq_max or k > ws.k_max or rows_max > ws.rows_max:
            ws.reserve(max(nq, ws.nq_max), max(k, ws.k_max), max(rows_max, ws.rows_max))
        return ws

    def _scope_call(self, table, nq: int, k: int):
        """The workspace, grown eagerly when the call exceeds its reserve (capture() reserves first), and the table as
        the pointers the native call takes."""
        sp, rw, qs, n_scopes, rows_max = table
        assert sp.is_cuda and sp.dtype == torch.int64 and rw.dtype == torch.int64 and qs.dtype == torch.int32, "scope table"
        assert int(qs.numel()) == nq, "scope table: one qscope entry per query"
        ws = self._scope_reserve(nq, k, rows_max)
        return ws, (sp.data_ptr(), rw.data_ptr(), qs.data_ptr(), int(n_scopes), int(rows_max))

    def dense_topk_scoped(self, q_emb: torch.Tensor, k: int, table):
        nq = q_emb.shape[0]
        _check_emb(q_emb)
        ws, tb = self._scope_call(table, nq, k)
        s = self._buf("sds", (nq, k), torch.float32)
        i = self._buf("sdi", (nq, k), torch.int64)
        ws.dense_search_device(self.dense, q_emb.data_ptr(), tb, nq, k, s.data_ptr(), i.data_ptr(), _stream())
        return s, i

    def bm25_topk_scoped(self, q_terms: torch.Tensor, q_ptr: torch.Tensor, k: int, table):
        nq = q_ptr.shape[0] - 1
        _check_csr(q_terms, q_ptr)
        ws, tb = self._scope_call(table, nq, k)
        s = self._buf("sbs", (nq, k), torch.float64)
        i = self._buf("sbi", (nq, k), torch.int64)
        ws.bm25_search_device(self.bm25, q_terms.data_ptr(), q_ptr.data_ptr(), tb, nq, k, s.data_ptr(), i.data_ptr(),
                              _stream())
        return s, i

    def colbert_topk_scoped(self, q_tok: torch.Tensor, k: int, table):
        nq, q_len = q_tok.shape[0], q_tok.shape[1]
        _check_tok(q_tok)
        ws, tb = self._scope_call(table, nq, k)
        s = self._buf("scs", (nq, k), torch.float32)
        i = self._buf("sci", (nq, k), torch.int64)
        ws.maxsim_search_device(self.maxsim, q_tok.data_ptr(), q_len, tb, nq, k, s.data_ptr(), i.data_ptr(), _stream())
        return s, i

    def hybrid_scoped(self, params: _native.FuseParams, q_emb: torch.Tensor, q_terms: torch.Tensor, q_ptr: torch.Tensor,
                      k: int, dense_table, bm25_table, colbert=None):
        """dense_topk_scoped + bm25_topk_scoped + fuse as ONE native call (amdr_hybrid_scope_device: one launch when both
        tables' scopes fit a slab of their channel and all candidates of a query fit the packed fusion; the separate
        calls inside otherwise): (dense lists, BM25 lists, result).  colbert = the finished lists of colbert_topk_scoped,
        enqueued earlier on the stream.  Same results as the separate calls, bit for bit."""
        nq = int(q_emb.shape[0])
        _check_emb(q_emb)
        _check_csr(q_terms, q_ptr)
        assert q_ptr.shape[0] - 1 == nq
        ws, td = self._scope_call(dense_table, nq, k)
        ws, tb = self._scope_call(bm25_table, nq, k)
        ds = self._buf("sds", (nq, k), torch.float32)
        di = self._buf("sdi", (nq, k), torch.int64)
        bs = self._buf("sbs", (nq, k), torch.float64)
        bi = self._buf("sbi", (nq, k), torch.int64)
        kc = int(colbert[1].shape[1]) if colbert is not None else 0
        pk, ids, vals, mask, count = self._fused_outputs(nq, 2 * k + kc)
        maps = tuple(m.data_ptr() if m is not None else 0 for m in self.maps[:3])
        ws.hybrid(self.dense, self.bm25, params, q_emb.data_ptr(), q_terms.data_ptr(), q_ptr.data_ptr(), td, tb, nq, k, k,
                  maps, (colbert[1].data_ptr(), colbert[0].data_ptr(), kc) if colbert is not None else None,
                  (ds.data_ptr(), di.data_ptr(), bs.data_ptr(), bi.data_ptr()),
                  (ids.data_ptr(), vals.data_ptr(), mask.data_ptr(), count.data_ptr()), _stream())
        return (ds, di), (bs, bi), BatchResult(ids=ids, vals=vals, mask=mask, count=count, packed=pk)

    # -- fusion ---------------------------------------------------------------
    def fuse(self, params: _native.FuseParams, nq: int, dense=None, bm25=None, colbert=None) -> BatchResult:
        def chan(c, m):
            if c is None:
                return None, 0
            s, i = c
            return (i.data_ptr(), s.data_ptr(), int(i.shape[1]), m.data_ptr() if m is not None else 0), int(i.shape[1])
        d, kd = chan(dense, self.maps[0])
        b, kb = chan(bm25, self.maps[1])
        c, kc = chan(colbert, self.maps[2])
        mo = kd + kb + kc
        pk, ids, vals, mask, count = self._fused_outputs(nq, mo)
        _native.fuse_device(params, nq, d, b, c, ids.data_ptr(), vals.data_ptr(), mask.data_ptr(), count.data_ptr(),
                            device=self.device, stream=_stream())
        return BatchResult(ids=ids, vals=vals, mask=mask, count=count, packed=pk)

    def _fused_outputs(self, nq: int, mo: int):
        o1, o2, o3, tot = packed_layout(nq, mo)
        pk = self._buf("fpk", (tot,), torch.uint8)  # the four outputs side by side: one D2H serves the host API
        return (pk, pk[:o1].view(torch.int64).view(nq, mo), pk[o1:o2].view(torch.float64).view(nq, mo, NV),
                pk[o2:o3].view(torch.int32).view(nq, mo), pk[o3:].view(torch.int32))

    def dense_topk_fuse(self, params: _native.FuseParams, q_emb: torch.Tensor, k: int, bm25):
        """Dense top-k + fusion with the finished BM25 lists as ONE native call (amdr_dense_search_fuse_device: for the
        serving corpora under a batch one kernel ranks the score rows and fuses).  Same results as dense_topk + fuse."""
        nq = q_emb.shape[0]
        _check_emb(q_emb)
        bs, bi = bm25
        kb = int(bi.shape[1])
        s = self._buf("ds", (nq, k), torch.float32)
        i = self._buf("di", (nq, k), torch.int64)
        pk, ids, vals, mask, count = self._fused_outputs(nq, k + kb)
        m0, m1 = self.maps[0], self.maps[1]
        self.dense.search_fuse_device(params, q_emb.data_ptr(), nq, k,
                                      (bi.data_ptr(), bs.data_ptr(), kb, m1.data_ptr() if m1 is not None else 0),
                                      m0.data_ptr() if m0 is not None else 0, s.data_ptr(), i.data_ptr(), ids.data_ptr(),
                                      vals.data_ptr(), mask.data_ptr(), count.data_ptr(), _stream())
        return (s, i), BatchResult(ids=ids, vals=vals, mask=mask, count=count, packed=pk)

    def hybrid_batch(self, params: _native.FuseParams, q_emb: torch.Tensor, q_terms: torch.Tensor, q_ptr: torch.Tensor, k: int):
        """bm25_topk + dense_topk_fuse as ONE native call (amdr_hybrid_batch_device: on a long batch the BM25 kernel runs
        on a side stream beside the second dense pass, forked and joined inside the call): (dense lists, BM25 lists, result)."""
        nq = int(q_emb.shape[0])
        _check_emb(q_emb)
        _check_csr(q_terms, q_ptr)
        assert q_ptr.shape[0] - 1 == nq
        ds = self._buf("ds", (nq, k), torch.float32)
        di = self._buf("di", (nq, k), torch.int64)
        bs = self._buf("bs", (nq, k), torch.float64)
        bi = self._buf("bi", (nq, k), torch.int64)
        pk, ids, vals, mask, count = self._fused_outputs(nq, 2 * k)
        m0, m1 = self.maps[0], self.maps[1]
        _native.hybrid_batch_device(self.dense, self.bm25, params, q_emb.data_ptr(), q_terms.data_ptr(), q_ptr.data_ptr(),
                                    nq, k, k, m0.data_ptr() if m0 is not None else 0, m1.data_ptr() if m1 is not None else 0,
                                    ds.data_ptr(), di.data_ptr(), bs.data_ptr(), bi.data_ptr(), ids.data_ptr(),
                                    vals.data_ptr(), mask.data_ptr(), count.data_ptr(), _stream())
        return (ds, di), (bs, bi), BatchResult(ids=ids, vals=vals, mask=mask, count=count, packed=pk)

    def _hybrid_small(self, params: _native.FuseParams, q_emb: torch.Tensor, q_terms: torch.Tensor, q_ptr: torch.Tensor,
                      k: int):
        """bm25_topk + dense_topk_fuse through amdr_hybrid_small_device (one launch on a serving corpus): (dense lists,
        BM25 lists, result).  Issued once per query by search(): output tensors and the call's argument block are built
        once per (nq, k)."""
        nq = int(q_emb.shape[0])
        _check_emb(q_emb)
        _check_csr(q_terms, q_ptr)
        assert q_ptr.shape[0] - 1 == nq
        ent = self._xcache.get(("hs", nq, k))
        if ent is None:
            ds = self._buf("ds", (nq, k), torch.float32)
            di = self._buf("di", (nq, k), torch.int64)
            bs = self._buf("bs", (nq, k), torch.float64)
            bi = self._buf("bi", (nq, k), torch.int64)
            pk, ids, vals, mask, count = self._fused_outputs(nq, 2 * k)
            m0, m1 = self.maps[0], self.maps[1]
            plan = _native.hybrid_small_plan(self.dense, self.bm25, nq, k, k, m0.data_ptr() if m0 is not None else 0,
                                             m1.data_ptr() if m1 is not None else 0, ds.data_ptr(), di.data_ptr(),
                                             bs.data_ptr(), bi.data_ptr(), ids.data_ptr(), vals.data_ptr(), mask.data_ptr(),
                                             count.data_ptr())
            ent = (plan, (ids, vals, mask, count, pk), (ds, di, bs, bi))
            self._xcache[("hs", nq, k)] = ent
        plan, (ids, vals, mask, count, pk), (ds, di, bs, bi) = ent
        _native.hybrid_small_device(plan, params, q_emb.data_ptr(), q_terms.data_ptr(), q_ptr.data_ptr(), _stream())
        return (ds, di), (bs, bi), BatchResult(ids=ids, vals=vals, mask=mask, count=count, packed=pk)

    def rerank_blend(self, res: BatchResult, ce_raw: torch.Tensor, beta: float) -> BatchResult:
        nq, mo = res.ids.shape
        assert ce_raw.is_cuda and ce_raw.dtype == torch.float64 and ce_raw.is_contiguous() and ce_raw.shape[0] == nq
        out = self._buf("fr", (nq, mo, 2), torch.float64)
        _native.rerank_blend_device(nq, mo, res.count.data_ptr(), res.ids.data_ptr(), res.vals.data_ptr(),
                                    res.mask.data_ptr(), ce_raw.data_ptr(), int(ce_raw.shape[1]), float(beta),
                                    out.data_ptr(), device=self.device, stream=_stream())
        res.rerank = out
        return res

    # -- diversification ------------------------------------------------------
    def check_diversify(self) -> None:
        """ValueError unless diversify() can run on this engine; launches nothing."""
        if self.shard_offset is not None:
            raise ValueError("diversify: MMR selection does not run on a row-sharded index (the candidate rows are global)")
        if self.maps[0] is not None:
            raise ValueError("diversify: this engine maps dense rows to ids (dense_row2uid); the fused ids are then no "
                             "rows of the chunk matrix")
        if self.dense is None:
            raise ValueError("diversify: MMR selection needs the dense index (the cosine is taken between its rows)")

    def diversify(self, res: BatchResult, k_sel: int, lam: float, pool: int) -> BatchResult:
        """MMR selection over the first `pool` fused hits of every query (amdr_mmr_device on the current stream, after the
        optional rerank blend): a new result of width k_sel that holds the selected hits in selection order — ids / vals /
        mask (/ rerank) gathered by position, count = min(k_sel, count, pool), -1 / 0 past it — with mmr_pos / mmr /
        mmr_max_sim beside it.  The fused ids are rows of the dense matrix (no dense_row2uid map, not row-sharded:
        ValueError).  Needs no reserve; capturable."""
        self.check_diversify()
        nq, mo = (int(x) for x in res.ids.shape)
        pool = max(1, min(int(pool), mo, _native.MMR_MAX_POOL))
        k_sel = max(1, min(int(k_sel), pool))
        o1, o2, o3, tot = packed_layout(nq, k_sel)
        pk = self._buf("mpk", (tot,), torch.uint8)
        ids, vals = pk[:o1].view(torch.int64).view(nq, k_sel), pk[o1:o2].view(torch.float64).view(nq, k_sel, NV)
        mask, count = pk[o2:o3].view(torch.int32).view(nq, k_sel), pk[o3:].view(torch.int32)
        pos = self._buf("mpos", (nq, k_sel), torch.int32)
        val = self._buf("mval", (nq, k_sel), torch.float64)
        sim = self._buf("msim", (nq, k_sel), torch.float64)
        self.dense.mmr_device(res.ids, res.vals[:, :, _native.FV["score"]], res.count, nq, pool, k_sel, float(lam), pos, val,
                              sim, count, ld_rows=mo, stream=_stream())
        # the reorder: gathers on the same stream (a fused reorder kernel is not part of this stage)
        none = self._buf("mnone", (nq, k_sel), torch.bool)
        torch.lt(pos, 0, out=none)
        at = self._buf("mat", (nq, k_sel), torch.int64)
        at.copy_(pos)
        at.clamp_(min=0)
        torch.gather(res.ids, 1, at, out=ids)
        ids.masked_fill_(none, -1)
        torch.gather(res.mask, 1, at, out=mask)
        mask.masked_fill_(none, 0)
        torch.gather(res.vals, 1, at[:, :, None].expand(nq, k_sel, NV), out=vals)
        vals.masked_fill_(none[:, :, None], 0.0)
        out = BatchResult(ids=ids, vals=vals, mask=mask, count=count, packed=pk, mmr_pos=pos, mmr=val, mmr_max_sim=sim)
        for name in ("dense_ids", "dense_scores", "bm25_ids", "bm25_scores", "colbert_ids", "colbert_scores",
                     "needs_segmenter", "graph"):
            setattr(out, name, getattr(res, name))
        if res.rerank is not None:
            out.rerank = self._buf("mrr", (nq, k_sel, 2), torch.float64)
            torch.gather(res.rerank, 1, at[:, :, None].expand(nq, k_sel, 2), out=out.rerank)
            out.rerank.masked_fill_(none[:, :, None], math.nan)
        return out

    # -- whole pipeline ---------------------------------------------------------
    def search_batch(self, params: _native.FuseParams, k: int, *, q_emb: Optional[torch.Tensor] = None,
                     q_terms: Optional[torch.Tensor] = None, q_ptr: Optional[torch.Tensor] = None,
                     q_tok: Optional[torch.Tensor] = None, q_text=None, scopes=None, diversity=None) -> BatchResult:
        """dense + bm25 (+ colbert) top-k -> fuse -> min_final filter, all on device.
        q_text = (blob u8, offs i64 [nq + 1]) device tensors: the BM25 query side as text, tokenised on the device
        (tokenize_device) in the same stream, instead of q_terms / q_ptr.
        scopes = (dense table, BM25 table, ColBERT table) (upload_scopes; one per channel's row space, None for a
        channel that is off): every channel ranks each query's own rows and the fusion — its normalisation included —
        runs over those lists (the SCOPED form).  Not on a row-sharded engine (ValueError).
        diversity = (k_sel, lam, pool): the step ends with diversify(); None: the same launches as ever."""
        flags = None
        if diversity is not None:
            self.check_diversify()  # (before any launch)
        if q_text is not None:
            if q_terms is not None or q_ptr is not None:
                raise ValueError("search_batch: pass q_text or q_terms / q_ptr, not both")
            q_terms, q_ptr, flags = self.tokenize_device(*q_text)
        # a channel runs when it has both an index and an operand
        d_on = self.dense is not None and q_emb is not None
        b_on = self.bm25 is not None and q_ptr is not None
        c_on = self.maxsim is not None and q_tok is not None
        nq = int(q_tok.shape[0] if c_on else q_ptr.shape[0] - 1 if b_on else q_emb.shape[0])
        form, exchange = step_form(d_on, b_on, c_on, self.shard_offset is not None, nq, k,
                                   c_on and os.environ.get("AMDR_ENGINE_OVERLAP", "1") != "0")
        d = b = c = None
        if scopes is not None:
            if self.shard_offset is not None:
                raise ValueError("search_batch(scopes=): scoped search does not run on a row-sharded engine")
            form = SCOPED
            for on, tb, who in zip((d_on, b_on, c_on), scopes, ("dense", "BM25", "ColBERT")):
                if on and tb is None:
                    raise ValueError(f"search_batch(scopes=): the {who} channel runs but has no scope table")
        if form == SCOPED and d_on and b_on:  # one call: dense + BM25 + fusion behind the ColBERT lists, if any
            if c_on:
                c = self.colbert_topk_scoped(q_tok, k, scopes[2])
            d, b, res = self.hybrid_scoped(params, q_emb, q_terms, q_ptr, k, scopes[0], scopes[1], c)
        elif form == SCOPED:  # short launches on the caller's stream (regions of one workspace: no ordering needed)
            if d_on:
                d = self.dense_topk_scoped(q_emb, k, scopes[0])
            if b_on:
                b = self.bm25_topk_scoped(q_terms, q_ptr, k, scopes[1])
            if c_on:
                c = self.colbert_topk_scoped(q_tok, k, scopes[2])
            res = self.fuse(params, nq, d, b, c)
        elif form == ONE_LAUNCH:  # the serving call (search(): one query at a time)
            d, b, res = self._hybrid_small(params, q_emb, q_terms, q_ptr, k)
        elif form == BM25_THEN_FUSED:
            d, b, res = self.hybrid_batch(params, q_emb, q_terms, q_ptr, k)
        else:
            side = None
            if form == CHANNELS_SIDE:
                # the two short channels on a side stream, forked from and joined to the caller's: inside a hipGraph
                # capture the fork / join become edges
                main = torch.cuda.current_stream(self.tdev)
                if self._side_stream is None:
                    self._side_stream = torch.cuda.Stream(device=self.tdev)
                side = self._side_stream
                side.wait_stream(main)
            with torch.cuda.stream(side):  # (None: the caller's stream)
                if d_on:
                    d = self.dense_topk(q_emb, k)
                if b_on:
                    b = self.bm25_topk(q_terms, q_ptr, k)
            if c_on:
                c = self.colbert_topk(q_tok, k)
            if side is not None:
                main.wait_stream(side)
            if exchange:
                from . import sharding
                chans = [x for x in (d, b, c) if x is not None]
                merged = iter(sharding.exchange_topk(chans, int(self.shard_offset), group=self.shard_group, buf=self._buf,
                                                     cache=self._xcache))
                d, b, c = (next(merged) if x is not None else None for x in (d, b, c))
            res = self.fuse(params, nq, d, b, c)
        if d is not None:
            res.dense_scores, res.dense_ids = d
        if b is not None:
            res.bm25_scores, res.bm25_ids = b
        if c is not None:
            res.colbert_scores, res.colbert_ids = c
        res.needs_segmenter = flags
        return res if diversity is None else self.diversify(res, *diversity)

    # -- hipGraph form -----------------------------------------------------------
    def capture(self, params: _native.FuseParams, k: int, *, q_emb: Optional[torch.Tensor] = None,
                q_terms: Optional[torch.Tensor] = None, q_ptr: Optional[torch.Tensor] = None,
                q_tok: Optional[torch.Tensor] = None, q_text=None, graph: Optional[dict] = None, scopes=None,
                diversity=None):
        """Record one search_batch over the given tensors into a hipGraph.

        Returns (graph, result): `graph.replay()` re-runs the whole step — every kernel of every
        stage — as ONE launch on the current stream; new queries are written INTO the same input
        tensors (same nq; the BM25 term array may hold any number of terms up to its length).
        The "_device" entry points only enqueue and, after reserve(), allocate nothing
        (include/amdretrieval.h), which is what makes the step capturable.  A step of 4-5 short
        kernels is launch-bound at small batch: replay removes the per-kernel launch gaps.  (Measured: the BM25
        channel on a forked branch of the captured graph — it does not depend on the dense channel — replays in
        45 us against 33 us for the plain chain: the fork / join nodes cost more than the 5-us kernel they hide.)
        With q_text = (blob, offs) the graph starts from query BYTES: tokeniser + channels + fusion; a replay takes new
        text written into the same two tensors (same nq, at most blob.numel() bytes, offs[nq] <= that).
        graph = dict(q_emb=, k=, seed_n=, qsel=None): the step ends with graph_topk over the fused list (set_graph
        first); its outputs are result.graph.
        scopes: the scoped step (search_batch); a replay takes new tables written INTO the same table tensors (same
        nq; every scope at most the tables' rows_max rows, scope_ptr / rows within the tensors' lengths).
        diversity = (k_sel, lam, pool): the step ends with diversify() — behind the graph stage, whose seeds are the
        fused list as it was ranked; the MMR kernel has no workspace, so nothing more is reserved.
        """
        if self.shard_offset is not None:
            raise RuntimeError("capture: a sharded step contains a collective; it is not recorded into a hipGraph")
        if q_text is not None:
            nq = int(q_text[1].numel()) - 1
            self.reserve(nq, int(k), 0, bytes_max=max(int(q_text[0].numel()), 1))
        else:
            nq = (q_emb.shape[0] if q_emb is not None else q_ptr.shape[0] - 1 if q_ptr is not None else q_tok.shape[0])
            self.reserve(int(nq), int(k), int(q_terms.numel()) if q_terms is not None else 0)
        if scopes is not None:
            self._scope_reserve(int(nq), int(k), max(1, max(int(tb[4]) for tb in scopes if tb is not None)))
        gstage = graph
        if gstage is not None:
            ng = int(gstage["qsel"].numel()) if gstage.get("qsel") is not None else int(nq)
            self.graph.reserve(ng, int(gstage["k"]), self.graph_limit)

        def step():
            r = self.search_batch(params, k, q_emb=q_emb, q_terms=q_terms, q_ptr=q_ptr, q_tok=q_tok, q_text=q_text,
                                  scopes=scopes)
            if gstage is not None:
                r.graph = self.graph_topk(r.ids, r.count, gstage["q_emb"], gstage["k"], gstage["seed_n"],
                                          qsel=gstage.get("qsel"))
            return r if diversity is None else self.diversify(r, *diversity)
        side = torch.cuda.Stream(device=self.tdev)
        side.wait_stream(torch.cuda.current_stream(self.tdev))
        with torch.cuda.stream(side):  # eager warm-up sizes every lazily grown buffer outside the capture
            step()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            res = step()
        return graph, res

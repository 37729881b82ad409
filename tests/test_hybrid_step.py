"""The host side of one hybrid step, without a GPU: the engine's route (engine.step_form), the ONE layout of the packed
fused record (engine.packed_layout / packed_views, both record forms), the two columnar decoders of
HybridRetriever.search_batch_arrays, and the two ends of a split batch: its partition and the scatter of its columns."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from legal_rag_amd import _native
from legal_rag_amd.retrieval import engine as E
from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever


def restated_form(has_dense, has_bm25, has_colbert, sharded, nq, k, overlap):
    """The conditions HybridEngine.search_batch spelled out inline before the route was pulled out, in their order."""
    if has_dense and has_bm25 and not has_colbert and not sharded:
        if nq <= 4 and 2 * k <= 32:
            return E.ONE_LAUNCH, False
        return E.BM25_THEN_FUSED, False
    side = has_colbert and overlap and (has_dense or has_bm25)
    return (E.CHANNELS_SIDE if side else E.CHANNELS), sharded


def test_step_form_truth_table():
    seen = set()
    for hd, hb, hc, sh, ov in itertools.product((False, True), repeat=5):
        for nq in (1, 4, 5, 96):
            for k in (10, 16, 17):
                got = E.step_form(hd, hb, hc, sh, nq, k, ov)
                assert got == restated_form(hd, hb, hc, sh, nq, k, ov), (hd, hb, hc, sh, nq, k, ov)
                seen.add(got)
    # every form is reached; the exchange comes only with the separate channels
    assert seen == {(E.ONE_LAUNCH, False), (E.BM25_THEN_FUSED, False), (E.CHANNELS, False), (E.CHANNELS, True),
                    (E.CHANNELS_SIDE, False), (E.CHANNELS_SIDE, True)}
    # the edges of the one-launch test: 4 queries and 2 * 16 fused candidates are in, 5 and 2 * 17 are out
    assert E.step_form(True, True, False, False, 4, 16, True)[0] == E.ONE_LAUNCH
    assert E.step_form(True, True, False, False, 5, 16, True)[0] == E.BM25_THEN_FUSED
    assert E.step_form(True, True, False, False, 4, 17, True)[0] == E.BM25_THEN_FUSED


def synthetic_record(nq, w, nvals, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(-1, 1 << 40, size=(nq, w), dtype=np.int64)
    vals = rng.standard_normal((nq, w, nvals) if nvals > 1 else (nq, w))
    mask = rng.integers(0, 8, size=(nq, w), dtype=np.int32)
    count = rng.integers(0, w + 1, size=nq, dtype=np.int32)
    return ids, vals, mask, count


def test_packed_layout_round_trips_both_record_forms():
    for nq, w, nvals in ((1, 1, _native.FUSE_NVALS), (3, 20, _native.FUSE_NVALS), (7, 5, 1), (1, 32, 1)):
        arrs = synthetic_record(nq, w, nvals, nq * 100 + w)
        o1, o2, o3, tot = E.packed_layout(nq, w, nvals)
        assert (o1, o2 - o1, o3 - o2, tot - o3) == tuple(a.nbytes for a in arrs)
        buf = np.concatenate([a.reshape(-1).view(np.uint8) for a in arrs] + [np.full(13, 0xAB, np.uint8)])  # (+ slack)
        for got, exp in zip(E.packed_views(buf, nq, w, nvals), arrs):
            assert got.dtype == exp.dtype and got.shape == exp.shape and (got.view(np.uint8) == exp.view(np.uint8)).all()
        if nvals == _native.FUSE_NVALS:  # BatchResult.to_host reads the same record through the same views
            ids, vals, mask, count = (torch.from_numpy(a) for a in arrs)
            res = E.BatchResult(ids=ids, vals=vals, mask=mask, count=count, packed=torch.from_numpy(buf[:tot].copy()))
            for got, exp in zip(res.to_host(), arrs):
                assert got.dtype == exp.dtype and got.shape == exp.shape and (got.view(np.uint8) == exp.view(np.uint8)).all()


def compact(ids, vals, mask, count, w):
    """amdr_fuse_compact_device restated (csrc/fuse.hip fuse_compact_kernel): the first w hits, -1 / 0 past the count."""
    w = max(1, min(w, ids.shape[1]))
    c = np.minimum(count, w).astype(np.int32)
    keep = np.arange(w)[None, :] < c[:, None]
    return (np.where(keep, ids[:, :w], -1), np.where(keep, vals[:, :w, _native.FV["score"]], 0.0),
            np.where(keep, mask[:, :w], 0).astype(np.int32), c)


def test_lean_columns_equal_the_first_top_k_of_the_full_columns():
    nq, mo = 6, 20
    ids, vals, mask, count = synthetic_record(nq, mo, _native.FUSE_NVALS, 7)
    count[:3] = (0, 4, mo)  # nothing survives / fewer than top_k / every candidate
    exact = np.array([True, False, True, True, False, True])
    chunks = [object()]
    for top_k in (1, 10, 20, 25):
        full = HybridRetriever._decode_columns((ids, vals, mask, count), exact, top_k, chunks)
        lean = HybridRetriever._decode_lean(compact(ids, vals, mask, count, top_k), exact, chunks)
        assert set(lean) == {"rows", "scores", "count", "channel_mask", "zh_exact", "chunks"}
        assert set(full) == set(lean) | {"values", "value_names"}
        w = min(top_k, mo)
        for name, dt in (("rows", np.int64), ("scores", np.float64), ("count", np.int32), ("channel_mask", np.int32)):
            assert lean[name].dtype == full[name].dtype == dt, name
            assert lean[name].shape == full[name].shape == ((nq,) if name == "count" else (nq, w)), name
            assert (lean[name] == full[name]).all(), name
        assert lean["zh_exact"] is exact and full["zh_exact"] is exact and lean["chunks"] is chunks
        assert full["values"].shape == (nq, w, _native.FUSE_NVALS) and full["value_names"] == _native.FV
        assert (full["values"] == vals[:, :w]).all()


# ---- a split batch: the partition and the scatter ------------------------------------------------------------------------
def listed(parts):
    return [(list(idxs), scoped, colbert) for idxs, scoped, colbert in parts]


def test_partition_has_a_fixed_order_and_places_every_question_once():
    from legal_rag_amd.retrieval.scope import Scope
    chunks = [SimpleNamespace(id=f"c{i}", section="A" if i < 3 else "B") for i in range(5)]
    a, b, miss = Scope(section="A"), Scope(section="B"), Scope(section="no such section")
    # {no scope, a scope with rows, a scope that matches nothing} x {blank, not blank}, two of the six twice
    scopes = [b, None, miss, None, b, miss, None, a]
    qs = ["q0", "  ", "q2", "q3", "", None, "q6", "q7"]
    part = HybridRetriever._partition
    for colbert, exp in ((True, [([1], False, False), ([3, 6], False, True), ([4], True, False), ([0, 7], True, True)]),
                         (False, [([1, 3, 6], False, False), ([0, 4, 7], True, False)])):  # channel off: no blank split
        parts, empty = part(qs, scopes, None, chunks, colbert, "search_batch")
        assert listed(parts) == exp and empty == [2, 5]
        assert sorted(i for idxs, _, _ in parts for i in idxs) + empty == [0, 1, 3, 4, 6, 7, 2, 5]  # each index once
        # decisions that ask for no graph change nothing
        assert listed(part(qs, scopes, [SimpleNamespace(mode="RAG")] * 8, chunks, colbert, "search_batch")[0]) == exp
    # no scope and no blank question: ONE part, the whole batch, with and without the list of Nones
    for sc in (None, [None] * 3):
        for colbert in (False, True):
            assert listed(part(["x", "y", "z"], sc, None, chunks, colbert, "search")[0]) == [([0, 1, 2], False, colbert)]
    assert listed(part(["x", " "], None, None, chunks, False, "search")[0]) == [([0, 1], False, False)]
    assert part(["x"], [miss], None, chunks, True, "search") == ([], [0])  # parts without an index are left out
    graph = SimpleNamespace(mode="GRAPH_AUGMENTED")
    assert listed(part(["x", "y"], [None, a], [graph, None], chunks, False, "search_batch")[0]) == \
        [([0], False, False), ([1], True, False)]
    with pytest.raises(ValueError, match="search_batch: scopes must have one entry per question"):
        part(["x", "y"], [None], None, chunks, False, "search_batch")
    with pytest.raises(ValueError, match="search_batch_arrays: decisions must have one entry per question"):
        part(["x", "y"], None, [None], chunks, False, "search_batch_arrays")
    with pytest.raises(TypeError, match=r"scopes\[1\] is not a Scope"):
        part(["x", "y"], [None, "A"], None, chunks, False, "search_batch")
    with pytest.raises(ValueError, match="question 1 has a graph-mode decision and a scope.*graph"):
        part(["x", "y"], [None, miss], [None, graph], chunks, False, "search_batch")


@pytest.mark.parametrize("graph", [False, True], ids=["no-graph-columns", "graph-columns"])
@pytest.mark.parametrize("values", [True, False], ids=["full", "lean"])
@pytest.mark.parametrize("top_k", [1, 10])
def test_scatter_places_the_parts_and_fills_the_rest_from_the_schema(top_k, values, graph):
    from legal_rag_amd.retrieval.hybrid_retriever import COLUMNS
    chunks, rng = [object()], np.random.default_rng(top_k)
    n, at = 6, ([0, 3, 5], [4, 1])  # a plain part of 3, a scoped part of 2; question 2: a scope that matches nothing
    parts = []
    for seed, idxs in enumerate(at):
        rec = synthetic_record(len(idxs), 20, _native.FUSE_NVALS, 50 + seed)
        exact = rng.integers(0, 2, size=len(idxs)).astype(bool)
        parts.append((idxs, HybridRetriever._decode_columns(rec, exact, top_k, chunks) if values
                      else HybridRetriever._decode_lean(compact(*rec, top_k), exact, chunks)))
    names = ["rows", "scores", "count", "channel_mask", "zh_exact"] + ["values"] * values
    if graph:  # the plain part carries the graph columns, the scoped part does not
        for name, dt, _, hit in COLUMNS:
            if name.startswith("graph_"):
                parts[0][1][name] = rng.integers(-1, 50, size=(3,) if hit is None else (3, top_k) + hit).astype(dt)
                names.append(name)
        parts[0][1]["graph_relation_names"] = ["cite", "next"]
    out = HybridRetriever._scatter_columns(n, top_k, values, chunks, parts)
    assert set(out) == set(names) | {"chunks"} | ({"value_names"} if values else set()) | \
        ({"graph_relation_names"} if graph else set())
    assert out["chunks"] is chunks and (not values or out["value_names"] == _native.FV)
    assert not graph or out["graph_relation_names"] == ["cite", "next"]
    schema = {name: rest for name, *rest in COLUMNS}
    assert len(schema) == 13 and set(names) <= set(schema)
    for name in names:
        dt, fill, hit = schema[name]
        assert out[name].dtype == dt and out[name].shape == ((n,) if hit is None else (n, top_k) + hit), name
        rest = np.ones(n, dtype=bool)
        for idxs, cols in parts:
            if name in cols:
                assert cols[name].dtype == dt and out[name][idxs].tobytes() == cols[name].tobytes(), name  # bit for bit
                rest[idxs] = False
        assert rest[2] and (rest[[4, 1]].all() if name.startswith("graph_") else rest.sum() == 1)
        assert (out[name][rest] == fill).all(), name
    # ONE part that holds every question is the result as it is (no copy on the path of a batch that is not split)
    whole = parts[0][1]
    assert HybridRetriever._scatter_columns(3, top_k, values, chunks, [(range(3), whole)]) is whole

"""Withdrawal from a live HybridRetriever: after builders/remove.py remove_chunk_ids ran, the dense matrix and the
ColBERT token store resident in HBM lost the rows in place (amdr_dense_remove, amdr_maxsim_remove: the same native
handles, nothing reloaded), the files hold consistent rows / pids, and the live VectorStore and ColBERTRetriever answer
as retrievers loaded afresh from the rewritten files."""
import json
import shutil

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import assert_hits_equal_mod_ties

pytestmark = pytest.mark.gpu

QUESTIONS = ["what warranty does a merchant give that goods are merchantable", "Short Titles",
             "statute of frauds signed writing sale of goods price of $500", "risk of loss passes to the buyer"]


def dump(h):
    return {"id": h.chunk.id, "score": float(h.score), "rank": h.rank, "source": h.source, "breakdown": h.score_breakdown}


def _cfg(root):
    from legal_rag_amd.config import AppConfig
    cfg = AppConfig.for_data_dir(str(root), "en")
    cfg.retrieval.encoder_backend = "hashing"
    cfg.retrieval.enable_colbert = True
    cfg.retrieval.enable_rerank = False
    return cfg


def _jsonl(path, chunks):
    path.write_text("".join(json.dumps(c.model_dump(), ensure_ascii=False) + "\n" for c in chunks), encoding="utf-8")
    return path


def test_removal_reaches_a_live_hybrid_retriever(tmp_path):
    from pathlib import Path

    from legal_rag_amd import _native, artifacts
    from legal_rag_amd.retrieval.builders.colbert_builder import build_colbert_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    from legal_rag_amd.retrieval.builders.remove import remove_chunk_ids
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    chunks = load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")[:48]
    assert len({c.id for c in chunks}) == 48
    cfg = _cfg(tmp_path / "live")
    build_faiss_index(cfg, chunks)
    assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "all.jsonl", chunks)) == 48
    build_colbert_index(cfg, chunks)
    r = HybridRetriever(cfg)
    assert r.colbert is not None and r.colbert.enabled
    assert all(len(h) > 0 for h in r.search_batch(QUESTIONS, top_k=10))
    assert r.native_engine(with_colbert=True) is not None
    vs, col = r.dense.store, r.colbert
    index, native, searcher = vs.index, vs.index.native, col._searcher
    assert native.ntotal == 48 and searcher.info()[0] == 48 and index.rows_epoch == 0
    probes = [chunks[i].text[:200] for i in (0, 17, 18, 30, 47)] + QUESTIONS

    def channel_hits(q):
        """The ids the dense and the ColBERT channel return for q (host-pointer searches, one query, depth 10)."""
        dense, colbert = vs.search(q, 10), r.search_colbert(q, 10)
        assert dense and colbert
        return {c.id for c, _ in dense} | {h.chunk.id for h in colbert}

    seen = set().union(*(channel_hits(q) for q in probes))
    assert {chunks[i].id for i in (0, 17, 18, 30, 47)} & seen  # the probes do find chunks that are about to go
    files = [Path(cfg.retrieval.faiss_index_file), Path(cfg.retrieval.faiss_meta_file), Path(cfg.retrieval.colbert_meta_file),
             col.index_dir() / "amdr_tokens.npz", Path(cfg.retrieval.bm25_index_file)]

    # ids nobody holds: 0 everywhere, no file touched
    before = [(p.stat().st_mtime_ns, p.stat().st_size) for p in files]
    assert remove_chunk_ids(cfg, ["no-such-chunk", "nor-this-one"]) == {"bm25": 0, "dense": 0, "colbert": 0}
    assert [(p.stat().st_mtime_ns, p.stat().st_size) for p in files] == before
    assert native.ntotal == 48 and searcher.info()[0] == 48

    gone = [chunks[i] for i in (0, 17, 18, 30, 47)]
    assert remove_chunk_ids(cfg, [c.id for c in gone] + ["no-such-chunk"]) == {"bm25": 5, "dense": 5, "colbert": 5}
    left = [c for c in chunks if c.id not in {g.id for g in gone}]

    # (a) the same native handles, shrunk in place; the mtimes this process wrote are the ones it remembers
    assert vs.index is index and vs.index.native is native and native.ntotal == 43 and index.rows_epoch == 1
    assert native.remove_kernel_ms() >= 0.0
    assert col._searcher is searcher and searcher.info()[0] == 43 and searcher.remove_kernel_ms() >= 0.0
    assert vs._index_mtime == files[0].stat().st_mtime and vs._meta_mtime == files[1].stat().st_mtime
    assert col._store_mtime == files[3].stat().st_mtime and col.store_is_current()
    # (b) the files hold consistent rows / pids
    X, _ = artifacts.read_faiss_index(files[0])
    meta = artifacts.read_faiss_meta(files[1])
    assert X.shape[0] == 43 and [c.id for c in meta] == [c.id for c in left] == [c.id for c in vs.chunks]
    assert np.array_equal(X.view(np.uint32), native.read_rows(0, 43).view(np.uint32))
    by_pid = artifacts.read_colbert_meta(files[2])
    assert sorted(by_pid) == list(range(43)) and [by_pid[p].id for p in range(43)] == [c.id for c in left]
    D, ptr = artifacts.read_token_store(col.index_dir())
    rd, rp = searcher.read()
    assert ptr.shape[0] == 44 and np.array_equal(ptr, rp) and np.array_equal(D.view(np.uint32), rd.view(np.uint32))
    assert not [p for p in files[1].parent.iterdir() if p.name.endswith(".tmp")]

    # (c) the withdrawn chunks are gone from every channel; the searches made before run again on the same handles,
    # and no workspace of the process grows: a reload would have made a new handle with workspaces of its own
    growths = _native.workspace_growths()
    seen = set().union(*(channel_hits(q) for q in probes))
    assert not seen & {g.id for g in gone} and seen <= {c.id for c in left}
    assert _native.workspace_growths() == growths
    assert vs.index is index and vs.index.native is native and col._searcher is searcher
    for q in probes:
        assert not {c.id for c, _ in r.bm25.search(q, 10)} & {g.id for g in gone}
    assert r.bm25.gpu_index().info()[0] == 43
    got = r.search_batch(QUESTIONS, top_k=10)
    assert r._native_channels(10) is not None and r.native_engine(with_colbert=True) is not None
    assert vs.index.native is native and col._searcher is searcher

    # (d) against retrievers loaded afresh from the rewritten files (a copy of the directory: other singletons)
    shutil.copytree(tmp_path / "live", tmp_path / "fresh")
    fresh = _cfg(tmp_path / "fresh")
    rw = HybridRetriever(fresh)
    assert rw.dense.store is not vs and rw.colbert is not col
    exp = rw.search_batch(QUESTIONS, top_k=10)
    assert rw.native_engine(with_colbert=True) is not None and rw.dense.store.index.native is not native
    for g, e in zip(got, exp):
        assert len(e) > 0
        assert_hits_equal_mod_ties([dump(h) for h in g], [dump(h) for h in e])
    for q in QUESTIONS + [left[5].text[:200]]:
        a, b = r.search_colbert(q, 10), rw.search_colbert(q, 10)
        assert [(h.chunk.id, h.score) for h in a] == [(h.chunk.id, h.score) for h in b]
        a, b = vs.search(q, 10), rw.dense.store.search(q, 10)
        assert [(c.id, s) for c, s in a] == [(c.id, s) for c, s in b]
    assert rw.colbert._searcher.info()[:2] == searcher.info()[:2]
    assert np.array_equal(np.float32(rw.colbert._searcher.stats()).view(np.uint32), np.float32(searcher.stats()).view(np.uint32))

    # (e) everything a channel holds cannot go: nothing is touched
    before = [(p.stat().st_mtime_ns, p.stat().st_size) for p in files]
    with pytest.raises(ValueError):
        remove_chunk_ids(cfg, [c.id for c in left])
    assert [(p.stat().st_mtime_ns, p.stat().st_size) for p in files] == before
    assert native.ntotal == 43 and searcher.info()[0] == 43

"""An amendment reaches a live HybridRetriever: after builders/replace.py replace_chunks ran, the dense matrix, the BM25
postings and the ColBERT token store resident in HBM hold the amended chunks at their old rows (amdr_dense_replace,
amdr_bm25_replace, amdr_maxsim_replace: the same native handles, nothing reloaded), the files hold the same state, and
the live retriever answers exactly as a retriever freshly built from the amended corpus."""
import json
import shutil
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN
from test_graph_device_gpu import ucc_graph

pytestmark = pytest.mark.gpu

QUESTIONS = ["what warranty does a merchant give that goods are merchantable", "Short Titles",
             "statute of frauds signed writing sale of goods price of $500", "risk of loss passes to the buyer"]
ROWS = (0, 17, 47)  # the first, one inside, the last


def dump(h):
    return {"id": h.chunk.id, "score": float(h.score), "rank": h.rank, "source": h.source, "breakdown": h.score_breakdown,
            "text": h.chunk.text}


def _cfg(root, graph=None):
    from legal_rag_amd.config import AppConfig
    cfg = AppConfig.for_data_dir(str(root), "en")
    cfg.retrieval.encoder_backend = "hashing"
    cfg.retrieval.enable_colbert = True
    cfg.retrieval.enable_rerank = False
    if graph is not None:
        cfg.retrieval.enable_graph = True
        cfg.retrieval.graph_channel = "device"
        cfg.paths.law_graph_jsonl = str(graph)
    return cfg


def _jsonl(path, chunks):
    path.write_text("".join(json.dumps(c.model_dump(), ensure_ascii=False) + "\n" for c in chunks), encoding="utf-8")
    return path


def _build(cfg, chunks, jsonl):
    from legal_rag_amd.retrieval.builders.colbert_builder import build_colbert_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    build_faiss_index(cfg, chunks)
    assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(jsonl, chunks)) == len(chunks)
    build_colbert_index(cfg, chunks)


@pytest.fixture(scope="module")
def corpus():
    """48 chunks, and their amendment: rows 0, 17 and 47 take the wording of articles outside the 48 (their ids, law and
    section stay), so the amended chunks answer other questions than before."""
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    every = load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")
    chunks = every[:48]
    assert len({c.id for c in chunks}) == 48
    new = {r: chunks[r].model_copy(update={"text": every[100 + 7 * j].text + " As amended."}) for j, r in enumerate(ROWS)}
    amended = [new.get(r, c) for r, c in enumerate(chunks)]
    return chunks, amended, new, every


def _assert_same_answers(r, w, questions, scopes=None, decisions=None):
    got = r.search_batch(questions, top_k=10, scopes=scopes, decisions=decisions)
    exp = w.search_batch(questions, top_k=10, scopes=scopes, decisions=decisions)
    for q, g, e in zip(questions, got, exp):
        assert len(e) > 0, q
        assert [dump(h) for h in g] == [dump(h) for h in e], q
    return got


def test_replacement_reaches_a_live_hybrid_retriever(tmp_path, corpus):
    from pathlib import Path

    from legal_rag_amd import _native, artifacts
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    from legal_rag_amd.retrieval.builders.incremental_colbert_builder import IncrementalColBERTBuilder
    from legal_rag_amd.retrieval.builders.incremental_dense_builder import IncrementalDenseBuilder
    from legal_rag_amd.retrieval.builders.replace import replace_chunks
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from legal_rag_amd.retrieval.scope import Scope
    chunks, amended, new, every = corpus
    cfg = _cfg(tmp_path / "live")
    _build(cfg, chunks, tmp_path / "all.jsonl")
    r = HybridRetriever(cfg)
    assert r.colbert is not None and r.colbert.enabled
    probes = QUESTIONS + [new[row].text[:200] for row in ROWS] + [chunks[row].text[:200] for row in ROWS]
    before = r.search_batch(probes, top_k=10)
    assert all(len(h) > 0 for h in before) and r.native_engine(with_colbert=True) is not None
    vs, col, bm = r.dense.store, r.colbert, r.bm25
    index, native, searcher, bm_model, bm_native = vs.index, vs.index.native, col._searcher, bm.bm25, bm.gpu_index()
    files = [Path(cfg.retrieval.faiss_index_file), Path(cfg.retrieval.faiss_meta_file), Path(cfg.retrieval.colbert_meta_file),
             col.index_dir() / "amdr_tokens.npz", Path(cfg.retrieval.bm25_index_file)]

    # ids nobody holds: 0 everywhere, no file touched
    stamp = [(p.stat().st_mtime_ns, p.stat().st_size) for p in files]
    assert replace_chunks(cfg, _jsonl(tmp_path / "none.jsonl", every[60:62])) == {"bm25": 0, "dense": 0, "colbert": 0}
    assert [(p.stat().st_mtime_ns, p.stat().st_size) for p in files] == stamp

    # the amendment, with a chunk the indexes do not hold (left alone) and an earlier version of row 17 (the later counts)
    incoming = [new[47], every[50], new[17].model_copy(update={"text": "superseded"}), new[0], new[17]]
    assert replace_chunks(cfg, _jsonl(tmp_path / "amend.jsonl", incoming)) == {"bm25": 3, "dense": 3, "colbert": 3}

    # (a) the same native handles, edited in place; every chunk keeps its row; the mtimes written are the ones remembered
    assert vs.index is index and vs.index.native is native and native.ntotal == 48 and index.rows_epoch == 1
    assert native.replace_kernel_ms() >= 0.0
    assert col._searcher is searcher and searcher.info()[0] == 48 and searcher.replace_kernel_ms() >= 0.0
    assert bm.bm25 is bm_model and bm.gpu_index() is bm_native and bm_native.replaces() == 1 and bm_native.info()[0] == 48
    assert bm_native.replace_kernel_ms() >= 0.0 and bm.state_is_current()
    assert vs._index_mtime == files[0].stat().st_mtime and vs._meta_mtime == files[1].stat().st_mtime
    assert col._store_mtime == files[3].stat().st_mtime and col.store_is_current()
    want = [(c.id, c.text) for c in amended]
    assert [(c.id, c.text) for c in vs.chunks] == want and [(c.id, c.text) for c in bm.chunks] == want
    assert [(col._pid2chunk[p].id, col._pid2chunk[p].text) for p in range(48)] == want
    # (b) the files hold the resident state
    X, _ = artifacts.read_faiss_index(files[0])
    assert [(c.id, c.text) for c in artifacts.read_faiss_meta(files[1])] == want
    assert X.shape[0] == 48 and np.array_equal(X.view(np.uint32), native.read_rows(0, 48).view(np.uint32))
    by_pid = artifacts.read_colbert_meta(files[2])
    assert sorted(by_pid) == list(range(48)) and [(by_pid[p].id, by_pid[p].text) for p in range(48)] == want
    D, ptr = artifacts.read_token_store(col.index_dir())
    rd, rp = searcher.read()
    assert ptr.shape[0] == 49 and np.array_equal(ptr, rp) and np.array_equal(D.view(np.uint32), rd.view(np.uint32))
    assert [(c.id, c.text) for c in artifacts.read_bm25_pickle(files[4])[1]] == want
    assert not [p for p in files[1].parent.iterdir() if p.name.endswith(".tmp")]

    # (c) against a retriever freshly built from the amended corpus, in its original order: exactly its answers
    fresh = _cfg(tmp_path / "fresh")
    _build(fresh, amended, tmp_path / "amended.jsonl")
    w = HybridRetriever(fresh)
    assert w.dense.store is not vs and w.colbert is not col and w.bm25 is not bm
    got = _assert_same_answers(r, w, probes)
    assert r.native_engine(with_colbert=True) is not None and vs.index.native is native and col._searcher is searcher
    assert [[dump(h) for h in g] for g in got] != [[dump(h) for h in b] for b in before]  # and they did change
    for row in ROWS:  # an amended chunk is found by its new wording, at its old id
        hits = r.search(new[row].text[:200], top_k=10)
        assert [dump(h) for h in hits] == [dump(h) for h in w.search(new[row].text[:200], top_k=10)]
        assert any(h.chunk.id == chunks[row].id and h.chunk.text == new[row].text for h in hits)
    sections = sorted({c.section for c in chunks if c.section})
    scopes = [Scope(section=chunks[0].section), None, Scope(section=chunks[17].section), Scope(section=sections[-1])]
    _assert_same_answers(r, w, QUESTIONS, scopes=scopes)
    for q, s in zip(QUESTIONS, scopes):
        assert [dump(h) for h in r.search(q, top_k=10, scope=s)] == [dump(h) for h in w.search(q, top_k=10, scope=s)]
    for q in probes:
        a, b = r.search_colbert(q, 10), w.search_colbert(q, 10)
        assert [(h.chunk.id, h.score) for h in a] == [(h.chunk.id, h.score) for h in b]
        a, b = vs.search(q, 10), w.dense.store.search(q, 10)
        assert [(c.id, s) for c, s in a] == [(c.id, s) for c, s in b]
        a, b = bm.search(q, 10), w.bm25.search(q, 10)
        assert [(c.id, s) for c, s in a] == [(c.id, s) for c, s in b]
    assert w.colbert._searcher.info()[:2] == searcher.info()[:2]
    assert np.array_equal(np.float32(w.colbert._searcher.stats()).view(np.uint32), np.float32(searcher.stats()).view(np.uint32))
    for x, y in zip(bm_native.read(), w.bm25.gpu_index().read()):
        assert x.tobytes() == y.tobytes()

    # (d) the files on disk load to the same state in a new retriever object (a copy of the directory: other singletons)
    shutil.copytree(tmp_path / "live", tmp_path / "reloaded")
    rw = HybridRetriever(_cfg(tmp_path / "reloaded"))
    assert rw.dense.store is not vs and rw.colbert is not col
    _assert_same_answers(r, rw, probes)
    _assert_same_answers(r, rw, QUESTIONS, scopes=scopes)

    # (e) add_jsonl of the amended chunks still adds nothing
    known = _jsonl(tmp_path / "known.jsonl", [new[row] for row in ROWS])
    stamp = [(p.stat().st_mtime_ns, p.stat().st_size) for p in files]
    assert IncrementalBM25Builder(cfg).add_jsonl(known) == 0 and IncrementalDenseBuilder(cfg).add_jsonl(known) == 0
    assert IncrementalColBERTBuilder(cfg).add_jsonl(known) == 0
    assert [(p.stat().st_mtime_ns, p.stat().st_size) for p in files] == stamp
    assert native.ntotal == 48 and searcher.info()[0] == 48 and bm_native.info()[0] == 48


def test_replacement_with_the_graph_channel_on_the_device_and_a_scope(tmp_path, corpus):
    """graph_channel="device": the graph stage holds row norms and device tables of the dense rows; after the replacement
    (FlatIPIndex.rows_epoch) they are bound again, and the graph-augmented answers are the freshly built retriever's."""
    from legal_rag_amd.retrieval.builders.replace import replace_chunks
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from legal_rag_amd.retrieval.scope import Scope
    chunks, amended, new, every = corpus
    gpath = tmp_path / "graph.jsonl"
    ucc_graph(chunks, gpath)
    cfg = _cfg(tmp_path / "live", graph=gpath)
    _build(cfg, chunks, tmp_path / "all.jsonl")
    r = HybridRetriever(cfg)
    assert r.graph is not None and r.colbert is not None and r.colbert.enabled
    qs = QUESTIONS + [new[row].text[:200] for row in ROWS] + [chunks[5].text[:150]]
    decisions = [SimpleNamespace(mode="GRAPH_AUGMENTED" if i % 2 == 0 else "HYBRID") for i in range(len(qs))]
    before = r.search_batch(qs, top_k=10, decisions=decisions)  # binds the graph stage to the old rows
    assert any(h.score_breakdown.get("channel") == ["graph"] for hits in before for h in hits)
    native = r.dense.store.index.native
    assert replace_chunks(cfg, _jsonl(tmp_path / "amend.jsonl", [new[row] for row in ROWS])) == {"bm25": 3, "dense": 3, "colbert": 3}
    assert r.dense.store.index.native is native and r.dense.store.index.rows_epoch == 1
    fresh = _cfg(tmp_path / "fresh", graph=gpath)
    _build(fresh, amended, tmp_path / "amended.jsonl")
    w = HybridRetriever(fresh)
    got = _assert_same_answers(r, w, qs, decisions=decisions)
    assert any(h.score_breakdown.get("channel") == ["graph"] for hits in got for h in hits)
    hybrid = [SimpleNamespace(mode="HYBRID")] * len(QUESTIONS)
    scopes = [Scope(section=chunks[0].section), Scope(section=chunks[47].section), None, Scope(section=chunks[17].section)]
    _assert_same_answers(r, w, QUESTIONS, scopes=scopes, decisions=hybrid)

"""Ingest into a live HybridRetriever, BM25 side: after IncrementalBM25Builder ran, the retriever's resident postings
were appended to in HBM (amdr_bm25_add) — the same native handle, now over all documents — the batch stage is still the
device-resident one, and every hit equals that of a retriever loaded from the rewritten files."""
import json

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
    cfg.retrieval.enable_colbert = False
    cfg.retrieval.enable_rerank = False
    return cfg


def _jsonl(path, chunks):
    path.write_text("".join(json.dumps(c.model_dump(), ensure_ascii=False) + "\n" for c in chunks), encoding="utf-8")
    return path


def test_bm25_ingest_appends_to_the_resident_postings(tmp_path):
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    from legal_rag_amd.retrieval.builders.incremental_dense_builder import IncrementalDenseBuilder
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    chunks = load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")[:95]
    cfg = _cfg(tmp_path / "live")
    build_faiss_index(cfg, chunks[:60])
    # through the incremental builder, from nothing, so that the old tokens are the ones a later add re-fits with
    assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "first.jsonl", chunks[:60])) == 60
    r = HybridRetriever(cfg)
    assert all(len(h) > 0 for h in r.search_batch(QUESTIONS, top_k=10))
    assert r.native_engine() is not None
    handle, model = r.bm25.gpu_index(), r.bm25.bm25
    assert handle.info()[0] == 60 and handle.info()[3] == 0
    target = chunks[89]
    assert all(c.id != target.id for c, _ in r.bm25.search(target.text[:200], 5))

    inc = _jsonl(tmp_path / "incoming.jsonl", chunks[60:95])
    assert IncrementalDenseBuilder(cfg).add_jsonl(inc) == 35
    assert IncrementalBM25Builder(cfg).add_jsonl(inc) == 35
    got_one = [r.search(q, top_k=10) for q in QUESTIONS]
    got = r.search_batch(QUESTIONS, top_k=10)
    # the same native handle and host object, grown in place
    assert r.bm25.bm25 is model and r.bm25.gpu_index() is handle and r.bm25.appends == 1
    assert handle.info()[0] == 95 and handle.info()[3] == 1 and len(r.bm25.chunks) == 95
    assert r.bm25.search(target.text[:200], 3)[0][0].id == target.id
    # still the device-resident stage
    assert r._native_channels(10) is not None and r.native_engine() is not None

    rw = HybridRetriever(cfg)  # loads the rewritten files
    exp = rw.search_batch(QUESTIONS, top_k=10)
    assert rw.bm25.bm25 is not model and rw.bm25.gpu_index().info()[:4] == (95, handle.info()[1], handle.info()[2], 0)
    exp_one = [rw.search(q, top_k=10) for q in QUESTIONS]
    for g, e in list(zip(got, exp)) + list(zip(got_one, exp_one)):
        assert len(e) > 0
        assert_hits_equal_mod_ties([dump(h) for h in g], [dump(h) for h in e])
    for a, b in zip(handle.read(), rw.bm25.gpu_index().read()):
        assert a.tobytes() == b.tobytes()

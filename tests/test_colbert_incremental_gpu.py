"""Ingest into a live HybridRetriever: after the three incremental builders ran, the ColBERT channel finds the new
documents without a restart (the resident token store was appended to in HBM, amdr_maxsim_add), the batch stage is
still the device-resident one, and every hit equals that of a retriever over indexes built from the whole list; a
token store rewritten by another process is reloaded."""
import json

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


def test_ingest_reaches_a_live_hybrid_retriever(tmp_path):
    from legal_rag_amd import artifacts
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.colbert_builder import build_colbert_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    from legal_rag_amd.retrieval.builders.incremental_colbert_builder import IncrementalColBERTBuilder
    from legal_rag_amd.retrieval.builders.incremental_dense_builder import IncrementalDenseBuilder
    from legal_rag_amd.retrieval.colbert_retriever import get_token_encoder
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    chunks = load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")[:95]
    cfg = _cfg(tmp_path / "live")
    build_faiss_index(cfg, chunks[:60])
    build_bm25_index(cfg, chunks[:60])
    build_colbert_index(cfg, chunks[:60])
    r = HybridRetriever(cfg)
    assert r.colbert is not None and r.colbert.enabled
    assert all(len(h) > 0 for h in r.search_batch(QUESTIONS, top_k=10))
    assert r.native_engine(with_colbert=True) is not None
    target = chunks[89]
    assert all(h.chunk.id != target.id for h in r.search_colbert(target.text[:200], 5))
    searcher = r.colbert._searcher
    assert searcher.info()[0] == 60

    inc = _jsonl(tmp_path / "incoming.jsonl", chunks[55:90])  # 5 ids are there already
    assert IncrementalDenseBuilder(cfg).add_jsonl(inc) == 30
    assert IncrementalBM25Builder(cfg).add_jsonl(inc) == 30
    assert IncrementalColBERTBuilder(cfg).add_jsonl(inc) == 30
    # (a) the channel finds a new document; the resident store was appended to, not reloaded
    assert r.search_colbert(target.text[:200], 3)[0].chunk.id == target.id
    assert r.colbert._searcher is searcher and searcher.info()[0] == 90 and searcher.info()[5] == 1
    # (b) still the device-resident stage
    got = r.search_batch(QUESTIONS, top_k=10)
    assert r._native_channels(10) is not None and r.native_engine(with_colbert=True) is not None
    assert r.colbert._searcher is searcher
    # (c) against indexes built from the whole list in another directory.  (BM25 there through the incremental builder
    # too, from nothing: it tokenises English as the reference's incremental path does, build_bm25_index with a regex —
    # the two fits differ by design, incremental_bm25_builder.py.)
    whole = _cfg(tmp_path / "whole")
    build_faiss_index(whole, chunks[:90])
    assert IncrementalBM25Builder(whole).add_jsonl(_jsonl(tmp_path / "all.jsonl", chunks[:90])) == 90
    build_colbert_index(whole, chunks[:90])
    rw = HybridRetriever(whole)
    exp = rw.search_batch(QUESTIONS, top_k=10)
    assert rw.native_engine(with_colbert=True) is not None
    for g, e in zip(got, exp):
        assert len(e) > 0
        assert_hits_equal_mod_ties([dump(h) for h in g], [dump(h) for h in e])
    for q in QUESTIONS:
        a, b = r.search_colbert(q, 10), rw.search_colbert(q, 10)
        assert [(h.chunk.id, h.score) for h in a] == [(h.chunk.id, h.score) for h in b]

    # (d) another process appends: the files change behind the retriever's back and the next search reloads the store
    extra = chunks[90:95]
    enc = get_token_encoder(cfg.retrieval.colbert_model_name, "hashing", int(cfg.retrieval.colbert_doc_maxlen),
                            device="cuda:0")
    mats = [np.asarray(enc.encode_doc(c.text.strip()), dtype=np.float32) for c in extra]
    with open(cfg.retrieval.colbert_meta_file, "a", encoding="utf-8") as f:
        f.writelines(json.dumps({"pid": 90 + i, "chunk": c.model_dump()}, ensure_ascii=False) + "\n"
                     for i, c in enumerate(extra))
    artifacts.append_token_store(r.colbert.index_dir(), np.concatenate(mats),
                                 np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]))
    assert r.search_colbert(extra[-1].text[:200], 3)[0].chunk.id == extra[-1].id
    assert r.colbert._searcher is not searcher and r.colbert._searcher.info()[0] == 95

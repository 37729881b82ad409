"""Phrase constraints through the public interface, on the UCC-en fixture (tests/golden/corpus/law_en.jsonl, 591 articles,
the BM25 index cut by the English index rule): search(q, terms=Terms(all_of=[Phrase(...)])) equals
search(q, scope=Scope(chunk_ids=ids)) with `ids` computed on the host by a window scan of each chunk's tokens, hit for hit,
with tolerance 0; every returned chunk's text holds the phrase; the row counts are not the conjunction's; and a live
replacement that takes the phrase out of a chunk takes the chunk out of the results."""
import numpy as np
import pytest

from conftest import GOLDEN
from helpers import assert_hits_equal_mod_ties
from test_replace_api_gpu import _build, _cfg, _jsonl

pytestmark = pytest.mark.gpu

QUESTIONS = ["what rights does a secured party have after default", "Short Titles",
             "statute of frauds signed writing sale of goods price of $500"]
TOP_K = 20


def dump(h):
    return {"id": h.chunk.id, "score": float(h.score), "rank": h.rank, "source": h.source, "breakdown": h.score_breakdown}


def same(got, exp):
    assert_hits_equal_mod_ties([dump(h) for h in got], [dump(h) for h in exp], float_tol=0.0)


def ucc_chunks():
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    seen, chunks = set(), []
    for c in load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl"):  # (592 lines, one id twice: the first is kept)
        if c.id not in seen:
            seen.add(c.id)
            chunks.append(c)
    assert len(chunks) == 591
    return chunks


@pytest.fixture(scope="module")
def live(tmp_path_factory):
    """The whole fixture behind a live HybridRetriever (stand-in encoders, ColBERT included; min_final_score below every
    fused score).  The BM25 index is the batch builder's: English text cut by the index rule on lower-cased text."""
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.colbert_builder import build_colbert_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    root = tmp_path_factory.mktemp("phrase_api")
    chunks = ucc_chunks()
    cfg = _cfg(root / "live")
    cfg.retrieval.min_final_score = -1.0
    build_faiss_index(cfg, chunks)
    build_bm25_index(cfg, chunks)
    build_colbert_index(cfg, chunks)
    r = HybridRetriever(cfg)
    assert r.colbert is not None and r.colbert.enabled
    r.bm25.load()
    assert r.bm25.index_tokenizer == "en_regex"
    return cfg, r


def sequences(r):
    """[(chunk, its token sequence)]: the chunk texts cut again by the index's own document rule."""
    return [(c, r.bm25.document_tokens(c.text)) for c in r.bm25.chunks]


def ids_of(r, terms):
    return [c.id for c, seq in sequences(r) if terms.matches(seq)]


def phrases():
    from legal_rag_amd.retrieval.terms import Phrase
    return (Phrase("security", "interest"), Phrase("from", "time", "to", "time"), Phrase("interest", "security"),
            Phrase("holder", "in", "due", "course"))


def test_search_with_a_phrase_equals_the_explicit_scope_and_every_hit_holds_it(live):
    from legal_rag_amd.retrieval.scope import Scope
    from legal_rag_amd.retrieval.terms import Terms
    cfg, r = live
    si, fttt, rev, hidc = phrases()
    assert r.phrase("Security Interest") == si and r.phrase("from time to time") == fttt
    seqs = {c.id: seq for c, seq in sequences(r)}
    # the counts of the issue's table: the conjunction and the phrase differ
    counts = {p: (len(ids_of(r, Terms(all_of=[p.tokens]))), len(ids_of(r, Terms(all_of=[p])))) for p in (si, fttt, rev, hidc)}
    assert counts == {si: (135, 121), fttt: (99, 2), rev: (135, 0), hidc: (23, 21)}
    assert not r.bm25.gpu_index().tokens_info()[0]  # the stream is made on the first phrase
    for q in QUESTIONS:
        for p in (si, fttt, hidc):
            t = Terms(all_of=[p])
            ids = ids_of(r, t)
            got = r.search(q, top_k=TOP_K, terms=t)
            same(got, r.search(q, top_k=TOP_K, scope=Scope(chunk_ids=ids)))
            assert len(got) == min(TOP_K, len(ids)) and all(p.within(seqs[h.chunk.id]) for h in got)
            assert all(" ".join(p.tokens) in " ".join(r.bm25.document_tokens(h.chunk.text)) for h in got)
            assert [h.rank for h in got] == list(range(1, len(got) + 1))
        assert r.search(q, top_k=TOP_K, terms=Terms(all_of=[rev])) == []
        # the conjunction ranks other rows
        conj = r.search(q, top_k=200, terms=Terms(all_of=[si.tokens]))
        assert len(conj) == 135 and len(r.search(q, top_k=200, terms=Terms(all_of=[si]))) == 121
    info = r.bm25.gpu_index().tokens_info()
    assert info == (True, sum(len(s) for s in seqs.values())) and info[1] == 148_101
    # excluded, and beside plain tokens
    for t in (Terms(none_of=[si]), Terms(all_of=["debtor", ("collateral", si)], none_of=[fttt]), Terms(any_of=[fttt, hidc])):
        ids = ids_of(r, t)
        assert 0 < len(ids) < 591
        got = r.search(QUESTIONS[0], top_k=TOP_K, terms=t)
        same(got, r.search(QUESTIONS[0], top_k=TOP_K, scope=Scope(chunk_ids=ids)))
        assert all(t.matches(seqs[h.chunk.id]) for h in got) and len(got) == min(TOP_K, len(ids))
    assert len(ids_of(r, Terms(none_of=[si]))) == 591 - 121


def test_batches_and_the_columnar_form_agree_and_the_per_channel_searches_take_phrases(live):
    from legal_rag_amd.retrieval.scope import Scope
    from legal_rag_amd.retrieval.terms import Terms
    cfg, r = live
    si, fttt, rev, hidc = phrases()
    sec = next(c.section for c, seq in sequences(r) if c.section and si.within(seq))
    terms = [None, Terms(all_of=[si]), Terms(all_of=[fttt]), Terms(all_of=[rev]), Terms(none_of=[si]), Terms(all_of=[si]),
             Terms(all_of=["goods"])]
    scopes = [None, None, None, None, None, Scope(section=sec), None]
    qs = [QUESTIONS[j % len(QUESTIONS)] for j in range(len(terms))]
    out = r.search_batch(qs, top_k=TOP_K, terms=terms, scopes=scopes)
    for j, hits in enumerate(out):
        same(hits, r.search(qs[j], top_k=TOP_K, terms=terms[j], scope=scopes[j]))
    assert out[3] == [] and all(out[j] for j in (0, 1, 2, 4, 5, 6)) and len(out[2]) == 2
    assert all(h.chunk.section == sec for h in out[5])
    same(out[1], r.search(qs[1], top_k=TOP_K, scope=Scope(chunk_ids=ids_of(r, terms[1]))))
    for values in (True, False):
        arr = r.search_batch_arrays(qs, top_k=TOP_K, terms=terms, scopes=scopes, values=values)
        for j, hits in enumerate(out):
            assert arr["count"][j] == len(hits)
            assert arr["scores"][j, :len(hits)].tolist() == [h.score for h in hits]
            assert sorted(arr["chunks"][int(x)].id for x in arr["rows"][j, :len(hits)]) == sorted(h.chunk.id for h in hits)
            assert np.all(arr["rows"][j, len(hits):] == -1)
    t = Terms(all_of=[hidc])
    ids = ids_of(r, t)
    for fn in (r.search_dense, r.search_bm25, r.search_colbert):
        got = fn(QUESTIONS[0], TOP_K, terms=t)
        same(got, fn(QUESTIONS[0], TOP_K, scope=Scope(chunk_ids=ids)))
        assert len(got) == min(TOP_K, len(ids))
        assert fn(QUESTIONS[0], TOP_K, terms=Terms(all_of=[rev])) == []


def test_a_status_word_raises_and_names_the_phrase(live, monkeypatch):
    from legal_rag_amd.retrieval import hybrid_retriever as HR
    from legal_rag_amd.retrieval.terms import Terms
    cfg, r = live
    si, fttt, _, _ = phrases()
    pack = HR._pack_terms

    def short(*a, **k):
        tt = pack(*a, **k)
        tt.phr_cand_max = min(tt.phr_ops[1].size, 3)  # far below the phrases' drivers: their status words are 1
        return tt
    monkeypatch.setattr(HR, "_pack_terms", short)
    with pytest.raises(RuntimeError, match=r"Phrase\('from', 'time', 'to', 'time'\) of the batch overflowed"):
        r.search_batch([QUESTIONS[0]] * 2, top_k=TOP_K, terms=[Terms(all_of=[fttt]), Terms(all_of=[si])])
    with pytest.raises(RuntimeError, match=r"Phrase\('security', 'interest'\) overflowed"):
        r.search_bm25(QUESTIONS[0], TOP_K, terms=Terms(all_of=[si]))


def test_a_live_replacement_that_takes_the_phrase_out_of_a_chunk_takes_the_chunk_out_of_the_results(tmp_path):
    """An index of its own, built by the incremental builder: the one a live replace_jsonl edits in place (it records that
    builder's segmenter, and `retriever.phrase` cuts the phrase with it)."""
    from legal_rag_amd.retrieval.builders.replace import replace_chunks
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from legal_rag_amd.retrieval.scope import Scope
    from legal_rag_amd.retrieval.terms import Terms
    chunks = [c for c in ucc_chunks() if "security interest" in c.text][:40] + ucc_chunks()[:24]
    chunks = list({c.id: c for c in chunks}.values())
    cfg = _cfg(tmp_path / "live")
    cfg.retrieval.min_final_score = -1.0
    _build(cfg, chunks, tmp_path / "all.jsonl")
    r = HybridRetriever(cfg)
    p = r.phrase("security interest")
    assert len(p) >= 2 and p.tokens[0] == "security" and p.tokens[-1] == "interest"
    t = Terms(all_of=[p])
    q = QUESTIONS[0]
    before = r.search(q, top_k=TOP_K, terms=t)
    ids = ids_of(r, t)
    assert len(before) == TOP_K and 30 <= len(ids) < len(chunks)
    same(before, r.search(q, top_k=TOP_K, scope=Scope(chunk_ids=ids)))
    native = r.bm25.gpu_index()
    assert native.tokens_info()[0]
    victim = before[0].chunk
    amended = victim.model_copy(update={"text": victim.text.replace("security interest", "interest in the security")})
    assert "security interest" not in amended.text and "security" in amended.text
    assert replace_chunks(cfg, _jsonl(tmp_path / "amend.jsonl", [amended])) == {"bm25": 1, "dense": 1, "colbert": 1}
    assert r.bm25.gpu_index() is native and native.replaces() == 1 and not native.tokens_info()[0]  # dropped by the update
    after = r.search(q, top_k=TOP_K, terms=t)
    assert native.tokens_info()[0]  # made again on the next phrase
    ids_after = ids_of(r, t)
    assert victim.id not in ids_after and len(ids_after) == len(ids) - 1
    assert victim.id not in [h.chunk.id for h in after] and len(after) == TOP_K
    same(after, r.search(q, top_k=TOP_K, scope=Scope(chunk_ids=ids_after)))
    # the conjunction still names the chunk: its words are all there
    assert victim.id in [c.id for c, seq in sequences(r) if set(p.tokens) <= set(seq)]

"""Highlighting through the public interface, on a subset of the UCC-en fixture (tests/golden/corpus/law_en.jsonl) behind a
live HybridRetriever: search(..., highlight=Highlight()) marks the phrase of a Terms in every hit and the snippet shows
it; a PhraseOf with a Prefix marks the tokens with the stem; highlight=None returns what the call returns without the
argument; after a live replacement under cfg.retrieval.token_stream = "carry" the amended chunk is highlighted from its
new text, without the host cutting the corpus again."""
import pytest

from test_tok_carry_api_gpu import QUESTION, _build, _cfg, _jsonl, ucc  # noqa: F401 - `ucc` is the fixture

pytestmark = pytest.mark.gpu

TOP_K = 10


@pytest.fixture(scope="module")
def live(tmp_path_factory, ucc):  # noqa: F811
    """The subset behind a live HybridRetriever whose BM25 index is cut by the English index rule (lower-cased words)."""
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.colbert_builder import build_colbert_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    root = tmp_path_factory.mktemp("highlight_api")
    chunks, _ = ucc
    cfg = _cfg(root / "live")
    build_faiss_index(cfg, chunks)
    build_bm25_index(cfg, chunks)
    build_colbert_index(cfg, chunks)
    r = HybridRetriever(cfg)
    r.bm25.load()
    assert r.bm25.index_tokenizer == "en_regex"
    return cfg, r, root


def check_marks(hit):
    hl = hit.score_breakdown["highlight"]
    text = hit.chunk.text
    assert hl is not None and hl["snippet"] == text[hl["window_chars"][0]:hl["window_chars"][1]]
    for m in hl["marks"]:
        assert hl["window_tokens"][0] <= m["token"] < hl["window_tokens"][1]
        assert hl["window_chars"][0] <= m["char_start"] < m["char_end"] <= hl["window_chars"][1]
    return hl


def test_a_phrase_is_marked_in_every_hit_and_shown_in_the_snippet(live):
    from legal_rag_amd.retrieval.highlight import Highlight
    from legal_rag_amd.retrieval.terms import Phrase, Terms
    cfg, r, _ = live
    t = Terms(all_of=[Phrase("security", "interest")])
    hits = r.search(QUESTION, top_k=TOP_K, terms=t, highlight=Highlight(question=False))
    assert len(hits) >= 1
    most = 0
    for h in hits:
        hl = check_marks(h)
        assert "security interest" in hl["snippet"].lower()
        toks = r.bm25.document_tokens(h.chunk.text)
        for m in hl["marks"]:
            assert h.chunk.text[m["char_start"]:m["char_end"]].lower() == toks[m["token"]] == m["label"]  # slices to its token
        assert {m["label"] for m in hl["marks"]} == {"security", "interest"} and hl["found"] == ["security", "interest"]
        assert hl["missing"] == [] and hl["n_marks_in_chunk"] >= len(hl["marks"]) >= 2 and not hl["truncated"]
        # phrase-only slots: every marked "security" is followed by a marked "interest"
        at = {m["token"]: m["label"] for m in hl["marks"]}
        assert all(at.get(p + 1) == "interest" for p, lab in at.items() if lab == "security")
        assert hl["window_tokens"][1] - hl["window_tokens"][0] <= 48 and hl["score"] > 0.0
        most = max(most, len(hl["marks"]))
    assert most >= 2
    # the question's own words beside the phrase's: more labels, the phrase still found
    both = r.search(QUESTION, top_k=TOP_K, terms=t, highlight=Highlight())
    assert [h.chunk.id for h in both] == [h.chunk.id for h in hits]
    labels = {m["label"] for h in both for m in check_marks(h)["marks"]}
    assert labels <= set(r.bm25.document_tokens(QUESTION)) | {"security", "interest"} and labels - {"security", "interest"}
    assert all({"security", "interest"} <= set(h.score_breakdown["highlight"]["found"]) for h in both)
    # the batch form and the method give the same highlights
    batch = r.search_batch([QUESTION], top_k=TOP_K, terms=[t], highlight=Highlight())[0]
    assert [h.score_breakdown["highlight"] for h in batch] == [h.score_breakdown["highlight"] for h in both]
    direct = r.highlight(QUESTION, both, terms=t)
    assert [d.as_dict() for d in direct] == [h.score_breakdown["highlight"] for h in both]


def test_a_phraseof_with_a_prefix_marks_a_token_with_the_stem(live):
    from legal_rag_amd.retrieval.highlight import Highlight
    from legal_rag_amd.retrieval.terms import PhraseOf, Prefix, Terms
    cfg, r, _ = live
    t = Terms(all_of=[PhraseOf(Prefix("secur"), "interest")])
    hits = r.search(QUESTION, top_k=TOP_K, terms=t, highlight=Highlight(question=False))
    assert len(hits) >= 1
    stems = set()
    for h in hits:
        hl = check_marks(h)
        for m in hl["marks"]:
            word = h.chunk.text[m["char_start"]:m["char_end"]].lower()
            assert m["label"] in ("secur!", "interest") and (word.startswith("secur") if m["label"] == "secur!" else word == "interest")
            stems.add(word)
        assert any(m["label"] == "secur!" for m in hl["marks"])
    assert "security" in stems


def test_highlight_none_changes_nothing(live):
    from legal_rag_amd.retrieval.highlight import Highlight
    from legal_rag_amd.retrieval.terms import Phrase, Terms
    cfg, r, _ = live
    for kw in ({}, {"terms": Terms(all_of=[Phrase("security", "interest")])}):
        plain = r.search(QUESTION, top_k=TOP_K, **kw)
        none = r.search(QUESTION, top_k=TOP_K, highlight=None, **kw)
        assert [h.chunk.id for h in none] == [h.chunk.id for h in plain]
        assert [h.score for h in none] == [h.score for h in plain] and [str(h) for h in none] == [str(h) for h in plain]
        assert all("highlight" not in h.score_breakdown for h in none)
        marked = r.search(QUESTION, top_k=TOP_K, highlight=Highlight(), **kw)  # the ranking is the same with it
        assert [(h.chunk.id, h.score) for h in marked] == [(h.chunk.id, h.score) for h in plain]
        assert all(h.score_breakdown["highlight"] is not None for h in marked)
    # a hit whose chunk the BM25 index does not hold gets None; refusals
    from types import SimpleNamespace
    stranger = SimpleNamespace(chunk=SimpleNamespace(id="no-such-chunk", text="security interest"))
    assert r.highlight(QUESTION, [stranger, plain[0]])[0] is None and r.highlight(QUESTION, [stranger, plain[0]])[1] is not None
    with pytest.raises(TypeError):
        r.search(QUESTION, top_k=TOP_K, highlight={"window": 5})
    r.bm25.shard = SimpleNamespace()
    try:
        with pytest.raises(ValueError, match="row-sharded"):
            r.highlight(QUESTION, plain)
    finally:
        r.bm25.shard = None


def test_after_a_live_replacement_the_amended_chunk_is_highlighted_from_its_new_text(tmp_path, ucc, monkeypatch):  # noqa: F811
    """An index the incremental builder made (its tokeniser keeps case and cuts blanks and punctuation as tokens of their
    own) under token_stream = "carry": the replacement carries the stream, and the highlight reads the new text from it."""
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.retrieval.builders.replace import replace_chunks
    from legal_rag_amd.retrieval.highlight import Highlight
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from legal_rag_amd.retrieval.scope import Scope
    from legal_rag_amd.retrieval.terms import Terms
    chunks, _ = ucc
    cfg = _cfg(tmp_path / "live", token_stream="carry")
    _build(cfg, chunks, tmp_path / "all.jsonl")
    r = HybridRetriever(cfg)
    p = r.phrase("security interest")
    t = Terms(all_of=[p])
    spec = Highlight(question=False)
    before = r.search(QUESTION, top_k=TOP_K, terms=t, highlight=spec)
    victim = before[0].chunk
    hl0 = before[0].score_breakdown["highlight"]
    assert hl0["n_marks_in_chunk"] >= len(p) and "security interest" in hl0["snippet"]
    assert [victim.text[m["char_start"]:m["char_end"]] for m in hl0["marks"][:len(p)]] == list(p.tokens)
    amended = victim.model_copy(update={"text": "zebra crossing. " + victim.text.replace("security interest", "interest in the security")})
    assert "security interest" not in amended.text
    native = r.bm25.gpu_index()
    assert replace_chunks(cfg, _jsonl(tmp_path / "amend.jsonl", [amended])) == {"bm25": 1, "dense": 1, "colbert": 1}
    assert r.bm25.gpu_index() is native and native.tokens_info()[0]  # kept by the update

    def no_rebuild(self, docs):
        raise AssertionError("the host cut the corpus again: BM25Okapi.token_stream was called")
    monkeypatch.setattr(BM25Okapi, "token_stream", no_rebuild)
    hit = r.search(QUESTION, top_k=1, scope=Scope(chunk_ids=[victim.id]))[0]
    assert hit.chunk.id == victim.id
    hl = r.highlight(QUESTION, [hit], terms=t, spec=spec)[0]
    assert hl.n_marks_in_chunk == 0 and hl.marks == [] and hl.found == [] and hl.missing == list(p.tokens)
    assert hl.snippet == amended.text[hl.window_chars[0]:hl.window_chars[1]] and hl.snippet.startswith("zebra crossing")
    loose = r.highlight("zebra security", [hit], spec=Highlight(window=8))[0]  # the new text's own word, from the carried stream
    assert loose.marks[0].label == "zebra" and loose.marks[0].token == 0
    assert amended.text[loose.marks[0].char_start:loose.marks[0].char_end] == "zebra"
    assert loose.n_marks_in_chunk == 1 + r.bm25.document_tokens(amended.text).count("security")
    assert " " not in loose.found + loose.missing  # a question token without a letter or a digit is no query word

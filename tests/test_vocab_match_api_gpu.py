"""Wildcard and Fuzzy through the public interface, on the UCC-en fixture (tests/golden/corpus/law_en.jsonl): for a handful
of patterns the hits of search(terms=) and search_bm25(terms=), count, facets and the marks of highlight equal those of the
OneOf of the tokens the plain evaluator (tests/vocab_match_cases.py) picks from the index's own vocabulary, and the rows
equal `Terms.matches` over every chunk's tokens — a pattern with no match, one with a single match, one inside a PhraseOf,
one inside a NearOf and one under none_of among them; suggest on a misspelling; a live ingest of a chunk holding a new token
within one edit of an old one, seen by the next Fuzzy and suggest and gone after its removal, under token_stream = "carry"
as under the default; and the refusals before any launch."""
from types import SimpleNamespace

import pytest

import vocab_match_cases as VC
from test_facets_api_gpu import corpus, retriever
from test_phrase_api_gpu import QUESTIONS, TOP_K, same, ucc_chunks
from test_tok_carry_api_gpu import _jsonl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def live(tmp_path_factory):
    """The whole fixture behind a live HybridRetriever with a dense and a BM25 index."""
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from test_replace_api_gpu import _cfg
    chunks = ucc_chunks()
    cfg = _cfg(tmp_path_factory.mktemp("vocab_match_api") / "live")
    cfg.retrieval.enable_colbert = False
    cfg.retrieval.min_final_score = -1.0
    build_faiss_index(cfg, chunks)
    build_bm25_index(cfg, chunks)
    r = HybridRetriever(cfg)
    r.bm25.load()
    assert r.bm25.index_tokenizer == "en_regex"
    seqs = [r.bm25.document_tokens(c.text) for c in r.bm25.chunks]  # (cut once, shared, left unchanged)
    return r, seqs


def named(r, pat):
    """The vocabulary tokens the plain evaluator picks for a Wildcard or a Fuzzy, in vocabulary order."""
    from legal_rag_amd.retrieval.terms import Wildcard
    key = ("w", pat.pattern) if isinstance(pat, Wildcard) else ("f", pat.token, pat.edits)
    return [t for t in r.bm25.bm25.vocab() if VC.fits(key, t)[0]]


def stand_in(r, pat):
    """What the pattern must behave like: the OneOf of its tokens, the one token, or a token nobody holds."""
    from legal_rag_amd.retrieval.terms import OneOf
    toks = named(r, pat)
    return OneOf(*toks) if len(toks) > 1 else toks[0] if toks else "zzzqnotoken"


def cases(r):
    """[(name, Terms with patterns, the same Terms over the evaluator's OneOfs)]"""
    from legal_rag_amd.retrieval.terms import Fuzzy, NearOf, OneOf, PhraseOf, Terms, Wildcard
    s = lambda p: stand_in(r, p)  # noqa: E731
    warr, ee, sell, buy, none, secur = (Fuzzy("warrenty"), Wildcard("*ee"), Wildcard("s?ll*"), Wildcard("b?y*"), Wildcard("zzq*x"),
                                        Fuzzy("securty", edits=2))
    single = next(p for p in (Fuzzy("warrenty"), Fuzzy("judgement"), Fuzzy("lesee"), Wildcard("warr?nty")) if len(named(r, p)) == 1)
    assert len(named(r, none)) == 0 and len(named(r, ee)) > 5 and len(named(r, sell)) > 2 and len(named(r, secur)) >= 2
    return [("fuzzy", Terms(all_of=[warr]), Terms(all_of=[s(warr)])),
            ("wildcard", Terms(all_of=[ee, "goods"]), Terms(all_of=[s(ee), "goods"])),
            ("no match", Terms(any_of=[none, sell]), Terms(any_of=[s(none), s(sell)])),
            ("nothing at all", Terms(all_of=[none]), Terms(all_of=[s(none)])),
            ("single match", Terms(all_of=[single]), Terms(all_of=[s(single)])),
            ("in a OneOf", Terms(all_of=[OneOf("lessor", Fuzzy("lesee"))]), Terms(all_of=[OneOf("lessor", *named(r, Fuzzy("lesee")))])),
            ("in a PhraseOf", Terms(all_of=[PhraseOf(secur, "interest")]), Terms(all_of=[PhraseOf(s(secur), "interest")])),
            ("in a NearOf", Terms(all_of=[NearOf(sell, buy, distance=5)]), Terms(all_of=[NearOf(s(sell), s(buy), distance=5)])),
            ("under none_of", Terms(all_of=["goods"], none_of=[sell]), Terms(all_of=["goods"], none_of=[s(sell)]))]


def test_a_pattern_is_the_oneof_of_the_tokens_the_evaluator_picks(live):
    from legal_rag_amd.retrieval.facets import Facets
    r, seqs = live
    spec = Facets(by=("law_name", "section"), top=8)
    for name, t, want in cases(r):
        rows = [i for i, seq in enumerate(seqs) if t.matches(seq)]
        assert rows == [i for i, seq in enumerate(seqs) if want.matches(seq)], name  # the classes' own rule agrees
        assert r._term_rows("search_bm25", r.bm25.chunks, None, t).tolist() == rows, name
        assert r.count(terms=t) == r.count(terms=want) == len(rows), name
        assert r.facets(terms=t, spec=spec) == r.facets(terms=want, spec=spec), name
        if name == "nothing at all":
            assert rows == [] and r.search(QUESTIONS[0], top_k=TOP_K, terms=t) == [] and r.search_bm25(QUESTIONS[0], TOP_K, terms=t) == []
            continue
        assert 0 < len(rows) < len(seqs), name
        got = r.search(QUESTIONS[0], top_k=TOP_K, terms=t)
        same(got, r.search(QUESTIONS[0], top_k=TOP_K, terms=want))
        assert len(got) == min(TOP_K, len(rows)) and {h.chunk.id for h in got} <= {r.bm25.chunks[i].id for i in rows}, name
        same(r.search_bm25(QUESTIONS[2], TOP_K, terms=t), r.search_bm25(QUESTIONS[2], TOP_K, terms=want))
        hl, hl_want = r.highlight(QUESTIONS[0], got[:5], terms=t), r.highlight(QUESTIONS[0], got[:5], terms=want)
        for a, b in zip(hl, hl_want):
            assert (a.window_tokens, a.score, [(m.token, m.slot) for m in a.marks], a.n_marks_in_chunk) == \
                (b.window_tokens, b.score, [(m.token, m.slot) for m in b.marks], b.n_marks_in_chunk), name
        if name == "fuzzy":
            assert all("warrenty~1" in a.found for a in hl)  # (the slot's label is the pattern's)
    # a batch resolves its distinct patterns once and equals the single calls
    ts = [t for _, t, _ in cases(r)]
    assert r.count_batch(terms=ts) == [r.count(terms=t) for t in ts]
    out = r.search_batch([QUESTIONS[j % 3] for j in range(len(ts))], top_k=TOP_K, terms=ts)
    for j, hits in enumerate(out):
        same(hits, r.search(QUESTIONS[j % 3], top_k=TOP_K, terms=ts[j]))


def test_expand_equals_the_evaluator_and_the_cap_names_the_member(live):
    from legal_rag_amd.retrieval.terms import Fuzzy, Wildcard
    r, _ = live
    m = r.bm25.vocab_matcher()
    assert m is r.bm25.vocab_matcher() and m.device == r.bm25.device_index and m.tokens == list(r.bm25.bm25.vocab())
    pats = [Fuzzy("warrenty"), Wildcard("*ee"), Fuzzy("recieve"), Fuzzy("judgement", edits=2), Wildcard("in*ment"), Fuzzy("warrenty")]
    got = m.expand(pats)
    assert list(got) == pats[:5]
    for p in pats:
        key = ("w", p.pattern) if isinstance(p, Wildcard) else ("f", p.token, p.edits)
        assert list(got[p]) == [(t, VC.fits(key, t)[1]) for t in m.tokens if VC.fits(key, t)[0]], p
    assert {"receive", "relieve"} <= {t for t, _ in got[Fuzzy("recieve")]} or "receive" not in m.tokens
    with pytest.raises(ValueError, match=r"Wildcard\('\*e\*'\) names \d+ vocabulary tokens, more than 5"):
        m.expand([Wildcard("*e*")], item_cap=5)
    with pytest.raises(TypeError):
        m.expand(["sell"])
    assert m.expand([]) == {}
    # a token -> id mapping is laid out by id, whatever its order; ids that are not 0 .. n - 1 are refused
    from legal_rag_amd.retrieval.vocab_match import VocabMatcher
    shuffled = VocabMatcher({"sells": 2, "sell": 0, "tell": 1}, device=m.device)
    assert shuffled.tokens == ["sell", "tell", "sells"] and shuffled.expand([Fuzzy("sell")]) == {Fuzzy("sell"): (("sell", 0), ("tell", 1), ("sells", 1))}
    for bad in ({"a": 1}, {"a": 0, "b": 0}, {"a": -1, "b": 0}):
        with pytest.raises(ValueError, match="term ids"):
            VocabMatcher(bad, device=m.device)


def test_suggest_on_a_misspelling(live):
    from legal_rag_amd.retrieval.terms import Fuzzy
    from legal_rag_amd.retrieval.vocab_match import Suggestion
    r, _ = live
    assert r.fuzzy("Warrenty", edits=1) == Fuzzy("warrenty", edits=1) and r.fuzzy("lesee", 2).edits == 2
    with pytest.raises(ValueError, match="exactly one"):
        r.fuzzy("two words")
    df = r.bm25.bm25._doc_frequencies()
    got = r.suggest("Warrenty", edits=2, top=5)
    want = sorted((Suggestion(t, VC.osa("warrenty", t), df[t]) for t in df if abs(len(t) - 8) <= 2 and VC.osa("warrenty", t) <= 2),
                  key=lambda s: (s.distance, -s.doc_freq, s.token))
    assert got == tuple(want[:5]) and got[0].token == "warranty" and got[0].distance == 1 and got[0].doc_freq == df["warranty"] > 0
    both = r.suggest_batch(["Warrenty", "goods", "lesee"], edits=1, top=3)
    assert both[0] == r.suggest("warrenty", edits=1, top=3) and both[1][0] == Suggestion("goods", 0, df["goods"])
    assert both[2][0].token == "lessee" and r.suggest_batch([]) == []
    # a word no longer than the edits takes len(word) - 1 of them and never fails the batch
    absent = next(ch for ch in "0123456789zqxjkvw" if ch not in df and r.bm25.document_tokens(ch) == [ch])
    short = r.suggest_batch(["a", "of", absent, "Warrenty"], edits=2, top=50)
    assert short[0] == (Suggestion("a", 0, df["a"]),) and short[2] == () and short[3] == r.suggest("warrenty", edits=2, top=50)
    assert short[1] == tuple(sorted((Suggestion(t, VC.osa("of", t), df[t]) for t in df if len(t) <= 3 and VC.osa("of", t) <= 1),
                                    key=lambda s: (s.distance, -s.doc_freq, s.token)))
    assert short[1][0] == Suggestion("of", 0, df["of"]) and all(s.distance <= 1 for s in short[1])
    for bad in (0, 3, True):
        with pytest.raises(ValueError, match="edits"):
            r.suggest("warrenty", edits=bad)


@pytest.mark.parametrize("token_stream", (None, "carry"))
def test_a_live_ingest_and_a_removal_are_seen_by_the_next_fuzzy_and_suggest(tmp_path, token_stream):
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    from legal_rag_amd.retrieval.terms import Fuzzy, NearOf, Terms
    every = corpus()
    cfg, r = retriever(tmp_path, every[:120], incremental=True)
    if token_stream is not None:
        cfg.retrieval.token_stream = r.cfg.retrieval.token_stream = token_stream
    f = Fuzzy("warranty")
    # (the live index cuts blanks as tokens of their own: the class span is a Near, not a phrase)
    t, tp = Terms(all_of=[f]), Terms(all_of=[NearOf(f, "clause", distance=3, ordered=True)])
    host = lambda terms: sum(terms.matches(r.bm25.document_tokens(c.text)) for c in r.bm25.chunks)  # noqa: E731
    before = r.count(terms=t)
    assert before == host(t) and host(tp) == 0
    m0 = r.bm25.vocab_matcher()
    assert "warrantx" not in r.bm25.bm25.vocab() and before > 0 and r.count(terms=tp) == 0
    assert all(s.token != "warrantx" for s in r.suggest("warrantx", edits=1))
    new = every[300].model_copy(update={"id": "new-warrantx", "text": "The warrantx clause is void and unknownword applies."})
    assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "more.jsonl", [new])) == 1
    assert "warrantx" in r.bm25.bm25.vocab() and r.bm25.vocab_matcher() is not m0  # (the same vocab() object, longer)
    assert host(t) == before + 1 and host(tp) == 1  # (the certificate: the new chunk, and only it, holds the class span)
    assert r.count(terms=t) == before + 1 and r.count(terms=tp) == 1
    assert r.suggest("warrantx", edits=1)[0].token == "warrantx" and r.suggest("warrantx", edits=1)[0].doc_freq == 1
    hit = r.search_bm25("warrantx clause", 5, terms=tp)
    assert [h.chunk.id for h in hit] == ["new-warrantx"]
    assert IncrementalBM25Builder(cfg).remove_ids(["new-warrantx"]) == 1
    assert "warrantx" not in r.bm25.bm25.vocab()
    assert r.count(terms=t) == before and r.count(terms=tp) == 0
    assert all(s.token != "warrantx" for s in r.suggest("warrantx", edits=1))


def test_the_refusals_before_any_launch(live, monkeypatch):
    from legal_rag_amd import _native
    from legal_rag_amd.retrieval.terms import Fuzzy, Terms
    r, _ = live
    t = Terms(all_of=[Fuzzy("warrenty")])
    assert r.count(terms=t) > 0  # (the handles exist before the launches are forbidden)

    def no_launch(*a, **k):
        raise AssertionError("a refused call reached the library")
    monkeypatch.setattr(_native.VocabIndex, "match", no_launch)
    monkeypatch.setattr(r.bm25, "shard", object(), raising=False)
    for call in (lambda: r.count(terms=t), lambda: r.facets(terms=t), lambda: r.search_bm25("goods", 5, terms=t),
                 lambda: r.highlight("goods", [], terms=t), lambda: r.suggest("warrenty")):
        with pytest.raises(ValueError, match="row-sharded index"):
            call()
    monkeypatch.undo()
    monkeypatch.setattr(_native.VocabIndex, "match", no_launch)
    own = r.bm25
    try:
        r.bm25 = SimpleNamespace(search=lambda *a, **k: [], chunks=own.chunks)
        for call in (lambda: r.count(terms=t), lambda: r.facets(terms=t), lambda: r.suggest("warrenty"), lambda: r.fuzzy("warrenty")):
            with pytest.raises(ValueError, match="own BM25 retriever"):
                call()
    finally:
        r.bm25 = own
    with pytest.raises(TypeError):
        r.count(terms=[t])
    monkeypatch.undo()
    assert r.count(terms=t) > 0

"""Proximity constraints through the public interface, on the UCC-en fixture (tests/golden/corpus/law_en.jsonl, 591 articles,
the BM25 index cut by the English index rule): search(q, terms=Terms(all_of=[Near(...)])) equals
search(q, scope=Scope(chunk_ids=ids)) with `ids` computed on the host by a window scan of each chunk's tokens
(Terms.matches), hit for hit, with tolerance 0; every returned chunk's token sequence holds the Near; the row counts are
those of a window scan taken on the CPU over the 591 articles; batches that mix phrases and Nears equal the single searches."""
import pytest

from test_phrase_api_gpu import QUESTIONS, TOP_K, ids_of, same, sequences, ucc_chunks

pytestmark = pytest.mark.gpu

# tokens -> (conjunction, /1, /5, /10, /255, +1, +5, +10, +255): articles of the fixture, by a window scan on the CPU
COUNTS = {
    ("buyer", "seller"): (72, 2, 29, 47, 72, 1, 12, 22, 56),
    ("security", "interest"): (135, 121, 128, 132, 135, 121, 126, 129, 133),
    ("holder", "due", "course"): (23, 0, 21, 21, 23, 0, 21, 21, 21),
}
DISTANCES = (1, 5, 10, 255)


@pytest.fixture(scope="module")
def live(tmp_path_factory):
    """The whole fixture behind a live HybridRetriever, built as tests/test_phrase_api_gpu.py builds it."""
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.colbert_builder import build_colbert_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from test_replace_api_gpu import _cfg
    root = tmp_path_factory.mktemp("near_api")
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


def test_the_counts_of_the_fixture_on_the_gpu_and_on_the_host(live):
    from legal_rag_amd.retrieval.terms import Near, Phrase, Terms
    cfg, r = live
    assert r.near("Buyer Seller", distance=5) == Near("buyer", "seller", distance=5)
    assert r.near("holder due course", 5, ordered=True) == Near("holder", "due", "course", distance=5, ordered=True)
    assert not r.bm25.gpu_index().tokens_info()[0]  # the stream is made on the first Near
    n_of = lambda t: len(r.search(QUESTIONS[0], top_k=200, terms=t))  # noqa: E731  (the fused search ranks every row of a scope)
    seqs = sequences(r)  # (cut once)
    ids = lambda t: [c.id for c, seq in seqs if t.matches(seq)]  # noqa: E731
    for toks, want in COUNTS.items():
        nears = [Near(*toks, distance=n, ordered=o) for o in (False, True) for n in DISTANCES]
        host = [ids(Terms(all_of=[x])) for x in nears]
        assert (len(ids(Terms(all_of=[toks]))),) + tuple(len(x) for x in host) == want, toks
        out = r.search_batch([QUESTIONS[0]] * len(nears), top_k=200, terms=[Terms(all_of=[x]) for x in nears])
        assert tuple(len(h) for h in out) == want[1:], toks
        for want_ids, hits in zip(host, out):
            assert sorted(h.chunk.id for h in hits) == sorted(want_ids)
    assert r.bm25.gpu_index().tokens_info() == (True, 148_101)
    goods = Near("goods", "goods", distance=5)
    assert n_of(Terms(all_of=[goods])) == 31 == len(ids(Terms(all_of=[goods]))) and len(ids(Terms(all_of=["goods"]))) == 213
    # security +1 interest is the phrase
    plus1 = Terms(all_of=[Near("security", "interest", distance=1, ordered=True)])
    phrase = Terms(all_of=[Phrase("security", "interest")])
    assert ids(plus1) == ids(phrase) and n_of(plus1) == n_of(phrase) == 121


def test_search_with_a_near_equals_the_explicit_scope_and_every_hit_holds_it(live):
    from legal_rag_amd.retrieval.scope import Scope
    from legal_rag_amd.retrieval.terms import Near, Phrase, Terms
    cfg, r = live
    seqs = {c.id: seq for c, seq in sequences(r)}
    bs, hdc = Near("buyer", "seller", distance=5), Near("holder", "due", "course", distance=5, ordered=True)
    si10 = Near("interest", "security", distance=10, ordered=True)
    for q in QUESTIONS:
        for x in (bs, hdc, si10, Near("goods", "goods", distance=5)):
            t = Terms(all_of=[x])
            ids = ids_of(r, t)
            got = r.search(q, top_k=TOP_K, terms=t)
            same(got, r.search(q, top_k=TOP_K, scope=Scope(chunk_ids=ids)))
            assert len(got) == min(TOP_K, len(ids)) > 0 and all(x.within(seqs[h.chunk.id]) for h in got)
            assert [h.rank for h in got] == list(range(1, len(got) + 1))
        assert r.search(q, top_k=TOP_K, terms=Terms(all_of=[Near("holder", "due", "course", distance=1)])) == []
    # excluded, as an alternative, and beside plain tokens and a phrase
    for t in (Terms(none_of=[bs]), Terms(all_of=["goods", ("contract", bs)], none_of=[Phrase("security", "interest")]),
              Terms(any_of=[hdc, bs]), Terms(all_of=[bs], none_of=[Near("buyer", "seller", distance=5, ordered=True)])):
        ids = ids_of(r, t)
        assert 0 < len(ids) < 591
        got = r.search(QUESTIONS[0], top_k=TOP_K, terms=t)
        same(got, r.search(QUESTIONS[0], top_k=TOP_K, scope=Scope(chunk_ids=ids)))
        assert all(t.matches(seqs[h.chunk.id]) for h in got) and len(got) == min(TOP_K, len(ids))
    assert len(ids_of(r, Terms(none_of=[bs]))) == 591 - 29


def test_batches_mix_phrases_and_nears_and_the_per_channel_searches_take_nears(live):
    from legal_rag_amd.retrieval.scope import Scope
    from legal_rag_amd.retrieval.terms import Near, Phrase, Terms
    cfg, r = live
    si, bs = Phrase("security", "interest"), Near("buyer", "seller", distance=5)
    hdc = Near("holder", "due", "course", distance=5)
    sec = next(c.section for c, seq in sequences(r) if c.section and bs.within(seq))
    terms = [None, Terms(all_of=[si]), Terms(all_of=[bs]), Terms(all_of=[Near("holder", "due", "course", distance=1)]),
             Terms(none_of=[bs]), Terms(all_of=[bs]), Terms(all_of=["goods"]), Terms(all_of=[hdc], none_of=[Phrase("holder", "in", "due", "course")]),
             Terms(any_of=[si, hdc])]
    scopes = [None, None, None, None, None, Scope(section=sec), None, None, None]
    qs = [QUESTIONS[j % len(QUESTIONS)] for j in range(len(terms))]
    out = r.search_batch(qs, top_k=TOP_K, terms=terms, scopes=scopes)
    for j, hits in enumerate(out):
        same(hits, r.search(qs[j], top_k=TOP_K, terms=terms[j], scope=scopes[j]))
    assert out[3] == [] and out[7] == [] and all(out[j] for j in (0, 1, 2, 4, 5, 6, 8))
    assert all(h.chunk.section == sec for h in out[5])
    same(out[2], r.search(qs[2], top_k=TOP_K, scope=Scope(chunk_ids=ids_of(r, terms[2]))))
    same(out[8], r.search(qs[8], top_k=TOP_K, scope=Scope(chunk_ids=ids_of(r, terms[8]))))
    t = Terms(all_of=[hdc])
    ids = ids_of(r, t)
    for fn in (r.search_dense, r.search_bm25, r.search_colbert):
        got = fn(QUESTIONS[0], TOP_K, terms=t)
        same(got, fn(QUESTIONS[0], TOP_K, scope=Scope(chunk_ids=ids)))
        assert len(got) == min(TOP_K, len(ids))


def test_a_status_word_raises_and_names_the_near(live, monkeypatch):
    from legal_rag_amd.retrieval import hybrid_retriever as HR
    from legal_rag_amd.retrieval.terms import Near, Phrase, Terms
    cfg, r = live
    bs, si = Near("buyer", "seller", distance=5), Phrase("security", "interest")
    pack = HR._pack_terms

    def short(*a, **k):
        tt = pack(*a, **k)
        tt.near_cand_max, tt.phr_cand_max = 3, min(tt.phr_cand_max, 3)  # far below the drivers: the status words are 1
        return tt
    monkeypatch.setattr(HR, "_pack_terms", short)
    with pytest.raises(RuntimeError, match=r"Near\('buyer', 'seller', distance=5\) of the batch overflowed"):
        r.search_batch([QUESTIONS[0]] * 2, top_k=TOP_K, terms=[Terms(all_of=[bs]), Terms(all_of=["goods"])])
    with pytest.raises(RuntimeError, match=r"Phrase\('security', 'interest'\) of the batch overflowed"):
        r.search_batch([QUESTIONS[0]] * 2, top_k=TOP_K, terms=[Terms(all_of=[bs]), Terms(all_of=[si])])
    with pytest.raises(RuntimeError, match=r"Near\('buyer', 'seller', distance=5\) overflowed"):
        r.search_bm25(QUESTIONS[0], TOP_K, terms=Terms(all_of=[bs]))

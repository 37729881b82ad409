"""A root expander and alternatives INSIDE a phrase or a Near through the public interface, on the UCC-en fixture
(tests/golden/corpus/law_en.jsonl, 591 articles, the BM25 index cut by the English index rule): the rows a NearOf / PhraseOf
resolves to equal the rows the host reference (`within` over the articles' own tokens) accepts; search(q, terms=...) equals
search(q, scope=Scope(chunk_ids=ids)) hit for hit with tolerance 0, through search, search_batch and the per-channel
searches; buy! /5 sell! names strictly more articles than the 29 of Near("buyer", "seller", distance=5), and "secur!
interest!" at least those of "security interest"; a status word raises and names the member; the overlap rule raises
before any launch."""
import numpy as np
import pytest

from test_phrase_api_gpu import QUESTIONS, TOP_K, ids_of, same, sequences, ucc_chunks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def live(tmp_path_factory):
    """The whole fixture behind a live HybridRetriever, built as tests/test_phrase_api_gpu.py builds it."""
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.colbert_builder import build_colbert_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from test_replace_api_gpu import _cfg
    root = tmp_path_factory.mktemp("class_span_api")
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


def spans(r):
    from legal_rag_amd.retrieval.terms import NearOf, OneOf, PhraseOf
    return (NearOf(r.prefix("Buy"), r.prefix("Sell"), distance=5), PhraseOf(r.prefix("Secur"), r.prefix("Interest")),
            NearOf(OneOf("buyer", "purchaser"), r.prefix("accept"), distance=3, ordered=True),
            NearOf(r.prefix("sell"), r.prefix("good"), distance=5), PhraseOf("security", OneOf("interest", "interests")))


def test_the_counts_of_the_issue_device_and_host_agree_and_the_stems_find_more(live):
    """The count table of DESIGN.md §4.21: buy! /5 sell! 37 articles against the 29 of buyer /5 seller; "secur! interest!"
    124 against the 121 of "security interest"."""
    from legal_rag_amd.retrieval.terms import Near, NearOf, Phrase, PhraseOf, Prefix, Terms
    cfg, r = live
    seqs = sequences(r)  # (cut once)
    n_of = NearOf(Prefix("buy"), Prefix("sell"), distance=5)
    assert spans(r)[0] == n_of
    vocab = r.bm25.bm25.vocab()
    assert len([w for w in vocab if w.startswith("buy")]) == 6 and len([w for w in vocab if w.startswith("sell")]) == 5
    for wide, exact, counts in ((n_of, Near("buyer", "seller", distance=5), (37, 29)),
                                (PhraseOf(Prefix("secur"), Prefix("interest")), Phrase("security", "interest"), (124, 121))):
        host = [i for i, (c, toks) in enumerate(seqs) if wide.within(toks)]
        host_exact = [i for i, (c, toks) in enumerate(seqs) if exact.within(toks)]
        rows = r._term_rows("search_bm25", r.bm25.chunks, None, Terms(all_of=[wide]))
        rows_exact = r._term_rows("search_bm25", r.bm25.chunks, None, Terms(all_of=[exact]))
        assert rows.dtype == np.int64 and rows.tolist() == host and rows_exact.tolist() == host_exact
        assert (len(host), len(host_exact)) == counts and len(host) > len(host_exact) and set(host_exact) <= set(host)
    assert r.bm25.gpu_index().tokens_info()[0]  # a class span needs the token stream: it was made on the first one


def test_search_with_a_class_span_equals_the_explicit_scope_and_every_hit_holds_it(live):
    from legal_rag_amd.retrieval.scope import Scope
    from legal_rag_amd.retrieval.terms import Terms
    cfg, r = live
    seqs = {c.id: seq for c, seq in sequences(r)}
    for q in QUESTIONS[:2]:
        for item in spans(r):
            t = Terms(all_of=[item])
            ids = ids_of(r, t)
            got = r.search(q, top_k=TOP_K, terms=t)
            same(got, r.search(q, top_k=TOP_K, scope=Scope(chunk_ids=ids)))  # ids and score bits of the unscoped channels
            assert len(got) == min(TOP_K, len(ids)) > 0, item
            assert all(item.within(seqs[h.chunk.id]) for h in got)
            assert [h.rank for h in got] == list(range(1, len(got) + 1))


def test_class_spans_in_every_field_in_a_batch_and_in_the_per_channel_searches(live, monkeypatch):
    from legal_rag_amd.retrieval import hybrid_retriever as HR
    from legal_rag_amd.retrieval.scope import Scope
    from legal_rag_amd.retrieval.terms import Near, NearOf, Phrase, PhraseOf, Prefix, Terms
    cfg, r = live
    seqs = {c.id: seq for c, seq in sequences(r)}
    near, phr, alt, goods, _ = spans(r)
    mixed = Terms(all_of=[(phr, Phrase("security", "interest"), Prefix("debtor"))], none_of=[near])
    anyof = Terms(any_of=[near, alt], none_of=[(goods, "lease")])
    folded = Terms(all_of=[NearOf("buyer", "seller", distance=5), PhraseOf("security", "interest")])
    plain = Terms(all_of=[Near("buyer", "seller", distance=5), Phrase("security", "interest")])
    tables = []
    pack = HR._pack_terms

    def recording(*a, **k):
        tables.append(pack(*a, **k))
        return tables[-1]
    monkeypatch.setattr(HR, "_pack_terms", recording)
    for t in (mixed, anyof, Terms(all_of=[(near, goods)]), Terms(all_of=["goods"], none_of=[near])):
        ids = ids_of(r, t)
        assert 0 < len(ids) < 591, t
        got = r.search(QUESTIONS[0], top_k=TOP_K, terms=t)
        same(got, r.search(QUESTIONS[0], top_k=TOP_K, scope=Scope(chunk_ids=ids)))
        assert len(got) == min(TOP_K, len(ids)) and all(t.matches(seqs[h.chunk.id]) for h in got)
    # a batch: equal class spans are stored once, a folded item IS the plain one, and the batch equals the single searches
    terms = [None, Terms(all_of=[near]), mixed, anyof, Terms(all_of=[NearOf(Prefix("buy"), Prefix("sell"), distance=5)]), folded, plain,
             Terms(all_of=[NearOf(Prefix("zzzq"), Prefix("sell"), distance=5)])]
    sec = next(c.section for c in r.bm25.chunks if c.section and near.within(seqs[c.id]))
    scopes = [None, Scope(section=sec), None, None, None, None, None, None]
    qs = [QUESTIONS[j % len(QUESTIONS)] for j in range(len(terms))]
    del tables[:]
    out = r.search_batch(qs, top_k=TOP_K, terms=terms, scopes=scopes)
    tt = tables[0]
    # near, phr, alt, goods and the span with the stem nothing starts with; the Near and the Phrase once each, shared by `folded`
    assert (tt.n_cspan, tt.n_near, tt.n_phr) == (5, 1, 1) and tt.cspans[:4] == (near, phr, alt, goods)
    for j, hits in enumerate(out):
        same(hits, r.search(qs[j], top_k=TOP_K, terms=terms[j], scope=scopes[j]))
    assert out[7] == [] and all(out[j] for j in range(7)) and all(h.chunk.section == sec for h in out[1])
    same(out[5], r.search(qs[5], top_k=TOP_K, terms=plain))  # the folded constraint is the plain one
    same(out[4], r.search(qs[4], top_k=TOP_K, scope=Scope(chunk_ids=ids_of(r, terms[4]))))
    for t in (Terms(all_of=[near]), mixed):  # the per-channel searches
        ids = ids_of(r, t)
        for fn in (r.search_dense, r.search_bm25, r.search_colbert):
            got = fn(QUESTIONS[0], TOP_K, terms=t)
            same(got, fn(QUESTIONS[0], TOP_K, scope=Scope(chunk_ids=ids)))
            assert len(got) == min(TOP_K, len(ids))


def test_a_status_word_raises_and_names_the_member_and_the_overlap_rule_raises_before_any_launch(live, monkeypatch):
    from legal_rag_amd.retrieval import hybrid_retriever as HR
    from legal_rag_amd.retrieval.terms import NearOf, Prefix, Terms
    cfg, r = live
    near = spans(r)[0]
    bad = NearOf("seller", Prefix("sell"), distance=3)
    with pytest.raises(ValueError, match=r"NearOf\('seller', Prefix\('sell'\), distance=3\): members 0 and 1 name overlapping"):
        r.search(QUESTIONS[0], top_k=TOP_K, terms=Terms(all_of=[bad]))
    with pytest.raises(ValueError, match="overlapping"):
        r.search_bm25(QUESTIONS[0], TOP_K, terms=Terms(none_of=[bad]))
    assert r.search(QUESTIONS[0], top_k=TOP_K, terms=Terms(all_of=[NearOf("seller", Prefix("sell"), distance=3, ordered=True)]))
    pack = HR._pack_terms
    seqs = [toks for _, toks in sequences(r)]

    def short(*a, **k):
        tt = pack(*a, **k)
        # The capacity is the whole list array's and a union's bound is the SUM of its tokens' lists, so the unions leave
        # room behind them: give them exactly their lists, and the class spans three rows — far below theirs: status 2
        tt.union_rows_cap = sum(sum(1 for toks in seqs if u.within(toks)) for u in tt.unions)
        tt.cspan_rows_cap = 3
        return tt
    monkeypatch.setattr(HR, "_pack_terms", short)
    with pytest.raises(RuntimeError, match=r"NearOf\(Prefix\('buy'\), Prefix\('sell'\), distance=5\) of the batch overflowed"):
        r.search_batch([QUESTIONS[0]] * 2, top_k=TOP_K, terms=[Terms(all_of=[near]), Terms(all_of=["goods"])])
    with pytest.raises(RuntimeError, match=r"NearOf\(Prefix\('buy'\), Prefix\('sell'\), distance=5\) overflowed"):
        r.search_bm25(QUESTIONS[0], TOP_K, terms=Terms(all_of=[near]))

"""The root expander and alternatives through the public interface, on the UCC-en fixture (tests/golden/corpus/law_en.jsonl,
591 articles, the BM25 index cut by the English index rule): the rows a Prefix resolves to equal the rows whose tokens
`Terms.matches` on the host and are merged, not concatenated; search(q, terms=Terms(all_of=[Prefix(...)])) equals
search(q, scope=Scope(chunk_ids=ids)) hit for hit with tolerance 0, and every hit holds a token with the stem; a OneOf and a
Prefix stand beside each other, a Phrase and a Near in one group, through search, search_batch and the per-channel searches;
a status word raises and names the member; a stem that matches nothing is an unknown token."""
import numpy as np
import pytest

from test_phrase_api_gpu import QUESTIONS, TOP_K, ids_of, same, sequences, ucc_chunks

pytestmark = pytest.mark.gpu

STEMS = ("sell", "secur", "warrant", "buy")


@pytest.fixture(scope="module")
def live(tmp_path_factory):
    """The whole fixture behind a live HybridRetriever, built as tests/test_phrase_api_gpu.py builds it."""
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.colbert_builder import build_colbert_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from test_replace_api_gpu import _cfg
    root = tmp_path_factory.mktemp("prefix_api")
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


def test_a_prefix_resolves_to_the_rows_the_host_rule_names_merged_not_concatenated(live):
    from legal_rag_amd.retrieval.terms import OneOf, Prefix, Terms, pack
    cfg, r = live
    assert r.prefix("Sell") == Prefix("sell")
    model = r.bm25.bm25
    vocab, df = model.vocab(), model._doc_frequencies()
    seqs = sequences(r)  # (cut once)
    for stem in STEMS:
        t = Terms(all_of=[Prefix(stem)])
        tt = pack([(None, t)], vocab, df, int(model.corpus_size), None, model.sorted_vocab())
        ids = tt.union_ops[1].tolist()
        words = sorted(w for w in vocab if w.startswith(stem))
        assert tt.n_union == 1 and len(ids) >= 2 and ids == sorted(vocab[w] for w in words), stem
        rows = r._term_rows("search_bm25", r.bm25.chunks, None, t)
        want = [i for i, (c, toks) in enumerate(seqs) if t.matches(toks)]
        assert rows.dtype == np.int64 and rows.tolist() == want, stem
        assert max(df[w] for w in words) < len(want) < sum(df[w] for w in words), stem  # merged and de-duplicated
        # the OneOf of the same tokens shares the list
        one = Terms(all_of=[OneOf(*words)])
        assert r._term_rows("search_bm25", r.bm25.chunks, None, one).tolist() == want
        both = pack([(None, t), (None, one)], vocab, df, int(model.corpus_size), None, model.sorted_vocab())
        assert both.n_union == 1 and both.n_cons == 2
    assert not r.bm25.gpu_index().tokens_info()[0]  # a union needs the postings alone: no token stream was made


def test_search_with_a_prefix_equals_the_explicit_scope_and_every_hit_holds_the_stem(live):
    from legal_rag_amd.retrieval.scope import Scope
    from legal_rag_amd.retrieval.terms import Prefix, Terms
    cfg, r = live
    seqs = {c.id: seq for c, seq in sequences(r)}
    for q in QUESTIONS:
        for stem in ("sell", "warrant"):
            t = Terms(all_of=[Prefix(stem)])
            ids = ids_of(r, t)
            got = r.search(q, top_k=TOP_K, terms=t)
            same(got, r.search(q, top_k=TOP_K, scope=Scope(chunk_ids=ids)))  # ids and score bits
            assert len(got) == min(TOP_K, len(ids)) > 0
            assert all(any(w.startswith(stem) for w in seqs[h.chunk.id]) for h in got)
            assert [h.rank for h in got] == list(range(1, len(got) + 1))
    # more hits than the exact token finds
    assert len(ids_of(r, Terms(all_of=[Prefix("sell")]))) > len(ids_of(r, Terms(all_of=["seller"])))


def test_alternatives_in_a_conjunction_and_groups_with_a_phrase_and_a_near(live, monkeypatch):
    from legal_rag_amd.retrieval import hybrid_retriever as HR
    from legal_rag_amd.retrieval.scope import Scope
    from legal_rag_amd.retrieval.terms import Near, OneOf, Phrase, Prefix, Terms
    cfg, r = live
    seqs = {c.id: seq for c, seq in sequences(r)}
    alt = Terms(all_of=[(OneOf("buyer", "purchaser"), Prefix("sell"))], none_of=[Prefix("leas")])
    mixed = Terms(all_of=[(Prefix("secur"), Phrase("security", "interest"), Near("debtor", "collateral", distance=10))])
    two = Terms(all_of=[OneOf("buyer", "purchaser"), OneOf("goods", "inventory")])
    tables = []
    pack = HR._pack_terms

    def recording(*a, **k):
        tables.append(pack(*a, **k))
        return tables[-1]
    monkeypatch.setattr(HR, "_pack_terms", recording)
    for t in (alt, mixed, two, Terms(any_of=[Prefix("warrant"), OneOf("lessee", Prefix("bail"))]), Terms(none_of=[Prefix("secur")])):
        ids = ids_of(r, t)
        assert 0 < len(ids) < 591, t
        got = r.search(QUESTIONS[0], top_k=TOP_K, terms=t)
        same(got, r.search(QUESTIONS[0], top_k=TOP_K, scope=Scope(chunk_ids=ids)))
        assert len(got) == min(TOP_K, len(ids)) and all(t.matches(seqs[h.chunk.id]) for h in got)
    assert all(not any(w.startswith("leas") for w in seqs[i]) for i in ids_of(r, alt))
    # a batch: equal unions are stored once, and the batch equals the single searches
    terms = [None, alt, Terms(all_of=[Prefix("sell")]), mixed, Terms(all_of=[OneOf("sell", "seller", "seller's", "selling", "sells")]),
             Terms(all_of=[Prefix("zzzq")]), two, Terms(all_of=[Prefix("sell")])]
    sec = next(c.section for c in r.bm25.chunks if c.section and alt.matches(seqs[c.id]))
    scopes = [None, Scope(section=sec), None, None, None, None, None, None]
    qs = [QUESTIONS[j % len(QUESTIONS)] for j in range(len(terms))]
    del tables[:]
    out = r.search_batch(qs, top_k=TOP_K, terms=terms, scopes=scopes)
    batch_table = tables[0]
    # sell! (three times, once as a OneOf), buyer|purchaser (twice), leas!, secur!, goods|inventory
    assert batch_table.n_union == 5 and batch_table.n_phr == 1 and batch_table.n_near == 1
    for j, hits in enumerate(out):
        same(hits, r.search(qs[j], top_k=TOP_K, terms=terms[j], scope=scopes[j]))
    assert out[5] == [] and all(out[j] for j in (0, 1, 2, 3, 4, 6, 7)) and all(h.chunk.section == sec for h in out[1])
    same(out[2], r.search(qs[2], top_k=TOP_K, scope=Scope(chunk_ids=ids_of(r, terms[2]))))
    for t in (alt, mixed):  # the per-channel searches
        ids = ids_of(r, t)
        for fn in (r.search_dense, r.search_bm25, r.search_colbert):
            got = fn(QUESTIONS[0], TOP_K, terms=t)
            same(got, fn(QUESTIONS[0], TOP_K, scope=Scope(chunk_ids=ids)))
            assert len(got) == min(TOP_K, len(ids))


def test_a_status_word_raises_and_names_the_member(live, monkeypatch):
    from legal_rag_amd.retrieval import hybrid_retriever as HR
    from legal_rag_amd.retrieval.terms import OneOf, Prefix, Terms
    cfg, r = live
    sell, alt = Prefix("sell"), OneOf("buyer", "purchaser")
    pack = HR._pack_terms

    def short(*a, **k):
        tt = pack(*a, **k)
        tt.union_rows_cap = 3  # far below the lists: the status words are 2
        return tt
    monkeypatch.setattr(HR, "_pack_terms", short)
    with pytest.raises(RuntimeError, match=r"Prefix\('sell'\) of the batch overflowed"):
        r.search_batch([QUESTIONS[0]] * 2, top_k=TOP_K, terms=[Terms(all_of=[sell]), Terms(all_of=["goods"])])
    with pytest.raises(RuntimeError, match=r"OneOf\('buyer', 'purchaser'\) of the batch overflowed"):
        r.search_batch([QUESTIONS[0]] * 2, top_k=TOP_K, terms=[Terms(all_of=["goods"]), Terms(any_of=[alt])])
    with pytest.raises(RuntimeError, match=r"Prefix\('sell'\) overflowed"):
        r.search_bm25(QUESTIONS[0], TOP_K, terms=Terms(all_of=[sell]))
    with pytest.raises(RuntimeError, match=r"OneOf\('buyer', 'purchaser'\) overflowed"):
        r.search_dense(QUESTIONS[0], TOP_K, terms=Terms(all_of=[(alt, "goods")]))


def test_a_stem_that_matches_nothing_is_an_unknown_token_in_each_field(live):
    from legal_rag_amd.retrieval.terms import OneOf, Prefix, Terms
    cfg, r = live
    none = Prefix("zzzq")
    assert not any(w.startswith("zzzq") for w in r.bm25.bm25.vocab())
    q = QUESTIONS[0]
    for nothing in (none, OneOf("zzzq", Prefix("qqqz")), "zzzq"):
        assert r.search(q, top_k=TOP_K, terms=Terms(all_of=[nothing])) == []                  # empties all_of
        assert r.search(q, top_k=TOP_K, terms=Terms(all_of=["goods", (nothing, "seller")])) == []
        assert r.search(q, top_k=TOP_K, terms=Terms(any_of=[nothing])) == []                  # every entry unknown
        same(r.search(q, top_k=TOP_K, terms=Terms(any_of=[nothing, "goods"])), r.search(q, top_k=TOP_K, terms=Terms(any_of=["goods"])))
        same(r.search(q, top_k=TOP_K, terms=Terms(all_of=["goods"], none_of=[nothing])),    # ignored in none_of
             r.search(q, top_k=TOP_K, terms=Terms(all_of=["goods"])))
        assert r.search_bm25(q, TOP_K, terms=Terms(all_of=[nothing])) == []

"""The same-sentence and same-paragraph connectors through the public interface, on the UCC-en fixture
(tests/golden/corpus/law_en.jsonl, 591 articles, the BM25 index cut by the English index rule): count(terms=) of
Within("buyer", "seller") by sentence and by paragraph, ordered and not, equals the brute-force evaluator of
tests/unit_span_cases.py run over the chunk texts; the four sets nest; a Within in none_of, in a tuple group and with a
Prefix and a Fuzzy member; search(q, terms=) equals search(q, scope=Scope(chunk_ids=ids)) hit for hit with tolerance 0 and
every hit's text holds the constraint; highlight marks the members; a live add, remove and replace under token_stream =
"carry" cut only the new chunks; a row-sharded retriever raises."""
import numpy as np
import pytest

import unit_span_cases as UC
from test_phrase_api_gpu import QUESTIONS, TOP_K, same, ucc_chunks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def live(tmp_path_factory):
    """The whole fixture behind a live HybridRetriever, built as tests/test_phrase_api_gpu.py builds it."""
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.colbert_builder import build_colbert_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from test_replace_api_gpu import _cfg
    root = tmp_path_factory.mktemp("unit_span_api")
    chunks = ucc_chunks()
    cfg = _cfg(root / "live")
    cfg.retrieval.min_final_score = -1.0
    build_faiss_index(cfg, chunks)
    build_bm25_index(cfg, chunks)
    build_colbert_index(cfg, chunks)
    r = HybridRetriever(cfg)
    r.bm25.load()
    assert r.bm25.index_tokenizer == "en_regex"
    return cfg, r


def cut(r):
    """[(chunk, its tokens, its break flags)]: the chunk texts cut again by the index's own document rule, the flags by the
    rule of retrieval/units.py."""
    from legal_rag_amd.retrieval.units import break_flags
    lowered = r.bm25.index_tokenizer == "en_regex"  # (the incremental builder's index is not lower-cased)
    out = []
    for c in r.bm25.chunks:
        toks = r.bm25.document_tokens(c.text)
        out.append((c, toks, break_flags(c.text, toks, lowered)[0].tolist()))
    return out


def evaluator_rows(docs, kind, words):
    """The rows the brute-force evaluator accepts for the plain tokens `words` (ids of a vocabulary of its own)."""
    ids = {}
    seqs = [[ids.setdefault(t, len(ids)) for t in toks] for _, toks, _ in docs]
    item = (kind, [ids.get(w, -1) for w in words])
    return [d for d, (_, _, brk) in enumerate(docs) if UC.holds(seqs[d], brk, item, n_terms=len(ids))]


def ids_of(docs, terms):
    return [c.id for c, toks, brk in docs if terms.matches(toks, brk)]


def test_buyer_and_seller_in_one_sentence_and_in_one_paragraph_equal_the_evaluator_and_nest(live):
    from legal_rag_amd.retrieval.terms import Terms, Within
    cfg, r = live
    docs = cut(r)
    assert r.within("Buyer Seller", unit="paragraph", ordered=True) == Within("buyer", "seller", unit="paragraph", ordered=True)
    rows = {}
    for unit, p in (("sentence", 0), ("paragraph", UC.PARAGRAPH)):
        for ordered in (False, True):
            w = r.within("Buyer Seller", unit=unit, ordered=ordered)
            want = evaluator_rows(docs, p | (UC.ORDERED if ordered else 0), ["buyer", "seller"])
            assert r.count(terms=Terms(all_of=[w])) == len(want) > 0, w             # the engine's chain
            got = r._term_rows("search_bm25", r.bm25.chunks, None, Terms(all_of=[w]))   # the host twins
            assert got.dtype == np.int64 and got.tolist() == want, w
            rows[(unit, ordered)] = set(want)
    both = {d for d, (_, toks, _) in enumerate(docs) if "buyer" in toks and "seller" in toks}
    assert len(both) == r.count(terms=Terms(all_of=["buyer", "seller"])) == 72
    assert rows[("sentence", False)] <= rows[("paragraph", False)] <= both
    assert rows[("sentence", True)] <= rows[("paragraph", True)] <= rows[("paragraph", False)]
    assert rows[("sentence", True)] <= rows[("sentence", False)] < both
    info = r.bm25.units_info()
    assert info[0] == r.bm25.gpu_index().breaks_info()[1] == sum(len(t) for _, t, _ in docs)
    assert info[1] == sum(1 + sum(1 for f in b[1:] if f & 1) for _, t, b in docs if t) >= info[2] >= len(docs) and info[3] == 0


def test_a_within_in_none_of_in_a_tuple_group_and_with_a_prefix_and_a_fuzzy_member(live):
    from legal_rag_amd.retrieval.terms import Fuzzy, OneOf, Prefix, Terms, Within
    cfg, r = live
    docs = cut(r)
    bs = Within("buyer", "seller")
    cases = [Terms(all_of=["buyer", "seller"], none_of=[bs]), Terms(all_of=[(bs, "goods", Prefix("accept"))]),
             Terms(all_of=[Within(Prefix("buy"), Prefix("sell"), unit="paragraph")]),
             Terms(any_of=[Within(Fuzzy("warrenty"), OneOf("seller", "lessor"), ordered=True), Within("goods", "goods", "goods")]),
             Terms(all_of=[Within(Prefix("secur"), "interest", "debtor")], none_of=[(Within("collateral", "collateral"), "default")])]
    got = r.count_batch(terms=cases)
    want = [len(ids_of(docs, t)) for t in cases]
    assert got == want and all(0 < n < 591 for n in want), (got, want)
    assert want[0] == 72 - r.count(terms=Terms(all_of=[bs]))
    f = r.facets(terms=cases[2])
    assert f.total == want[2]


def test_search_with_a_within_equals_the_explicit_scope_and_every_hit_holds_it(live):
    from legal_rag_amd.retrieval.scope import Scope
    from legal_rag_amd.retrieval.terms import Prefix, Terms, Within
    cfg, r = live
    docs = cut(r)
    by_id = {c.id: (toks, brk) for c, toks, brk in docs}
    for q in QUESTIONS[:2]:
        for t in (Terms(all_of=[Within("buyer", "seller")]), Terms(all_of=[Within(Prefix("sell"), "goods", unit="paragraph", ordered=True)]),
                  Terms(all_of=["goods"], none_of=[Within("buyer", "seller", unit="paragraph")])):
            ids = ids_of(docs, t)
            got = r.search(q, top_k=TOP_K, terms=t)
            same(got, r.search(q, top_k=TOP_K, scope=Scope(chunk_ids=ids)))  # ids and score bits of the scoped search over the rows
            assert len(got) == min(TOP_K, len(ids)) > 0, t
            assert all(t.matches(*by_id[h.chunk.id]) for h in got)
    t = Terms(all_of=[Within("buyer", "seller")])
    ids = ids_of(docs, t)
    out = r.search_batch([QUESTIONS[0], QUESTIONS[1]], top_k=TOP_K, terms=[t, None])
    same(out[0], r.search(QUESTIONS[0], top_k=TOP_K, terms=t))
    same(out[1], r.search(QUESTIONS[1], top_k=TOP_K))
    for fn in (r.search_dense, r.search_bm25, r.search_colbert):  # the per-channel searches: the host twins
        same(fn(QUESTIONS[0], TOP_K, terms=t), fn(QUESTIONS[0], TOP_K, scope=Scope(chunk_ids=ids)))


def test_highlight_marks_the_members_of_a_within(live):
    from legal_rag_amd.retrieval.highlight import Highlight
    from legal_rag_amd.retrieval.terms import Terms, Within
    cfg, r = live
    t = Terms(all_of=[Within("buyer", "seller")])
    hits = r.search(QUESTIONS[0], top_k=5, terms=t)
    hls = r.highlight(QUESTIONS[0], hits, terms=t, spec=Highlight(question=False))
    assert len(hls) == len(hits) == 5
    for h, hl in zip(hits, hls):
        assert hl is not None and set(hl.found) == {"buyer", "seller"} and not hl.missing
        assert {m.label for m in hl.marks} <= {"buyer", "seller"} and hl.marks
        assert all(h.chunk.text[m.char_start:m.char_end].lower() == m.label for m in hl.marks)


def test_a_live_add_remove_and_replace_under_carry_cut_only_the_new_chunks(tmp_path):
    from legal_rag_amd.retrieval.builders.remove import remove_chunk_ids
    from legal_rag_amd.retrieval.builders.replace import replace_chunks
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from legal_rag_amd.retrieval.terms import Terms, Within
    from test_tok_carry_api_gpu import _build, _cfg, _ingest, _jsonl
    every = ucc_chunks()
    t = Terms(all_of=[Within("buyer", "seller")])
    holders = [c for c in every if "buyer" in c.text.lower() and "seller" in c.text.lower()]
    chunks = list({c.id: c for c in holders[:30] + every[:24]}.values())
    more = [c for c in holders[30:] if c.id not in {x.id for x in chunks}][:3]
    cfg = _cfg(tmp_path / "live", token_stream="carry")
    _build(cfg, chunks, tmp_path / "all.jsonl")
    r = HybridRetriever(cfg)
    n0 = r.count(terms=t)
    ids0 = ids_of(cut(r), t)
    assert n0 == len(ids0) > 5 and sorted(r.bm25.breaks_cut) == sorted(c.id for c in chunks)  # the first call cuts every chunk
    native = r.bm25.gpu_index()
    assert native.breaks_info()[0] and r.count(terms=t) == n0 and sorted(r.bm25.breaks_cut) == sorted(c.id for c in chunks)

    # a replacement whose text loses its match: the old entry of that chunk must not be reused
    victim = next(c for c in r.bm25.chunks if c.id == ids0[0])
    amended = victim.model_copy(update={"text": victim.text.replace("seller", "vendor").replace("Seller", "Vendor")})
    assert replace_chunks(cfg, _jsonl(tmp_path / "amend.jsonl", [amended])) == {"bm25": 1, "dense": 1, "colbert": 1}
    assert r.bm25.gpu_index() is native and native.tokens_info()[0] and not native.breaks_info()[0]  # the stream kept, the flags gone
    assert r.count(terms=t) == n0 - 1 == len(ids_of(cut(r), t)) and victim.id not in ids_of(cut(r), t)
    assert r.bm25.breaks_cut == [victim.id] and native.breaks_info()[0]
    assert (victim.id, victim.text) not in r.bm25._break_cache and (victim.id, amended.text) in r.bm25._break_cache
    assert len(r.bm25._break_cache) == len(chunks)

    # an ingest of three further holders
    assert _ingest(cfg, _jsonl(tmp_path / "more.jsonl", more)) == (3, 3, 3)
    assert native.tokens_info()[0] and not native.breaks_info()[0]
    grown = ids_of(cut(r), t)
    assert r.count(terms=t) == len(grown) and len(grown) >= n0 - 1 and sorted(r.bm25.breaks_cut) == sorted(c.id for c in more)

    # a removal of a holder: nothing is cut
    gone = grown[0]
    assert remove_chunk_ids(cfg, [gone]) == {"bm25": 1, "dense": 1, "colbert": 1}
    assert not native.breaks_info()[0]
    left = ids_of(cut(r), t)
    assert r.count(terms=t) == len(left) == len(grown) - 1 and gone not in left and r.bm25.breaks_cut == []
    assert len(r.bm25._break_cache) == len(chunks) + 3 - 1
    assert np.array_equal(native.read_breaks(), np.concatenate([np.asarray(b, np.uint8) for _, _, b in cut(r)]))


def test_a_row_sharded_retriever_raises(live, monkeypatch):
    from legal_rag_amd.retrieval.terms import Terms, Within
    cfg, r = live
    t = Terms(all_of=[Within("buyer", "seller")])
    assert r.count(terms=t) > 0
    monkeypatch.setattr(r.bm25, "shard", object(), raising=False)
    with pytest.raises(ValueError, match="row-sharded"):
        r.bm25.ensure_breaks()
    for call in (lambda: r.count(terms=t), lambda: r.search(QUESTIONS[0], terms=t), lambda: r.search_bm25(QUESTIONS[0], 5, terms=t)):
        with pytest.raises(ValueError, match="row-sharded"):
            call()

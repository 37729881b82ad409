"""Proximity constraints without a GPU: the certificates of tests/near_cases.py, `Near` and `Terms` typing and hashing, the
packer (Nears stored once, virtual ids behind the phrases, both bounds, a table without a Near unchanged), `matches` on
token sequences, the refusals before a launch and the plan arithmetic (amdr_span_lists_plan)."""
import dataclasses
import pickle
from types import SimpleNamespace

import numpy as np
import pytest

import near_cases as NC
import phrase_cases as PC
from legal_rag_amd.retrieval.scope import Scope
from legal_rag_amd.retrieval.terms import ANY, MUST, NOT, Near, Phrase, Terms, pack


# ---- the certificates --------------------------------------------------------------------------------------------------
def test_edge_corpus_certificates():
    corpus, at = NC.edge_corpus()
    NC.edge_certificates(corpus, at)
    ptr, tokens = corpus.stream()
    assert ptr[-1] == tokens.size == sum(len(s) for s in corpus.docs) and np.array_equal(np.diff(ptr), corpus.postings()[4])
    assert all(0 <= t < corpus.n_terms for s in corpus.docs for t in s) and not corpus.holders(NC.NONE)


def test_tiles_corpus_certificates():
    NC.tiles_certificates(PC.tiles_corpus())


def test_rand_corpus_and_constraint_certificates():
    corpus = PC.rand_corpus()
    NC.rand_certificates(corpus, NC.rand_items(corpus))
    items = NC.scope_items(corpus)
    NC.scope_certificates(corpus, NC.scope_family(corpus), items)


def test_reference_scan_on_written_out_cases():
    h = NC.near_holds
    assert h([1, 9, 2], [1, 2], 2, False) and h([2, 9, 1], [1, 2], 2, False) and not h([1, 9, 2], [1, 2], 1, False)
    assert h([1, 9, 2], [1, 2], 2, True) and not h([2, 9, 1], [1, 2], 2, True)
    assert not h([1], [1, 1], 5, False) and h([1, 1], [1, 1], 1, False) and h([1, 1], [1, 1], 1, True)
    assert not h([], [1, 2], 255, False) and not h([1, 2], [1, 2, 2], 255, False)
    for seq, terms, n in (([0, 0, 1], [0, 1], 1), ([0, 3, 3, 1, 0], [0, 1], 1), ([1, 0, 1, 0], [0, 1, 0], 2), ([0, 1, 0, 1], [0, 0, 1], 2)):
        for o in (False, True):
            assert h(seq, terms, n, o) == NC.near_holds_tuples(seq, terms, n, o)


def test_the_two_identities_hold_on_the_reference():
    corpus = PC.rand_corpus()
    longest = max(len(s) for s in corpus.docs)
    assert longest <= NC.MAX_DIST
    for terms in NC.identity_terms(corpus):
        assert len(set(terms)) == len(terms)
        assert np.array_equal(NC.item_list(corpus, NC.near(terms, NC.MAX_DIST)), PC.conjunction(corpus, terms))
        if len(terms) == 2:
            assert np.array_equal(NC.item_list(corpus, NC.near(terms, 1, True)), PC.phrase_list(corpus, terms))


# ---- Near and Terms ----------------------------------------------------------------------------------------------------
def test_near_is_frozen_hashable_picklable_and_bounded():
    n = Near("buyer", "seller", distance=5)
    assert n == Near("buyer", "seller", distance=5) and hash(n) == hash(Near("buyer", "seller", distance=5, ordered=False))
    assert n != Near("seller", "buyer", distance=5) and n != Near("buyer", "seller", distance=6)
    assert n != Near("buyer", "seller", distance=5, ordered=True) and n != Phrase("buyer", "seller") and n != ("buyer", "seller")
    assert n.tokens == ("buyer", "seller") and n.distance == 5 and n.ordered is False and len(n) == 2
    assert repr(n) == "Near('buyer', 'seller', distance=5)"
    assert repr(Near("a", "b", distance=1, ordered=True)) == "Near('a', 'b', distance=1, ordered=True)"
    for x in (n, Near("a", "a", "b", distance=255, ordered=True)):
        assert pickle.loads(pickle.dumps(x)) == x and hash(pickle.loads(pickle.dumps(x))) == hash(x)
    assert {n: 1}[Near("buyer", "seller", distance=5)] == 1
    for attr in ("tokens", "distance", "ordered"):
        with pytest.raises(AttributeError):
            setattr(n, attr, 1)
    with pytest.raises(ValueError, match="2 to 8"):
        Near("a", distance=3)
    with pytest.raises(ValueError, match="2 to 8"):
        Near(*["t"] * 9, distance=3)
    assert len(Near(*["t"] * 8, distance=3)) == 8
    for bad in (0, 256, -1):
        with pytest.raises(ValueError, match="1 to 255"):
            Near("a", "b", distance=bad)
    assert Near("a", "b", distance=1).distance == 1 and Near("a", "b", distance=255).distance == 255
    with pytest.raises(TypeError):
        Near("a", 3, distance=2)
    with pytest.raises(TypeError):
        Near("a", "b", distance=2.0)
    with pytest.raises(TypeError):
        Near("a", "b")  # the distance has no default


def test_within_applies_the_rule_to_a_token_sequence():
    w = lambda near, text: near.within(text.split())  # noqa: E731
    assert w(Near("a", "b", distance=2), "a x b") and w(Near("a", "b", distance=2), "b x a")
    assert not w(Near("a", "b", distance=1), "a x b") and not w(Near("a", "b", distance=2, ordered=True), "b x a")
    assert w(Near("a", "b", distance=1, ordered=True), "a a b") and w(Near("a", "b", distance=1), "a x x b a")
    assert not w(Near("a", "a", distance=3), "a x") and w(Near("a", "a", distance=2), "a x a")
    assert not w(Near("a", "a", distance=2), "a x x a") and not w(Near("a", "a", "b", distance=4), "a b")
    assert w(Near("a", "b", "a", distance=2, ordered=True), "a b a") and not w(Near("a", "b", "a", distance=3, ordered=True), "a a b")
    assert not w(Near("a", "b", distance=5), "") and w(Near("a", "b", distance=255), "x x a b")
    corpus, _ = NC.edge_corpus()  # and against the window scan, item by item, document by document
    name = [f"t{t}" for t in range(corpus.n_terms)]
    for kind, terms, n in NC.edge_items():
        if all(0 <= t < corpus.n_terms for t in terms):
            near = Near(*[name[t] for t in terms], distance=n, ordered=kind == NC.ORDERED)
            got = [d for d, seq in enumerate(corpus.docs) if len(seq) < 200 and near.within([name[t] for t in seq])]
            want = [int(d) for d in NC.item_list(corpus, (kind, terms, n)) if len(corpus.docs[d]) < 200]
            assert got == want, near


def test_terms_take_a_near_wherever_a_token_stands():
    n, p = Near("a", "b", distance=3), Phrase("a", "b")
    t = Terms(all_of=[n, ("c", n, p)], any_of=n, none_of=[Near("b", "a", distance=1, ordered=True)])
    assert t.all_of == ((n,), ("c", n, p)) and t.any_of == ((n,),) and t.has_near and t.has_phrase
    assert t.none_of == ((Near("b", "a", distance=1, ordered=True),),)
    same = Terms(all_of=[Near("a", "b", distance=3), ("c", Near("a", "b", distance=3), Phrase("a", "b"))],
                 any_of=[Near("a", "b", distance=3)], none_of=Near("b", "a", distance=1, ordered=True))
    assert t == same and hash(t) == hash(same)
    assert t != Terms(all_of=[p, ("c", p, p)], any_of=p, none_of=[Near("b", "a", distance=1, ordered=True)])
    assert Terms(all_of=[n]) != Terms(all_of=[("a", "b")]) and not Terms(all_of=[p]).has_near and not Terms(all_of="a").has_near
    assert t.groups()[:3] == [(MUST, (n,)), (MUST, ("c", n, p)), (ANY, (n,))] and t.groups()[3][0] == NOT
    assert pickle.loads(pickle.dumps(t)) == t


def test_matches_takes_a_sequence_when_a_near_is_present():
    t = Terms(all_of=[Near("a", "b", distance=2)], none_of=[Near("b", "a", distance=2, ordered=True)])
    assert t.matches(["x", "a", "x", "b"]) and t.matches(("a", "b"))
    assert not t.matches(["b", "x", "a"]) and not t.matches(["a", "x", "x", "b"]) and not t.matches([])
    assert Terms(all_of=[("c", Near("a", "a", distance=1))]).matches(["a", "a", "x", "x", "c"])
    assert not Terms(all_of=[("c", Near("a", "a", distance=1))]).matches(["a", "c", "a"])
    assert Terms(any_of=[Near("a", "b", distance=1), "z"]).matches(["z"])
    for bad in ({"a", "b"}, frozenset(["a", "b"]), {"a": 1, "b": 1}):
        with pytest.raises(TypeError, match="sequence"):
            t.matches(bad)


# ---- the packer ------------------------------------------------------------------------------------------------------------
VOCAB = {"a": 0, "b": 1, "c": 2, "d": 3}
DF = {"a": 50, "b": 30, "c": 90, "d": 9}


def test_pack_stores_equal_nears_once_behind_the_phrases_with_both_bounds():
    ab, ab_o, cz = Near("a", "b", distance=5), Near("a", "b", distance=5, ordered=True), Near("c", "zzz", "c", distance=9)
    ph, ph2 = Phrase("b", "a"), Phrase("c", "d")
    # the Nears come first in the pairs, the second phrase last: the Nears' ids still stand behind BOTH phrases
    pairs = [(None, Terms(all_of=[ab])), (None, Terms(all_of=[("c", ab_o)], none_of=[ph])), (None, Terms(any_of=[ab, cz])),
             (None, Terms(all_of=[ab])), (None, Terms(all_of=["d", Near("a", "b", distance=5)])), (None, Terms(all_of=[cz, ph2]))]
    tt = pack(pairs, VOCAB, DF, 100)
    V = len(VOCAB)
    assert tt.phrases == (ph, ph2) and tt.nears == (ab, ab_o, cz) and (tt.n_phr, tt.n_near) == (2, 3)
    N = V + 2  # the first Near's id
    assert tt.qscope.tolist() == [0, 1, 2, 0, 3, 4] and tt.n_cons == 5
    assert tt.ops[3].tolist() == [N + 0, 2, N + 1, V + 0, N + 0, N + 2, 3, N + 0, N + 2, V + 1]
    assert tt.ops[0].tolist() == [0, 1, 3, 5, 7, 9] and tt.ops[2].tolist() == [0, 1, 3, 4, 5, 6, 7, 8, 9, 10]
    # the phrase fields are the phrases' alone; span_ops holds the one step's items: the phrases as kind 0, then the Nears
    assert tt.phr_ops[0].tolist() == [0, 2, 4] and tt.phr_ops[1].tolist() == [1, 0, 2, 3]
    ptr, terms, kind, dist = tt.span_ops
    assert ptr.tolist() == [0, 2, 4, 6, 8, 11] and terms.tolist() == [1, 0, 2, 3, 0, 1, 0, 1, 2, -1, 2]
    assert kind.tolist() == [0, 0, 1, 2, 1] and dist.tolist() == [0, 0, 5, 5, 9]
    assert ptr.dtype == np.int64 and terms.dtype == kind.dtype == dist.dtype == np.int32
    # the upper bound of a Near: the smallest document frequency among its tokens; 0 with an unknown one
    assert (tt.near_cand_max, tt.near_rows_cap) == (30, 30 + 30 + 0) and (tt.phr_cand_max, tt.phr_rows_cap) == (30, 30 + 9)
    assert (tt.span_cand_max, tt.span_rows_cap) == (30, 99)
    assert [tt.span_item(i) for i in range(5)] == [ph, ph2, ab, ab_o, cz]
    # the drivers: the Near's bound; min(c, the bound); no MUST: the corpus; "d" is rarer than the bound; an unknown token
    assert tt.driver_lens.tolist() == [30, 30, 100, 9, 0] and (tt.cand_max, tt.rows_cap) == (100, 169)


def test_a_table_without_a_near_is_what_it_was():
    pairs = [(None, Terms(all_of=[Phrase("a", "b")])), (None, Terms(all_of=["c"], none_of=[Phrase("b", "a")]))]
    tt = pack(pairs, VOCAB, DF, 100)
    assert (tt.n_near, tt.nears, tt.near_cand_max, tt.near_rows_cap) == (0, (), 0, 0)
    assert [x.tolist() for x in tt.span_ops] == [[0], [], [], []]
    assert tt.phr_ops[0].tolist() == [0, 2, 4] and tt.ops[3].tolist() == [4, 2, 5] and tt.driver_lens.tolist() == [30, 90]
    new = {"span_ops", "nears", "near_cand_max", "near_rows_cap"}
    names = [f.name for f in dataclasses.fields(tt)]
    assert names[-4:] == ["span_ops", "nears", "near_cand_max", "near_rows_cap"]  # behind the fields there were, defaulted
    assert all(f.default is not dataclasses.MISSING for f in dataclasses.fields(tt) if f.name in new)
    with_near = pack(pairs + [(None, Terms(any_of=[Near("a", "d", distance=2)]))], VOCAB, DF, 100)
    for f in ("phr_ops", "phrases", "phr_cand_max", "phr_rows_cap"):  # a Near changes no phrase field
        a, b = getattr(tt, f), getattr(with_near, f)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) if f == "phr_ops" else a == b


def test_pack_with_a_base_scope_and_a_near():
    s = Scope(section="S")
    tt = pack([(s, Terms(all_of=[Near("a", "b", distance=2)]))], VOCAB, DF, 100, lambda sc: np.arange(7, dtype=np.int64))
    assert tt.driver_lens.tolist() == [7] and tt.n_base == 1 and tt.near_cand_max == 30 and tt.n_phr == 0


# ---- the refusals of §4.17 carry over --------------------------------------------------------------------------------------
def retriever(monkeypatch, native):
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    r = HybridRetriever.__new__(HybridRetriever)
    r.cfg = SimpleNamespace(retrieval=SimpleNamespace(top_k=10))
    monkeypatch.setattr(HybridRetriever, "_native_channels", lambda self, eff: native)
    monkeypatch.setattr(HybridRetriever, "_diversity", lambda self, *a: None)

    def no_launch(*a, **k):
        raise AssertionError("a launch was attempted")
    monkeypatch.setattr(HybridRetriever, "_prepare", no_launch)
    monkeypatch.setattr(HybridRetriever, "_run", no_launch)
    return r


def plain_native(**over):
    chunks = [SimpleNamespace(id=f"c{j}", law_name="L", chapter="C", section="S", article_id=str(j)) for j in range(4)]
    store = SimpleNamespace(chunks=chunks, index=SimpleNamespace(spec=over.get("dense_spec")))
    return store, SimpleNamespace(shard=over.get("bm25_shard"), chunks=chunks), None


def test_nears_are_refused_where_terms_are(monkeypatch):
    t = Terms(all_of=[Near("buyer", "seller", distance=5)])
    r = retriever(monkeypatch, plain_native())
    graph = SimpleNamespace(mode="GRAPH_AUGMENTED")
    with pytest.raises(ValueError, match="graph-mode decision and term constraints"):
        r.search("q", terms=t, decision=graph)
    for over in ({"dense_spec": object()}, {"bm25_shard": object()}):
        r = retriever(monkeypatch, plain_native(**over))
        for call in (lambda: r.search_batch(["q"], terms=[t]), lambda: r.search_batch_arrays(["q"], terms=[t]),
                     lambda: r.search("q", terms=t)):
            with pytest.raises(ValueError, match="row-sharded"):
                call()
    r = retriever(monkeypatch, None)
    with pytest.raises(ValueError, match="one chunk list"):
        r.search("q", terms=t)


def test_near_cuts_a_string_with_the_document_side_tokeniser(tmp_path):
    from legal_rag_amd.retrieval.bm25_retriever import BM25Retriever
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    bm = BM25Retriever.__new__(BM25Retriever)
    bm.cfg = SimpleNamespace(retrieval=SimpleNamespace())
    bm.bm25_path = tmp_path / "bm25.pkl"
    bm.load = lambda: None
    bm.index_tokenizer = "en_regex"
    r = HybridRetriever.__new__(HybridRetriever)
    r.bm25 = bm
    assert r.near("Buyer Seller", distance=5) == Near("buyer", "seller", distance=5)
    assert r.near("Holder  DUE course", distance=5, ordered=True) == Near("holder", "due", "course", distance=5, ordered=True)
    assert r.near("goods goods", 5) == Near("goods", "goods", distance=5)
    with pytest.raises(ValueError, match="2 to 8"):
        r.near("buyer", distance=5)
    with pytest.raises(ValueError, match="2 to 8"):
        r.near(" ".join(["w"] * 9), distance=5)
    with pytest.raises(ValueError, match="1 to 255"):
        r.near("buyer seller", distance=0)
    bm.index_tokenizer = None  # a reference rank_bm25 pickle records no tokeniser
    with pytest.raises(ValueError, match="records no tokenizer"):
        r.near("buyer seller", distance=5)
    r.bm25 = object()
    with pytest.raises(ValueError, match="own BM25 retriever"):
        r.near("buyer seller", distance=5)


# ---- the plan --------------------------------------------------------------------------------------------------------------
def test_plan_arithmetic_and_null_handles():
    from legal_rag_amd import _native
    assert (_native.NEAR_MAX_TERMS, _native.NEAR_MAX_DIST) == (NC.MAX_TERMS, NC.MAX_DIST)
    assert (_native.SPAN_PHRASE, _native.SPAN_NEAR_UNORDERED, _native.SPAN_NEAR_ORDERED) == (NC.PHRASE, NC.UNORDERED, NC.ORDERED)
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for n in (1, 2, 65, 1168, 70_000):
        for cand_max in (0, 1, 255, 256, 257, 513, 4100):
            cells = n * max(1, -(-cand_max // _native.PHRASE_TILE))
            assert _native.span_lists_plan(n, cand_max) == up(8 * cells) + up(8 * (cells + 1)) + up(1024 * cells)
            assert _native.span_lists_plan(n, cand_max) == _native.phrase_lists_plan(n, cand_max)  # the phrase plan's arithmetic
    assert _native.span_lists_plan(0, 0) >= 0
    for bad in ((-1, 10), (1, -1), (1, 65_536 * 256)):
        with pytest.raises(_native.NativeError):
            _native.span_lists_plan(*bad)
    lib = _native.load()  # a null handle is refused before any device is touched
    assert lib.amdr_span_lists_device(None, None, None, None, None, 1, 0, 0, None, None, None, None, 0, None) == -1
    assert b"null handle" in lib.amdr_last_error()
    assert lib.amdr_span_lists(None, None, None, None, None, 1, 0, 0, None, None, None) == -1
    assert b"null handle" in lib.amdr_last_error()

"""The root expander and alternatives without a GPU: the certificates of tests/union_cases.py, `Prefix` and `OneOf` typing,
hashing and pickling, `Terms.matches` with both, the packer (bisection against a brute-force startswith, equal unions stored
once, the single-id and empty cases, the cap, ids behind the phrases and the Nears, the bounds, a table without a union
unchanged), `BM25Okapi.sorted_vocab()` across live updates, `retriever.prefix()`, and the plan arithmetic
(amdr_union_lists_plan)."""
import dataclasses
import pickle
from types import SimpleNamespace

import numpy as np
import pytest

import phrase_cases as PC
import union_cases as UC
from legal_rag_amd.retrieval.scope import Scope
from legal_rag_amd.retrieval.terms import (ANY, MUST, NOT, PREFIX_MAX_TERMS, Near, OneOf, Phrase, Prefix, Terms, pack,
                                           prefix_tokens)

# tokens that are prefixes of each other, and non-ASCII ones (code-point order is not byte order across planes)
VOCAB_TOKENS = ["sell", "seller", "seller's", "selling", "sells", "sel", "se", "self", "buyer", "buy", "buys", "buying",
                "purchaser", "goods", "merchandise", "zebra", "é", "école", "écoles", "eco", "合", "合同", "合同法", "同",
                "\U0001f600x", "￿y", "a", "b", "c", "d"]
VOCAB = {w: i for i, w in enumerate(VOCAB_TOKENS)}
DF = {w: 3 + 2 * i for i, w in enumerate(VOCAB_TOKENS)}
N_DOCS = 100


@pytest.fixture(scope="module")
def tile():
    from legal_rag_amd import _native
    return _native.UNION_TILE


# ---- the certificates --------------------------------------------------------------------------------------------------
def test_edge_corpora_certificates(tile):
    assert tile == 32768
    for n in UC.edge_sizes(tile):
        corpus = UC.edge_corpus(n, tile)
        UC.edge_certificates(corpus, tile)
        tp, pd = corpus.postings()[:2]
        assert tp[-1] == pd.size and all(np.all(np.diff(pd[tp[t]:tp[t + 1]]) > 0) for t in range(0, corpus.n_terms, 37))
    for n in (tile + 1, 3 * tile + 1):  # merged, not concatenated, where a list crosses tiles
        corpus = UC.edge_corpus(n, tile)
        item, df = UC.edge_items(corpus)["overlapping"], corpus.df()
        assert max(df[t] for t in item) < UC.item_list(corpus, item).size < sum(df[t] for t in item)
    assert [len(b) for b in (UC.batch(UC.edge_corpus(33, tile), k) for k in (1, 2, 65))] == [1, 2, 65]


def test_rand_corpus_and_constraint_certificates():
    corpus = PC.rand_corpus()
    phrases, unions = UC.scope_lists(corpus)
    UC.scope_certificates(corpus, UC.scope_family(corpus), phrases, unions)


def test_reference_on_written_out_cases():
    corpus = PC.SeqCorpus("small", 4, [[0, 1], [1], [], [2, 0], [3]])
    assert UC.item_list(corpus, [0, 1]).tolist() == [0, 1, 3] and UC.item_list(corpus, [3, 3]).tolist() == [4]
    assert UC.item_list(corpus, []).size == 0 and UC.item_list(corpus, [-1, 4]).size == 0
    assert UC.item_list(corpus, [-1, 2, 9]).tolist() == [3]
    ptr, docs = UC.expected_lists(corpus, [[0, 1], [], [2]], before=(np.asarray([0, 2]), np.asarray([7, 8], np.int32)))
    assert ptr.tolist() == [0, 2, 5, 5, 6] and docs.tolist() == [7, 8, 0, 1, 3, 3]
    assert UC.upper_bound(corpus, [0, 1, 1, -1]) == 4 and UC.upper_bound(corpus, [0, 1, 2, 3]) == 5  # min(n_docs, 2 + 2 + 1 + 1)


# ---- Prefix and OneOf ----------------------------------------------------------------------------------------------------
def test_prefix_and_oneof_are_frozen_hashable_picklable_and_validated():
    p, o = Prefix("sell"), OneOf("buyer", Prefix("purchas"))
    assert p == Prefix("sell") and hash(p) == hash(Prefix("sell")) and p != Prefix("sel") and p != "sell"
    assert o == OneOf("buyer", Prefix("purchas")) and hash(o) == hash(OneOf("buyer", Prefix("purchas")))
    assert o != OneOf(Prefix("purchas"), "buyer") and len({p, Prefix("sell"), o, OneOf("buyer", Prefix("purchas"))}) == 2
    assert repr(p) == "Prefix('sell')" and repr(o) == "OneOf('buyer', Prefix('purchas'))" and len(o) == 2
    for x in (p, o, Terms(all_of=[(o, p)], none_of=[Prefix("leas")])):
        assert pickle.loads(pickle.dumps(x)) == x and hash(pickle.loads(pickle.dumps(x))) == hash(x)
    for obj, name in ((p, "stem"), (o, "members")):
        with pytest.raises(AttributeError):
            setattr(obj, name, "x")
        with pytest.raises(AttributeError):
            delattr(obj, name)
    with pytest.raises(ValueError):
        Prefix("")
    for bad in (None, 3, b"sell", ("sell",)):
        with pytest.raises(TypeError):
            Prefix(bad)
    with pytest.raises(ValueError):
        OneOf()
    for bad in (Phrase("a", "b"), Near("a", "b", distance=2), OneOf("a", "b"), 3, None):
        with pytest.raises(TypeError):
            OneOf("x", bad)
    # not inside a Phrase or a Near: those keep their TypeError
    for make in (lambda: Phrase("a", p), lambda: Phrase(o, "a"), lambda: Near("a", p, distance=2), lambda: Near(o, "b", distance=2)):
        with pytest.raises(TypeError):
            make()


def test_terms_take_both_wherever_a_token_stands():
    p, o = Prefix("sell"), OneOf("buyer", "purchaser")
    t = Terms(all_of=[p, (o, "goods")], any_of=o, none_of=[(p, Phrase("a", "b"), Near("a", "b", distance=3))])
    assert t.all_of == ((p,), (o, "goods")) and t.any_of == ((o,),) and t.none_of[0][0] is p
    assert t.has_union and t.has_phrase and t.has_near and not Terms(all_of=["a", Phrase("a", "b")]).has_union
    assert Terms(any_of=[OneOf("x")]).any_of == (("x",),) and not Terms(any_of=[OneOf("x")]).has_union  # the plain term
    assert Terms(all_of=[OneOf(Prefix("x"))]).all_of == ((Prefix("x"),),)
    assert t == Terms(all_of=[p, (o, "goods")], any_of=[o], none_of=[(p, Phrase("a", "b"), Near("a", "b", distance=3))])
    assert [k for k, _ in t.groups()] == [MUST, MUST, ANY, NOT]


def test_matches_and_within_on_sets_and_sequences():
    p, o = Prefix("sell"), OneOf("buyer", Prefix("purchas"))
    assert p.within(["the", "seller's", "goods"]) and p.within({"sells"}) and not p.within(["sel", "resell"]) and not p.within([])
    assert o.within({"purchaser"}) and o.within(["x", "buyer"]) and not o.within(["buy", "purchas"[:-1]])
    t = Terms(all_of=[(o, p)], none_of=[Prefix("leas")])
    assert t.matches({"buyer", "selling"}) and t.matches(["a", "purchases", "sell"])
    assert not t.matches({"buyer", "goods"}) and not t.matches({"buyer", "sells", "lease"}) and not t.matches(["seller"])
    assert Terms(any_of=[p, "x"]).matches({"x"}) and not Terms(any_of=[p, "x"]).matches({"y"})
    seq = ["the", "buyer", "sells", "goods"]
    mixed = Terms(all_of=[(p, Phrase("sells", "goods"), Near("buyer", "goods", distance=2))])
    assert mixed.matches(seq) and not mixed.matches(seq[:3])
    with pytest.raises(TypeError):
        mixed.matches(set(seq))


# ---- the packer ----------------------------------------------------------------------------------------------------------
def test_bisection_equals_a_brute_force_startswith():
    sv = sorted(VOCAB)
    stems = ["sell", "sel", "se", "s", "seller", "seller's", "sellers", "buy", "é", "éc", "école", "合", "合同", "合同法", "同",
             "\U0001f600", "￿", "z", "zz", "a", "e", "\U0010ffff", " "]
    for stem in stems:
        brute = sorted(w for w in VOCAB if w.startswith(stem))
        assert prefix_tokens(stem, sv) == brute, stem
        tt = pack([(None, Terms(all_of=[Prefix(stem)]))], VOCAB, DF, 10_000)
        ids = sorted(VOCAB[w] for w in brute)
        if len(ids) >= 2:
            assert tt.n_union == 1 and tt.union_ops[1].tolist() == ids and tt.ops[3].tolist() == [len(VOCAB)], stem
        else:
            assert tt.n_union == 0 and tt.ops[3].tolist() == (ids or [-1]), stem
    assert len(prefix_tokens("sell", sv)) == 5 and len(prefix_tokens("合", sv)) == 3
    # a sorted vocabulary handed in is the one used; computed from `vocab` otherwise
    a = pack([(None, Terms(all_of=[Prefix("sell")]))], VOCAB, DF, N_DOCS, sorted_vocab=sv)
    b = pack([(None, Terms(all_of=[Prefix("sell")]))], VOCAB, DF, N_DOCS)
    assert a.union_ops[1].tolist() == b.union_ops[1].tolist() == sorted(VOCAB[w] for w in VOCAB if w.startswith("sell"))


def test_equal_unions_are_stored_once_and_single_or_empty_ones_are_plain_ids():
    V = len(VOCAB)
    sell = [w for w in VOCAB if w.startswith("sell")]
    p, o = Prefix("sell"), OneOf(*reversed(sell))
    pairs = [(None, Terms(all_of=[p])), (None, Terms(any_of=[o, "a"])), (None, Terms(all_of=[(OneOf("buyer", "purchaser"), p)])),
             (None, Terms(all_of=[OneOf("sells", "sell", "sells", Prefix("sell"), "nowhere")])),  # the same set again
             (None, Terms(all_of=[Prefix("zeb")])), (None, Terms(all_of=[Prefix("nope")], none_of=[OneOf("nope", "nix")])),
             (None, Terms(any_of=[OneOf("a", "nope")]))]
    tt = pack(pairs, VOCAB, DF, N_DOCS)
    sell_ids = sorted(VOCAB[w] for w in sell)
    assert tt.n_union == 2 and tt.unions == (p, OneOf("buyer", "purchaser"))
    assert tt.union_ops[0].tolist() == [0, 5, 7] and tt.union_ops[1].tolist() == sell_ids + sorted([VOCAB["buyer"], VOCAB["purchaser"]])
    assert tt.union_ops[0].dtype == np.int64 and tt.union_ops[1].dtype == np.int32
    assert tt.ops[3].tolist() == [V, V, VOCAB["a"], V + 1, V, V, VOCAB["zebra"], -1, -1, VOCAB["a"]]
    # the bound: min(n_docs, the sum of the distinct known ids' document frequencies)
    ub = [min(N_DOCS, sum(DF[w] for w in sell)), min(N_DOCS, DF["buyer"] + DF["purchaser"])]
    assert tt.union_rows_cap == sum(ub) and ub[0] == 3 + 5 + 7 + 9 + 11 and ub[1] < N_DOCS
    # drivers: the union's bound; no MUST; the smaller of the two bounds; the bound; zebra's df; an unknown MUST; no MUST
    assert tt.driver_lens.tolist() == [ub[0], N_DOCS, min(ub), ub[0], DF["zebra"], 0, N_DOCS]
    assert pack([(None, Terms(all_of=[Prefix("s")]))], VOCAB, DF, 20).union_rows_cap == 20  # never more than the corpus


def test_a_member_of_more_than_the_cap_is_refused_by_name():
    big = {f"w{i:05d}": i for i in range(PREFIX_MAX_TERMS)}
    big["wx"] = PREFIX_MAX_TERMS
    df = dict.fromkeys(big, 1)
    with pytest.raises(ValueError, match=r"Prefix\('w'\) names 4097 vocabulary tokens"):
        pack([(None, Terms(all_of=[Prefix("w")]))], big, df, 10_000)
    with pytest.raises(ValueError, match=r"OneOf\('x', Prefix\('w'\)\) names 4097"):
        pack([(None, Terms(any_of=[OneOf("x", Prefix("w"))]))], big, df, 10_000)
    ok = pack([(None, Terms(all_of=[Prefix("w0")]))], big, df, 10_000)  # exactly 4 096 tokens: w00000 .. w04095
    assert ok.n_union == 1 and ok.union_ops[1].size == PREFIX_MAX_TERMS == 4096 and ok.union_rows_cap == 4096


def test_union_ids_stand_behind_the_phrases_and_the_nears():
    V = len(VOCAB)
    ph, nr, p, o = Phrase("a", "b"), Near("c", "d", distance=4), Prefix("buy"), OneOf("goods", "merchandise")
    # the unions come first in the pairs: their ids still stand behind the phrase and the Near
    pairs = [(None, Terms(all_of=[p], none_of=[o])), (None, Terms(all_of=[(o, ph, nr)])), (None, Terms(any_of=[nr, p]))]
    tt = pack(pairs, VOCAB, DF, N_DOCS)
    assert (tt.n_phr, tt.n_near, tt.n_union) == (1, 1, 2) and tt.unions == (p, o)
    U = V + 2
    assert tt.ops[3].tolist() == [U + 0, U + 1, U + 1, V + 0, V + 1, V + 1, U + 0]
    assert [tt.list_item(i) for i in range(4)] == [ph, nr, p, o] and [tt.span_item(i) for i in range(2)] == [ph, nr]
    buy = min(N_DOCS, sum(DF[w] for w in VOCAB if w.startswith("buy")))
    goods = min(N_DOCS, DF["goods"] + DF["merchandise"])
    near_ub, phr_ub = min(DF["c"], DF["d"]), min(DF["a"], DF["b"])
    assert tt.driver_lens.tolist() == [buy, min(goods, phr_ub, near_ub), N_DOCS]
    assert tt.span_rows_cap == near_ub + phr_ub and tt.union_rows_cap == buy + goods


def test_a_table_without_a_union_is_what_it_was():
    pairs = [(None, Terms(all_of=[Phrase("a", "b")])), (None, Terms(all_of=["c"], none_of=[Near("b", "a", distance=3)])),
             (Scope(section="S"), Terms(any_of=[("a", "d")]))]
    rows = lambda sc: np.arange(7, dtype=np.int64)  # noqa: E731
    tt = pack(pairs, VOCAB, DF, N_DOCS, rows)
    assert (tt.n_union, tt.unions, tt.union_rows_cap) == (0, (), 0) and [x.tolist() for x in tt.union_ops] == [[0], []]
    assert not {"union_ops", "unions", "union_rows_cap"} & {f.name for f in dataclasses.fields(tt)}  # the fields are today's
    # a union beside them changes no field of the constraints it does not stand in, and no phrase or Near field
    more = pack(pairs + [(None, Terms(all_of=[Prefix("sell")]))], VOCAB, DF, N_DOCS, rows, sorted(VOCAB))
    for f in dataclasses.fields(tt):
        a, b = getattr(tt, f.name), getattr(more, f.name)
        if f.name in ("phr_ops", "span_ops"):
            assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b)), f.name
        elif f.name in ("phrases", "nears", "phr_cand_max", "phr_rows_cap", "near_cand_max", "near_rows_cap", "n_base"):
            assert a == b, f.name
    assert more.ops[3].tolist() == tt.ops[3].tolist() + [len(VOCAB) + 2] and more.n_cons == tt.n_cons + 1
    # ... and a sorted vocabulary handed to a table without a Prefix is not read
    same = pack(pairs, VOCAB, DF, N_DOCS, rows, sorted_vocab=["not", "the", "vocabulary"])
    for f in dataclasses.fields(tt):
        a, b = getattr(tt, f.name), getattr(same, f.name)
        if isinstance(a, tuple) and a and isinstance(a[0], np.ndarray):
            assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b)), f.name
        elif isinstance(a, np.ndarray):
            assert np.array_equal(a, b) and a.dtype == b.dtype, f.name
        else:
            assert a == b, f.name


# ---- the sorted vocabulary across live updates ---------------------------------------------------------------------------
def test_sorted_vocab_stays_correct_across_add_remove_and_replace():
    from legal_rag_amd.bm25_model import BM25Okapi
    m = BM25Okapi([["sell", "goods"], ["seller", "buys"], ["zebra"], ["goods", "buyer"]])
    first = m.sorted_vocab()
    assert first == sorted(m.vocab()) == ["buyer", "buys", "goods", "sell", "seller", "zebra"] and m.sorted_vocab() is first
    vocab = m.vocab()
    m.add_documents([["selling", "apple"], ["goods"]])
    assert m.vocab() is vocab and len(vocab) == 8  # extended IN PLACE: the same dict, longer
    assert m.sorted_vocab() == sorted(m.vocab()) and "selling" in m.sorted_vocab() and m.sorted_vocab() is not first
    tt = pack([(None, Terms(all_of=[Prefix("sell")]))], m.vocab(), m._doc_frequencies(), m.corpus_size, None, m.sorted_vocab())
    assert tt.union_ops[1].tolist() == sorted(m.vocab()[w] for w in ("sell", "seller", "selling"))
    m.remove_documents([2])
    assert "zebra" not in m.vocab() and m.sorted_vocab() == sorted(m.vocab()) and "zebra" not in m.sorted_vocab()
    m.replace_documents([0], [["sells", "wares"]])
    assert m.sorted_vocab() == sorted(m.vocab()) and "sells" in m.sorted_vocab() and "sell" not in m.sorted_vocab()
    back = pickle.loads(pickle.dumps(m))  # not pickled: made again on demand
    assert "_sorted_vocab" not in back.__dict__ and back.sorted_vocab() == m.sorted_vocab()


# ---- retriever.prefix ---------------------------------------------------------------------------------------------------
def test_prefix_cuts_a_string_with_the_document_side_tokeniser(tmp_path):
    from legal_rag_amd.retrieval.bm25_retriever import BM25Retriever
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    bm = BM25Retriever.__new__(BM25Retriever)
    bm.cfg = SimpleNamespace(retrieval=SimpleNamespace())
    bm.bm25_path = tmp_path / "bm25.pkl"
    bm.load = lambda: None
    bm.index_tokenizer = "en_regex"
    r = HybridRetriever.__new__(HybridRetriever)
    r.bm25 = bm
    assert r.prefix("Sell") == Prefix("sell") and r.prefix("  SECUR ") == Prefix("secur")
    for bad in ("", "buyer seller", "  "):
        with pytest.raises(ValueError, match="exactly one"):
            r.prefix(bad)
    bm.index_tokenizer = None
    with pytest.raises(ValueError, match="records no tokenizer"):
        r.prefix("sell")
    r.bm25 = object()
    with pytest.raises(ValueError, match="own BM25 retriever"):
        r.prefix("sell")


# ---- the plan --------------------------------------------------------------------------------------------------------------
def test_plan_arithmetic_and_null_handles(tile):
    from legal_rag_amd import _native
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for n in (1, 2, 65, 4096):
        for n_docs in (0, 1, tile - 1, tile, tile + 1, 3 * tile + 1, 10_000_000):
            cells = n * max(1, -(-n_docs // tile))
            assert _native.union_lists_plan(n, n_docs) == up(8 * cells) + up(8 * (cells + 1)) + up(tile // 8 * cells), (n, n_docs)
    assert _native.union_lists_plan(0, 100) >= 0
    for bad in ((-1, 10), (1, -1), (2**31, 1), (2**20, 10_000_000), (2**31 // 306 + 1, 10_000_000)):  # n_items x tiles >= 2^31
        with pytest.raises(_native.NativeError):
            _native.union_lists_plan(*bad)
    lib = _native.load()  # a null handle is refused before any device is touched
    assert lib.amdr_union_lists_device(None, None, None, 1, 0, 0, None, None, None, None, 0, None) == -1
    assert b"null handle" in lib.amdr_last_error()
    assert lib.amdr_union_lists(None, None, None, 1, 0, None, None, None) == -1
    assert b"null handle" in lib.amdr_last_error()

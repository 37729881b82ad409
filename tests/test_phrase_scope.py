"""Phrase constraints without a GPU: the certificates of tests/phrase_cases.py, `Phrase` and `Terms` typing and hashing, the
packer (phrases stored once, virtual ids, both bounds), `matches` on token sequences, the refusals before a launch, the
plan arithmetic (amdr_phrase_lists_plan) and the stream builder's consistency check (BM25Okapi.token_stream)."""
import pickle
from types import SimpleNamespace

import numpy as np
import pytest

import phrase_cases as PC
from legal_rag_amd.retrieval.scope import Scope
from legal_rag_amd.retrieval.terms import ANY, MUST, NOT, Phrase, Terms, driver_length, pack


# ---- the certificates --------------------------------------------------------------------------------------------------
def test_edge_corpus_certificates():
    corpus, at = PC.edge_corpus()
    PC.edge_certificates(corpus, at)
    ptr, tokens = corpus.stream()
    assert ptr[-1] == tokens.size == sum(len(s) for s in corpus.docs) and np.array_equal(np.diff(ptr), corpus.postings()[4])


def test_tiles_corpus_certificates():
    PC.tiles_certificates(PC.tiles_corpus())


def test_rand_corpus_and_constraint_certificates():
    corpus = PC.rand_corpus()
    PC.rand_certificates(corpus, PC.rand_phrases(corpus))
    phrases = PC.scope_phrases(corpus)
    PC.scope_certificates(corpus, PC.scope_family(corpus, phrases), phrases)


def test_reference_window_scan_on_written_out_cases():
    assert PC.holds([1, 2, 3], [2, 3]) and not PC.holds([1, 2, 3], [3, 2]) and not PC.holds([1], [1, 1])
    assert PC.starts([0, 0, 0], [0, 0]) == [0, 1] and PC.starts([], [0, 0]) == []


# ---- Phrase and Terms --------------------------------------------------------------------------------------------------
def test_phrase_is_frozen_hashable_and_bounded():
    p = Phrase("security", "interest")
    assert p == Phrase("security", "interest") and hash(p) == hash(Phrase("security", "interest"))
    assert p != Phrase("interest", "security") and p != ("security", "interest") and len(p) == 2
    assert p.tokens == ("security", "interest") and repr(p) == "Phrase('security', 'interest')"
    assert pickle.loads(pickle.dumps(p)) == p and {p: 1}[Phrase("security", "interest")] == 1
    with pytest.raises(AttributeError):
        p.tokens = ("x",)
    with pytest.raises(ValueError):
        Phrase()
    with pytest.raises(ValueError):
        Phrase(*["t"] * 17)
    assert len(Phrase(*["t"] * 16)) == 16
    with pytest.raises(TypeError):
        Phrase("a", 3)


def test_terms_take_a_phrase_wherever_a_token_stands():
    p = Phrase("a", "b")
    t = Terms(all_of=[p, ("c", p)], any_of=p, none_of=[Phrase("x")])
    assert t.all_of == ((p,), ("c", p)) and t.any_of == ((p,),) and t.has_phrase
    assert t.none_of == (("x",),)  # one token is the plain term
    assert t == Terms(all_of=[Phrase("a", "b"), ("c", Phrase("a", "b"))], any_of=[Phrase("a", "b")], none_of="x")
    assert hash(t) == hash(Terms(all_of=[Phrase("a", "b"), ("c", Phrase("a", "b"))], any_of=[Phrase("a", "b")], none_of="x"))
    assert t != Terms(all_of=[("a", "b"), ("c", "a", "b")], any_of=[("a", "b")], none_of="x")  # a group is not a phrase
    assert not Terms(all_of=[Phrase("x")]).has_phrase and Terms(all_of=[Phrase("x")]) == Terms(all_of="x")
    assert t.groups() == [(MUST, (p,)), (MUST, ("c", p)), (ANY, (p,)), (NOT, ("x",))]


def test_matches_takes_a_sequence_when_a_phrase_is_present():
    t = Terms(all_of=[Phrase("a", "b")], none_of=[Phrase("b", "a")])
    assert t.matches(["x", "a", "b"]) and t.matches(("a", "b"))
    assert not t.matches(["b", "a", "b"]) and not t.matches(["a", "x", "b"]) and not t.matches([])
    assert Terms(all_of=[("c", Phrase("a", "a"))]).matches(["a", "a", "a", "c"])
    assert not Terms(all_of=[("c", Phrase("a", "a"))]).matches(["a", "c", "a"])
    assert Terms(any_of=[Phrase("a", "b"), "z"]).matches(["z"])
    for bad in ({"a", "b"}, frozenset(["a", "b"]), {"a": 1, "b": 1}):
        with pytest.raises(TypeError, match="sequence"):
            t.matches(bad)
    assert Terms(all_of=["a", "b"]).matches({"a", "b"})  # without a phrase a set is what it always was


# ---- the packer ------------------------------------------------------------------------------------------------------------
VOCAB = {"a": 0, "b": 1, "c": 2, "d": 3}
DF = {"a": 50, "b": 30, "c": 90, "d": 9}


def test_pack_stores_equal_phrases_once_under_virtual_ids_with_both_bounds():
    ab, ba, az = Phrase("a", "b"), Phrase("b", "a"), Phrase("a", "zzz")
    pairs = [(None, Terms(all_of=[ab])), (None, Terms(all_of=[("c", ab)], none_of=[ba])), (None, Terms(any_of=[ab, az])),
             (None, Terms(all_of=[ab])), (None, Terms(all_of=["d", ab])), (None, Terms(all_of=[az]))]
    tt = pack(pairs, VOCAB, DF, 100)
    V = len(VOCAB)
    assert tt.phrases == (ab, ba, az) and tt.n_phr == 3
    assert tt.phr_ops[0].tolist() == [0, 2, 4, 6] and tt.phr_ops[1].tolist() == [0, 1, 1, 0, 0, -1]
    assert tt.phr_ops[0].dtype == np.int64 and tt.phr_ops[1].dtype == np.int32
    assert tt.qscope.tolist() == [0, 1, 2, 0, 3, 4] and tt.n_cons == 5
    assert tt.ops[3].tolist() == [V + 0, 2, V + 0, V + 1, V + 0, V + 2, 3, V + 0, V + 2]
    # the upper bound of a phrase: the smallest document frequency among its tokens; 0 with an unknown one
    assert (tt.phr_cand_max, tt.phr_rows_cap) == (30, 30 + 30 + 0)
    # the drivers: the phrase's bound; min(c, the bound); no MUST: the corpus; "d" is rarer than the bound; empty
    assert tt.driver_lens.tolist() == [30, 30, 100, 9, 0] and (tt.cand_max, tt.rows_cap) == (100, 169)
    plain = pack([(None, Terms(all_of=["a"]))], VOCAB, DF, 100)
    assert plain.n_phr == 0 and plain.phr_ops[0].tolist() == [0] and plain.phr_ops[1].size == 0
    assert (plain.phr_cand_max, plain.phr_rows_cap) == (0, 0)


def test_driver_length_reads_the_upper_bound_of_a_phrase():
    df = np.asarray([50, 30, 90, 9, 30, 0])  # four terms, then two phrases' upper bounds
    assert driver_length([(MUST, [4])], df, None, 100) == 30
    assert driver_length([(MUST, [4]), (MUST, [3])], df, None, 100) == 9
    assert driver_length([(MUST, [2, 4])], df, 12, 100) == 12
    assert driver_length([(MUST, [5])], df, None, 100) == 0
    assert driver_length([(ANY, [4]), (NOT, [4])], df, None, 100) == 100
    assert driver_length([(MUST, [6])], df, None, 100) == 0  # past the virtual ids: in no document


def test_pack_with_a_base_scope_and_a_phrase():
    s = Scope(section="S")
    tt = pack([(s, Terms(all_of=[Phrase("a", "b")]))], VOCAB, DF, 100, lambda sc: np.arange(7, dtype=np.int64))
    assert tt.driver_lens.tolist() == [7] and tt.n_base == 1 and tt.phr_cand_max == 30


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


def test_phrases_are_refused_where_terms_are(monkeypatch):
    t = Terms(all_of=[Phrase("security", "interest")])
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


def test_the_document_side_tokeniser_and_its_refusals(tmp_path):
    from legal_rag_amd.retrieval.bm25_retriever import BM25Retriever
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    bm = BM25Retriever.__new__(BM25Retriever)
    bm.cfg = SimpleNamespace(retrieval=SimpleNamespace())
    bm.bm25_path = tmp_path / "bm25.pkl"
    bm.load = lambda: None
    bm.index_tokenizer = "en_regex"
    r = HybridRetriever.__new__(HybridRetriever)
    r.bm25 = bm
    assert r.phrase("Security Interest") == Phrase("security", "interest")
    assert r.phrase("the buyer's  RIGHT") == Phrase("the", "buyer's", "right")
    with pytest.raises(ValueError, match="no token"):
        r.phrase(" ... ")
    with pytest.raises(ValueError, match="1 to 16"):
        r.phrase(" ".join(["w"] * 17))
    bm.index_tokenizer = None  # a reference rank_bm25 pickle records no tokeniser
    with pytest.raises(ValueError, match="records no tokenizer"):
        r.phrase("security interest")
    bm.index_tokenizer = "pretokenized"
    with pytest.raises(ValueError, match="cannot be cut again"):
        bm.document_tokens("security interest")
    r.bm25 = object()
    with pytest.raises(ValueError, match="own BM25 retriever"):
        r.phrase("security interest")


# ---- the stream builder ----------------------------------------------------------------------------------------------------
def test_token_stream_checks_every_document_against_the_index():
    from legal_rag_amd.bm25_model import BM25Okapi
    docs = [["a", "b", "a"], [], ["c"], ["b", "c", "c", "a"]]
    m = BM25Okapi(docs)
    ptr, tokens = m.token_stream(docs)
    v = m.vocab()
    assert ptr.tolist() == [0, 3, 3, 4, 8] and ptr.dtype == np.int64 and tokens.dtype == np.int32
    assert tokens.tolist() == [v[w] for d in docs for w in d]
    assert np.array_equal(np.diff(ptr), np.asarray(m.doc_len))
    with pytest.raises(RuntimeError, match="3 documents"):
        m.token_stream(docs[:3])
    with pytest.raises(RuntimeError, match="document 2 has 2 tokens"):
        m.token_stream([docs[0], docs[1], ["c", "c"], docs[3]])
    with pytest.raises(RuntimeError, match="document 0 are not the ones"):
        m.token_stream([["a", "b", "b"], docs[1], docs[2], docs[3]])  # the same length, other counts
    ptr2, tokens2 = m.token_stream([["a", "a", "b"], docs[1], docs[2], docs[3]])  # the counts cannot see an order
    assert tokens2.tolist()[:3] == [v["a"], v["a"], v["b"]]


# ---- the plan --------------------------------------------------------------------------------------------------------------
def test_plan_arithmetic_and_null_handles():
    from legal_rag_amd import _native
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    assert _native.PHRASE_TILE == PC.TILE and _native.PHRASE_MAX_LEN == PC.MAX_LEN
    for n_phr in (1, 2, 65, 1168, 70_000):
        for cand_max in (0, 1, 255, 256, 257, 513, 4100):
            cells = n_phr * max(1, -(-cand_max // _native.PHRASE_TILE))
            # counts i64 per cell | offsets i64 per cell + 1 | 256 ranks of 4 bytes per cell
            assert _native.phrase_lists_plan(n_phr, cand_max) == up(8 * cells) + up(8 * (cells + 1)) + up(1024 * cells)
    assert _native.phrase_lists_plan(0, 0) >= 0
    for bad in ((-1, 10), (1, -1), (1, 65_536 * 256)):  # negative sizes; more tiles than the grid's y holds
        with pytest.raises(_native.NativeError):
            _native.phrase_lists_plan(*bad)
    assert _native.phrase_lists_plan(1, 65_535 * 256) > 0
    lib = _native.load()  # a null handle is refused before any device is touched
    assert lib.amdr_phrase_lists_device(None, None, None, 1, 0, 0, None, None, None, None, 0, None) == -1
    assert b"null handle" in lib.amdr_last_error()
    assert lib.amdr_phrase_lists(None, None, None, 1, 0, 0, None, None, None) == -1
    assert b"null handle" in lib.amdr_last_error()
    assert lib.amdr_term_scope_lists_device(*([None] * 10), 0, 0, 1, 0, 0, 0, None, None, None, None, 0, None) == -1
    assert b"null handle" in lib.amdr_last_error()
    assert lib.amdr_term_scope_lists(*([None] * 10), 0, 0, 1, 0, 0, 0, None, None, None) == -1
    assert b"null handle" in lib.amdr_last_error()
    for fn in (lib.amdr_bm25_set_tokens, lib.amdr_bm25_read_tokens):
        assert fn(None, None, None) == -1
    assert lib.amdr_bm25_tokens_info(None, None) == -1

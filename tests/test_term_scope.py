"""Term constraints without a GPU: `Terms` (retrieval/terms.py), the packer and its host bounds, every refusal that is made
before a launch, the plan arithmetic (amdr_term_scope_plan) and the certificates of tests/term_scope_cases.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import term_scope_cases as TC
from legal_rag_amd.retrieval.scope import Scope
from legal_rag_amd.retrieval.terms import ANY, MUST, NOT, Terms, driver_length, pack


# ---- Terms -------------------------------------------------------------------------------------------------------------
def test_terms_are_frozen_equal_and_hash_alike():
    a = Terms(all_of=["seller", ("goods", "sale")], none_of="buyer")
    b = Terms(all_of=("seller", ["goods", "sale"]), none_of=["buyer"])
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    assert a.all_of == (("seller",), ("goods", "sale")) and a.none_of == (("buyer",),) and a.any_of is None
    assert a != Terms(all_of=["seller", ("sale", "goods")], none_of="buyer")  # a group is an ordered tuple of tokens
    assert a != Terms(all_of=["seller", ("goods", "sale")])
    with pytest.raises(Exception):
        a.all_of = None  # frozen
    assert a.groups() == [(MUST, ("seller",)), (MUST, ("goods", "sale")), (NOT, ("buyer",))]
    assert Terms(any_of=[("合", "同")]).groups() == [(ANY, ("合", "同"))]


def test_terms_with_nothing_given_are_unrestricted():
    for t in (Terms(), Terms(all_of=None, any_of=[], none_of=()), Terms(all_of=[])):
        assert t.unrestricted and t == Terms() and t.groups() == []
    assert not Terms(none_of="x").unrestricted


@pytest.mark.parametrize("field", ["all_of", "any_of", "none_of"])
def test_an_empty_group_is_refused(field):
    with pytest.raises(ValueError, match="empty group"):
        Terms(**{field: ["seller", ()]})


def test_matches_is_the_rule_on_one_token_set():
    t = Terms(all_of=["seller", ("goods", "sale")], any_of=["warranty", "lease"], none_of=[("buyer", "price")])
    assert t.matches({"seller", "goods", "sale", "lease"})
    assert t.matches(["seller", "goods", "sale", "lease", "buyer"])          # the NOT group needs both its tokens
    assert not t.matches({"seller", "goods", "sale", "lease", "buyer", "price"})
    assert not t.matches({"seller", "goods", "lease"})                        # a MUST group needs all its tokens
    assert not t.matches({"seller", "goods", "sale"})                         # no ANY entry
    assert Terms().matches(set())


# ---- the packer --------------------------------------------------------------------------------------------------------
VOCAB = {"seller": 0, "goods": 1, "buyer": 2, "warranty": 3, "lease": 4}
DF = {"seller": 40, "goods": 90, "buyer": 70, "warranty": 7, "lease": 12}
N = 100


def rows_of(scope):
    return {"A": np.arange(0, 30, dtype=np.int64), "B": np.arange(10, 15, dtype=np.int64)}[scope.section]


def test_pack_lays_out_the_operands_and_stores_equal_pairs_once():
    t1 = Terms(all_of=["seller", "goods"], none_of="buyer")
    t2 = Terms(any_of=["warranty", ("lease", "nope")])
    sa, sb = Scope(section="A"), Scope(section="B")
    pairs = [(None, t1), (sa, t2), (None, t1), (sb, t1), (sa, Terms()), (sa, t2), (Scope(), t1)]
    tt = pack(pairs, VOCAB, DF, N, rows_of)
    assert tt.qscope.tolist() == [0, 1, 0, 2, 3, 1, 0] and tt.qscope.dtype == np.int32  # (an unrestricted Scope is no base)
    assert (tt.n_cons, tt.n_groups, tt.n_base) == (4, 8, 2)
    grp_ptr, grp_kind, grp_term_ptr, grp_terms, base_ptr, base_rows, cons_base = tt.ops
    assert [a.dtype for a in tt.ops] == [np.int64, np.int32, np.int64, np.int32, np.int64, np.int64, np.int32]
    assert grp_ptr.tolist() == [0, 3, 5, 8, 8]
    assert grp_kind.tolist() == [MUST, MUST, NOT, ANY, ANY, MUST, MUST, NOT]
    assert grp_term_ptr.tolist() == [0, 1, 2, 3, 4, 6, 7, 8, 9]
    assert grp_terms.tolist() == [0, 1, 2, 3, 4, -1, 0, 1, 2]  # "nope" is not in the vocabulary: -1
    assert cons_base.tolist() == [-1, 0, 1, 0]                 # scope A stored once
    assert base_ptr.tolist() == [0, 30, 35] and base_rows.tolist() == list(range(30)) + list(range(10, 15))
    # the bounds: the shortest of {base, each MUST term's list}; no MUST term and a base: the base; cand_max / rows_cap
    assert tt.driver_lens.tolist() == [40, 30, 5, 30] and tt.cand_max == 40 and tt.rows_cap == 105


def test_driver_length_follows_the_header_rule():
    df = np.asarray([40, 90, 70, 7, 12])
    assert driver_length([(MUST, [0, 1])], df, None, N) == 40
    assert driver_length([(MUST, [1]), (MUST, [3]), (NOT, [0])], df, None, N) == 7
    assert driver_length([(MUST, [1]), (ANY, [3])], df, None, N) == 90     # ANY and NOT terms never drive
    assert driver_length([(MUST, [1, -1])], df, 3, N) == 0                 # an unknown MUST term: empty
    assert driver_length([(MUST, [5])], df, None, N) == 0                  # a term id past the vocabulary too
    assert driver_length([(ANY, [3])], df, None, N) == N                   # the iota form
    assert driver_length([(ANY, [3])], df, 0, N) == 0                      # an empty base drives
    assert driver_length([(MUST, [3])], df, 7, N) == 7                     # a tie: either way the same length
    assert driver_length([], df, None, N) == N
    tt = pack([(None, Terms(any_of="warranty"))], VOCAB, DF, N)
    assert tt.cand_max == N and tt.rows_cap == N


def test_pack_refuses_what_is_not_a_terms():
    with pytest.raises(TypeError, match="not a Terms"):
        pack([(None, "seller")], VOCAB, DF, N)


# ---- refusals before any launch ----------------------------------------------------------------------------------------
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


def test_terms_with_a_graph_mode_decision_are_refused(monkeypatch):
    r = retriever(monkeypatch, plain_native())
    graph = SimpleNamespace(mode="GRAPH_AUGMENTED")
    t = Terms(all_of="seller")
    with pytest.raises(ValueError, match="graph-mode decision and term constraints"):
        r.search_batch(["q", "q"], terms=[None, t], decisions=[None, graph])
    with pytest.raises(ValueError, match="graph-mode decision and term constraints"):
        r.search_batch_arrays(["q"], terms=[t], decisions=[graph])
    with pytest.raises(ValueError, match="graph-mode decision and term constraints"):
        r.search("q", terms=t, decision=graph)


def test_terms_on_a_row_sharded_index_are_refused(monkeypatch):
    t = Terms(all_of="seller")
    for over in ({"dense_spec": object()}, {"bm25_shard": object()}):
        r = retriever(monkeypatch, plain_native(**over))
        for call in (lambda: r.search_batch(["q"], terms=[t]), lambda: r.search_batch_arrays(["q"], terms=[t]),
                     lambda: r.search("q", terms=t)):
            with pytest.raises(ValueError, match="row-sharded"):
                call()
    from legal_rag_amd.retrieval.engine import HybridEngine
    eng = HybridEngine.__new__(HybridEngine)
    eng.shard_offset, eng.bm25 = 128, object()
    with pytest.raises(ValueError, match="row-sharded"):
        eng.check_term_scopes()
    with pytest.raises(ValueError, match="row-sharded"):
        eng.term_scopes(None)
    eng.shard_offset, eng.bm25 = None, None
    with pytest.raises(ValueError, match="BM25 index"):
        eng.check_term_scopes()


def test_terms_without_one_shared_chunk_list_are_refused(monkeypatch):
    r = retriever(monkeypatch, None)  # the channels do not share one chunk list: no device-resident stage
    t = Terms(all_of="seller")
    for call in (lambda: r.search_batch(["q"], terms=[t]), lambda: r.search_batch_arrays(["q"], terms=[t]),
                 lambda: r.search("q", terms=t)):
        with pytest.raises(ValueError, match="one chunk list"):
            call()
    with pytest.raises(RuntimeError):  # without terms: the error it always was
        r.search_batch(["q"], terms=[None])


def test_terms_must_be_one_per_question_and_of_the_type(monkeypatch):
    r = retriever(monkeypatch, plain_native())
    with pytest.raises(ValueError, match="one entry per question"):
        r.search_batch(["q", "q"], terms=[Terms(all_of="x")])
    with pytest.raises(TypeError, match="not a Terms"):
        r.search_batch(["q"], terms=["seller"])


def test_unrestricted_terms_leave_the_partition_as_it_was():
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    chunks = plain_native()[0].chunks
    qs = ["a", "b", "c"]
    base = HybridRetriever._partition(qs, None, None, chunks, False, "t")
    assert HybridRetriever._partition(qs, None, None, chunks, False, "t", [None, Terms(), None]) == base
    parts, empty = HybridRetriever._partition(qs, [None, None, Scope(section="S")], None, chunks, False, "t",
                                              [Terms(none_of="x"), None, None])
    assert parts == [([1], False, False), ([0, 2], True, False)] and empty == []
    parts, empty = HybridRetriever._partition(qs, [Scope(section="none"), None, None], None, chunks, False, "t",
                                              [Terms(none_of="x"), None, None])
    assert empty == [0] and parts == [([1, 2], False, False)]  # an empty base scope: nothing to resolve


# ---- the plan ----------------------------------------------------------------------------------------------------------
def test_plan_arithmetic():
    from legal_rag_amd import _native
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for n_cons in (1, 2, 65, 1168, 70_000):
        for cand_max in (0, 1, 1023, 1024, 1025, 2049, 4100):
            cells = n_cons * max(1, -(-cand_max // _native.TERM_SCOPE_TILE))
            # counts i64 per cell | offsets i64 per cell + 1 | 256 keep words of 4 bytes per cell
            assert _native.term_scope_plan(n_cons, cand_max) == up(8 * cells) + up(8 * (cells + 1)) + up(1024 * cells)
    assert _native.term_scope_plan(0, 0) >= 0
    for bad in ((-1, 10), (1, -1), (1, 65_536 * 1024)):  # negative sizes; more tiles than the grid's y holds
        with pytest.raises(_native.NativeError):
            _native.term_scope_plan(*bad)
    # a null handle is refused before any device is touched
    lib = _native.load()
    assert lib.amdr_term_scope_device(*([None] * 8), 0, 1, 0, 0, 0, None, None, None, None, 0, None) == -1
    assert b"null handle" in lib.amdr_last_error()
    assert lib.amdr_term_scope(*([None] * 8), 0, 1, 0, 0, 0, None, None, None) == -1
    assert b"null handle" in lib.amdr_last_error()


# ---- the certificates of the cases -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpora():
    return TC.corpora()


def test_cases_expected_rows_are_the_rule_and_the_bounds_hold(corpora):
    fams = TC.families()
    assert len(fams) >= 17
    for fam in fams:
        corpus = corpora[fam.corpus]
        df = corpus.df()
        proper, lens, counts = False, [], []
        for con in fam.cons:
            want = TC.expected(corpus, con, fam.bases)
            base_set = None if con[1] < 0 else {int(x) for x in fam.bases[con[1]]}
            slow = [d for d, have in enumerate(corpus.docs) if TC.doc_qualifies(d, have, con, base_set)]
            assert want.tolist() == slow and np.all(np.diff(want) > 0), (fam.name, con)
            proper = proper or 0 < want.size < corpus.n_docs
            lens.append(driver_length(con[0], df, None if con[1] < 0 else int(fam.bases[con[1]].size), corpus.n_docs))
            counts.append(int(want.size))
            assert counts[-1] <= lens[-1], (fam.name, con)  # the candidates hold every qualifying document
        # (a one-document corpus has no non-empty proper subset)
        assert proper or corpus.n_docs == 1, fam.name
        assert max(lens) >= max(counts) and sum(lens) >= sum(counts)  # cand_max, rows_cap
    big = corpora["big"]
    assert big.n_docs == 4100 and big.n_terms <= 64
    df = big.df()
    assert [int(df[t]) for t in (TC.T_NONE, TC.T_ONE, TC.T_1023, TC.T_1024, TC.T_1025, TC.T_2049)] == [0, 1, 1023, 1024, 1025, 2049]
    assert df[TC.T_TIE_A] == df[TC.T_TIE_B] == 500 and df[TC.T_ALL] == 4100
    assert big.holders(TC.T_ENDS) == {0, 4099}

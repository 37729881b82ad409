"""The carrying updates at the native level (amdr_bm25_add_carry / _remove_carry / _replace_carry, csrc/bm25_update.hip,
csrc/tok_carry_rule.hpp): small corpora given as one token sequence per document, whose expected stream after an edit is
SeqCorpus.stream() of the edited documents.  After every carrying call: read_tokens() is that stream, array for array
with the same dtypes; tokens_info() says so; phrases, Nears, unions and class spans resolve to the references' lists with
no set_tokens in between; and the six index arrays are a fresh handle's, as the plain updates' tests check."""
from types import SimpleNamespace

import ctypes as C
import numpy as np
import pytest

import class_span_cases as CC
import near_cases as NC
import phrase_cases as PC
import union_cases as UC
import update_sequence_cases as SQ
from bm25_update_cases import nat, same_arrays  # noqa: F401 - `nat` is the fixture

pytestmark = pytest.mark.gpu

TILE = 2048
V0 = 40  # terms of the generated corpora; V0 - 1, V0 - 2 and V0 - 3 live in one document each


def make_corpus(seed, n_docs, max_len, long_at=None, long_len=0, empties_at=None, empties=0):
    """Random documents of 0 .. max_len tokens over V0 - 3 terms; document 0, the middle one (`mid_of`) and the last hold a
    term of their own (it goes with them) and at least three tokens.  Optionally one long document, or a run of empty
    ones (the middle document is then the one in front of the run, which stays whole)."""
    rng = np.random.default_rng(seed)
    docs = [rng.integers(0, V0 - 3, size=int(rng.integers(0, max_len + 1))).tolist() for _ in range(n_docs)]
    if long_at is not None:
        docs[long_at] = rng.integers(0, V0 - 3, size=long_len).tolist()
    if empties_at is not None:
        docs[empties_at:empties_at] = [[] for _ in range(empties)]
    n = len(docs)
    docs[0] = [V0 - 1] + docs[0] + [0, 1]
    mid = mid_of(n) if empties_at is None else empties_at - 1
    docs[mid] = docs[mid] + [V0 - 3, 2, 3]
    docs[n - 1] = docs[n - 1] + [V0 - 2, 0, 1]
    return PC.SeqCorpus(f"c{seed}", V0, docs)


def mid_of(n):
    return n // 2


def total(corpus):
    return int(corpus.stream()[0][-1])


def index_of(nat, corpus, tokens=True):
    tp, pd, pt, idf, dl, avgdl = corpus.postings()
    g = nat.BM25Index(tp, pd, pt, idf, dl, avgdl)
    if tokens:
        g.set_tokens(*corpus.stream())
    return g


def csr_of(docs, n_terms):
    """The documents' own term-major CSR over n_terms terms (local ids) and their lengths."""
    tp, pd, pt, _, dl, _ = PC.SeqCorpus("add", n_terms, [list(d) for d in docs]).postings()
    return tp, pd, pt, dl


def refit_map(corpus, gone, new_words=0):
    """(term_map, n_terms_new): the terms the documents outside `gone` still use, in REVERSE order, the others dropped;
    `new_words` new ids behind them."""
    used = sorted({t for d, seq in enumerate(corpus.docs) if d not in set(gone) for t in seq})
    tmap = np.full(corpus.n_terms, -1, dtype=np.int32)
    for j, t in enumerate(used):
        tmap[t] = len(used) - 1 - j
    return tmap, len(used) + new_words


def edited(old, op):
    """The edited corpus, plainly."""
    kind = op[0]
    if kind == "add":
        _, added, v_new = op
        return PC.SeqCorpus("new", v_new, [list(d) for d in old.docs] + [list(d) for d in added])
    if kind == "remove":
        _, ids, tmap, v_new = op
        f = (lambda t: t) if tmap is None else (lambda t: int(tmap[t]))
        return PC.SeqCorpus("new", v_new, [[f(t) for t in d] for i, d in enumerate(old.docs) if i not in set(ids)])
    _, ids, docs_new, tmap, v_new = op
    f = (lambda t: t) if tmap is None else (lambda t: int(tmap[t]))
    put = dict(zip(ids, docs_new))
    return PC.SeqCorpus("new", v_new, [list(put[i]) if i in put else [f(t) for t in d] for i, d in enumerate(old.docs)])


def apply(g, old, op, carry=True):
    """The native call of `op` on handle g that holds `old`; returns the edited corpus."""
    new = edited(old, op)
    _, _, _, idf, _, avgdl = new.postings()
    if op[0] == "add":
        tp, pd, pt, dl = csr_of(op[1], op[2])
        g.add(tp, pd, pt, idf, dl, avgdl, tokens=PC.SeqCorpus("a", op[2], op[1]).stream() if carry else None)
    elif op[0] == "remove":
        g.remove(np.asarray(op[1], np.int64), idf, avgdl, term_map=op[2], carry=carry)
    else:
        tp, pd, pt, dl = csr_of(op[2], op[4])
        g.replace(np.asarray(op[1], np.int64), tp, pd, pt, dl, idf, avgdl, term_map=op[3],
                  tokens=PC.SeqCorpus("a", op[4], op[2]).stream() if carry else None)
    return new


def check_index(nat, g, corpus):
    f = index_of(nat, corpus, tokens=False)
    same_arrays(g.read(), f.read())
    assert g.info()[:3] == f.info()[:3]
    f.close()


def check_stream(g, corpus):
    dp, tk = corpus.stream()
    gp, gt = g.read_tokens()
    assert gp.dtype == dp.dtype and gt.dtype == tk.dtype
    assert np.array_equal(gp, dp) and np.array_equal(gt, tk)
    assert g.tokens_info() == (True, int(dp[-1]))


def check_resolvers(g, corpus, at):
    """Phrases, Nears, unions and class spans over tokens of both sides of document `at`, against the references.  (The
    nearest document of two tokens or more from `at` on gives a Near its own length as distance: at most 255 tokens.)"""
    st = SimpleNamespace(at=at, n=corpus.n_docs, docs=corpus.docs, vocab={t: t for t in range(corpus.n_terms)})
    phrases, nears, unions, classes = SQ.bm25_span_items(st)
    lens = [PC.driver_len(corpus, p) for p in phrases]
    for got, want, what in (
            (g.phrase_lists(*PC.operands(phrases), max(lens), sum(lens)), PC.expected_lists(corpus, phrases), "phrase"),
            (g.span_lists(*NC.operands(nears), *NC.bounds(corpus, nears)), NC.expected_lists(corpus, nears), "near"),
            (g.union_lists(*UC.operands(unions), UC.rows_cap(corpus, unions)), UC.expected_lists(corpus, unions), "union"),
            (g.class_spans(*[x for part in CC.operands(classes, corpus.n_terms) for x in part], *CC.bounds(corpus, classes)),
             CC.expected_lists(corpus, classes), "class span")):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and not got[2].any(), what
    assert PC.expected_lists(corpus, phrases)[0][-1] > 0  # the phrases are taken from documents: they match somewhere


def check(nat, g, corpus, at):
    check_stream(g, corpus)
    check_resolvers(g, corpus, at)
    check_index(nat, g, corpus)


def run(nat, old, op, at):
    g = index_of(nat, old)
    ms0 = g.carry_kernel_ms()
    new = apply(g, old, op)
    check(nat, g, new, at)
    assert ms0 == -1.0 and g.carry_kernel_ms() >= 0.0
    g.close()
    return new


def straddler(corpus, seam=TILE):
    """A document with tokens on both sides of stream position `seam`."""
    dp = corpus.stream()[0]
    d = int(np.searchsorted(dp, seam, side="right")) - 1
    assert dp[d] < seam < dp[d + 1], "no document straddles the seam"
    return d


@pytest.fixture(scope="module")
def base():
    c = make_corpus(11, 170, 30)  # more than one tile of tokens
    assert TILE < total(c) < 2 * TILE
    return c


# ---- add ----------------------------------------------------------------------------------------------------------------
def test_add_with_new_terms(nat, base):
    rng = np.random.default_rng(1)
    added = [rng.integers(0, V0 + 3, size=n).tolist() for n in (7, 0, 33, 2)] + [[V0, V0 + 1, V0 + 2, 0]]
    run(nat, base, ("add", added, V0 + 3), base.n_docs)


def test_add_of_only_empty_documents_with_a_null_token_array(nat, base):
    g = index_of(nat, base)
    new = apply(g, base, ("add", [[], [], []], V0))
    assert nat.BM25Index._token_args(PC.SeqCorpus("a", V0, [[], [], []]).stream(), 3, "add")[1] is None  # tok_add is null
    assert new.n_docs == base.n_docs + 3 and total(new) == total(base)
    check(nat, g, new, base.n_docs - 1)
    g.close()


def test_add_that_crosses_one_and_two_tiles(nat):
    old = make_corpus(12, 120, 28)
    rng = np.random.default_rng(2)
    added = [rng.integers(0, V0, size=int(n)).tolist() for n in rng.integers(20, 60, size=70)]
    new = run(nat, old, ("add", added, V0), old.n_docs)
    assert total(old) < TILE and total(new) > 2 * TILE


# ---- remove -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["first", "last", "straddler", "all but one", "null map"])
def test_remove(nat, base, which):
    n = base.n_docs
    ids = {"first": [0], "last": [n - 1], "straddler": [straddler(base)], "all but one": [d for d in range(n) if d != mid_of(n)],
           "null map": [3, n // 2, n - 4]}[which]
    if which == "null map":
        op = ("remove", ids, None, V0)  # the emptied term keeps its id with an empty list
    else:
        op = ("remove", ids) + refit_map(base, ids)
    new = run(nat, base, op, 0 if which == "all but one" else ids[0])
    assert new.n_docs == n - len(ids)


def test_remove_under_a_permutation_with_dropped_terms(nat, base):
    n = base.n_docs
    ids = [0, n // 2, n - 1]  # the three documents that hold a term of their own
    tmap, v_new = refit_map(base, ids)
    kept = tmap[tmap >= 0]
    assert v_new <= V0 - 3 and (tmap[[V0 - 1, V0 - 2, V0 - 3]] == -1).all() and (np.diff(kept) < 0).all()
    run(nat, base, ("remove", ids, tmap, v_new), n // 2)


def test_remove_around_a_document_of_5000_tokens(nat):
    old = make_corpus(13, 20, 20, long_at=2, long_len=5000)
    new = run(nat, old, ("remove", [0, 19]) + refit_map(old, [0, 19]), 2)  # (items from the long document and the next)
    dp = new.stream()[0]
    assert dp[1] // TILE == 0 and (dp[2] - 1) // TILE == 2  # the long document spans three tiles of the new stream


def test_remove_around_a_run_of_2051_empty_documents(nat):
    old = make_corpus(14, 16, 12, empties_at=8, empties=2051)
    n = old.n_docs
    new = run(nat, old, ("remove", [0, n - 1]) + refit_map(old, [0, n - 1]), 7)
    # one tile whose window of the new tok_ptr exceeds the LDS copy: tokens on both sides of the whole run
    assert total(new) < TILE and all(not d for d in new.docs[7:7 + 2051]) and new.docs[6] and any(new.docs[7 + 2051:])


# ---- replace ------------------------------------------------------------------------------------------------------------
def test_replace_a_document_by_an_empty_one(nat, base):
    run(nat, base, ("replace", [3], [[]], None, V0), 3)


def test_replace_a_document_by_one_longer_than_a_tile(nat, base):
    long_doc = np.random.default_rng(3).integers(0, V0, size=TILE + 500).tolist()
    new = run(nat, base, ("replace", [3], [long_doc], None, V0), 4)  # (items from the long document and the next)
    assert total(new) > total(base) + TILE


def test_replace_the_first_and_the_last_document(nat, base):
    n = base.n_docs
    docs_new = [[5, 6, 7, 5], [8, 9]]
    run(nat, base, ("replace", [0, n - 1], docs_new, None, V0), 0)


def test_replace_every_document(nat):
    old = make_corpus(15, 24, 12)
    rng = np.random.default_rng(4)
    docs_new = [rng.integers(0, V0 + 2, size=int(n)).tolist() for n in rng.integers(0, 20, size=old.n_docs)]
    docs_new[0], docs_new[-1] = [V0, V0 + 1, 0], [1, 2, 3]
    run(nat, old, ("replace", list(range(old.n_docs)), docs_new, None, V0 + 2), 1)


def test_replace_with_new_terms_and_a_reordering_map(nat, base):
    n = base.n_docs
    ids = [0, 17, n - 1]
    tmap, v_kept = refit_map(base, ids)
    v_new = v_kept + 2
    assert (tmap[[V0 - 1, V0 - 2]] == -1).all() and (np.diff(tmap[tmap >= 0]) < 0).all()
    docs_new = [[v_new - 1, 0, 1, v_new - 2], [], [2, v_new - 1, 2]]
    run(nat, base, ("replace", ids, docs_new, tmap, v_new), 17)


# ---- without a stream, plain calls with one, size 0 ----------------------------------------------------------------------
def ops_of(base):
    n = base.n_docs
    return (("add", [[1, 2, V0], []], V0 + 1), ("remove", [0, n - 1]) + refit_map(base, [0, n - 1]),
            ("replace", [2, n - 1], [[4, 4], [V0, 1]], None, V0 + 1))


def test_carrying_calls_without_a_stream_are_the_plain_calls(nat, base):
    for op in ops_of(base):
        g = index_of(nat, base, tokens=False)
        new = apply(g, base, op)
        assert g.tokens_info() == (False, 0) and g.carry_kernel_ms() == -1.0
        check_index(nat, g, new)
        g.close()


def test_plain_calls_still_drop_the_stream(nat, base):
    for op in ops_of(base):
        g = index_of(nat, base)
        new = apply(g, base, op, carry=False)
        assert g.tokens_info() == (False, 0) and g.carry_kernel_ms() == -1.0
        check_index(nat, g, new)
        g.close()


def test_calls_of_size_zero_leave_the_stream(nat, base):
    g = index_of(nat, base)
    idf = base.postings()[3]
    z64, z32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
    none = (np.zeros(1, np.int64), z32)
    g.add(np.zeros(V0 + 1, np.int64), z32, z32, idf, z32, 1.0, tokens=none)
    g.remove(z64, idf, 1.0, carry=True)
    g.replace(z64, np.zeros(V0 + 1, np.int64), z32, z32, z32, idf, 1.0, tokens=none)
    assert g.info()[3] == 0 and g.info()[5] == 0 and g.replaces() == 0 and g.carry_kernel_ms() == -1.0
    check(nat, g, base, 0)
    g.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------
def snapshot(g):
    return g.read(), g.read_tokens(), g.info(), g.replaces(), g.tokens_info()


def assert_unchanged(g, snap):
    now = snapshot(g)
    same_arrays(now[0], snap[0])
    same_arrays(now[1], snap[1])
    assert now[2:] == snap[2:]


def test_refusals_leave_index_and_stream_as_they_were(nat, base):
    g = index_of(nat, base)
    snap = snapshot(g)
    added = [[5, 6, 7], [4], []]
    tp, pd, pt, dl = csr_of(added, V0)
    new = edited(base, ("add", added, V0))
    _, _, _, idf, _, avgdl = new.postings()
    good_ptr, good_tok = PC.SeqCorpus("a", V0, added).stream()
    n = base.n_docs

    def add(tok_ptr, tok):
        g.add(tp, pd, pt, idf, dl, avgdl, tokens=(tok_ptr, tok))

    def replace(tok_ptr, tok):
        g.replace(np.asarray([1, 5, 9], np.int64), tp, pd, pt, dl, base.postings()[3], avgdl, tokens=(tok_ptr, tok))
    for call in (add, replace):
        for what, tok_ptr, tok in (
                ("lengths that disagree with doc_len_add", np.asarray([0, 2, 4, 4], np.int64), good_tok),
                ("a token >= n_terms_new", good_ptr, np.asarray([1, 2, V0, 4], np.int32)),
                ("a negative token", good_ptr, np.asarray([1, -1, 3, 4], np.int32)),
                ("tok_ptr_add[0] != 0", np.asarray([1, 3, 4, 4], np.int64), good_tok),
                ("tok_ptr_add not monotone", np.asarray([0, 4, 3, 4], np.int64), good_tok)):
            with pytest.raises(nat.NativeError, match="status -1"):
                call(tok_ptr, tok)
            assert_unchanged(g, snap)
    # a null tok_ptr_add: the wrapper never passes one, so the call is made as a C caller makes it
    lib = nat.load()
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    idf_c = np.ascontiguousarray(idf, np.float64)
    rc = lib.amdr_bm25_add_carry(g._h, p(tp, C.c_int64), p(pd, C.c_int32), p(pt, C.c_int32), p(idf_c, C.c_double),
                                 p(dl, C.c_int32), C.c_int64(V0), C.c_int64(3), C.c_double(avgdl), None, p(good_tok, C.c_int32))
    assert rc == -1 and b"bm25_add_carry" in lib.amdr_last_error()
    assert_unchanged(g, snap)
    # a null tok_add while the arrays hold tokens
    rc = lib.amdr_bm25_add_carry(g._h, p(tp, C.c_int64), p(pd, C.c_int32), p(pt, C.c_int32), p(idf_c, C.c_double),
                                 p(dl, C.c_int32), C.c_int64(V0), C.c_int64(3), C.c_double(avgdl), p(good_ptr, C.c_int64), None)
    assert rc == -1
    assert_unchanged(g, snap)
    # on the device flag path: the map sends term 0, which surviving documents still use, to -1
    tmap = np.arange(-1, V0 - 1, dtype=np.int32)
    assert any(0 in d for i, d in enumerate(base.docs) if i not in (0, n - 1))
    with pytest.raises(nat.NativeError, match="status -1.*mapped to -1"):
        g.remove(np.asarray([0, n - 1], np.int64), np.ones(V0 - 1), 3.0, term_map=tmap, carry=True)
    assert_unchanged(g, snap)
    # the handle still takes a good carrying call
    check(nat, g, apply(g, base, ("add", added, V0)), n)
    g.close()


def test_validation_holds_without_a_stream_too(nat, base):
    g = index_of(nat, base, tokens=False)
    added = [[1, 2, 3], [4], []]
    tp, pd, pt, dl = csr_of(added, V0)
    _, _, _, idf, _, avgdl = edited(base, ("add", added, V0)).postings()
    before = g.read()
    with pytest.raises(nat.NativeError, match="status -1"):
        g.add(tp, pd, pt, idf, dl, avgdl, tokens=(np.asarray([0, 2, 4, 4], np.int64), np.asarray([1, 2, 3, 4], np.int32)))
    same_arrays(g.read(), before)
    assert g.tokens_info() == (False, 0) and g.info()[3] == 0
    g.close()


# ---- the mixed sequence -------------------------------------------------------------------------------------------------
def ids_of(st, docs):
    return [[st.vocab[w] for w in d] for d in docs]


def test_the_mixed_sequence_carries_the_stream_through_every_step(nat):
    states = SQ.bm25_states()
    cur = PC.SeqCorpus("step0", len(states[0].vocab), ids_of(states[0], states[0].docs))
    g = index_of(nat, cur)  # the one set_tokens of this test
    prev = states[0]
    kinds = set()
    for st in states[1:]:
        if st.kind == "X":  # a refusal through the carrying form: nothing changes
            snap = snapshot(g)
            idf, n = cur.postings()[3], cur.n_docs
            with pytest.raises(nat.NativeError, match="status -1"):
                if st.op[1] == "remove id == n":
                    g.remove(np.asarray([0, n], np.int64), idf, 3.0, carry=True)
                elif st.op[1] == "remove every document":
                    g.remove(np.arange(n, dtype=np.int64), idf, 3.0, carry=True)
                else:
                    tp, pd, pt, dl = csr_of([[0, 1], [0]], cur.n_terms)
                    g.replace(np.asarray([3, 3], np.int64), tp, pd, pt, dl, idf, 3.0,
                              tokens=(np.asarray([0, 2, 3], np.int64), np.asarray([0, 1, 0], np.int32)))
            assert_unchanged(g, snap)
            continue
        tmap = np.asarray([st.vocab.get(w, -1) for w in prev.vocab], dtype=np.int32)
        v_new = len(st.vocab)
        if st.kind == "A":
            assert (tmap == np.arange(len(prev.vocab))).all()
            op = ("add", ids_of(st, st.op[1]), v_new)
        elif st.kind == "Rm":
            op = ("remove", list(st.op[1]), tmap, v_new)
        else:
            op = ("replace", list(st.op[1]), ids_of(st, st.op[2]), tmap, v_new)
        cur = apply(g, cur, op)
        assert cur.docs == ids_of(st, st.docs), st.note
        check_stream(g, cur)
        check_resolvers(g, cur, st.at)
        check_index(nat, g, cur)
        assert (g.info()[3], g.info()[5], g.replaces()) == (st.adds, st.removes, st.replaces), st.note
        prev = st
        kinds.add(st.kind)
    assert kinds == {"A", "Rm", "Rp"}
    g.close()

"""amdr_bm25_add: after any sequence of adds a BM25 handle is what amdr_bm25_create makes of the concatenated index — the
six resident arrays byte for byte, hence the same ids and score BITS from every entry point (csrc/bm25_update.hip).
`grown` is created from the first part and added to, `fresh` from the concatenation.  The add's arrays come from the
re-fit's own to_csr() cut by shard_csr, not from the code that add_documents uses; one test goes through add_documents
itself."""
import ctypes as C

import numpy as np
import pytest

from bm25_update_cases import (LENS, assert_same_results, assert_same_serving_step, fit, index_of, make_docs, nat,  # noqa: F401
                               queries_for, same_arrays, same_pair)

pytestmark = pytest.mark.gpu


def old_lead(i):
    return ["oldonly"] if i % 40 == 0 else []


def add_lead(i):
    return (["single"] if i == 0 else []) + [f"new{i % 5}"]


def parts_of(seed, n_base, adds):
    rng = np.random.default_rng(seed)
    return [make_docs(rng, n_base, old_lead)] + [make_docs(rng, n, add_lead) for n in adds]


def grow(nat, parts):
    """(grown, fresh, model of the concatenation): every add takes the re-fit's postings of its documents, the re-fit's
    idf vector and avgdl."""
    from legal_rag_amd.bm25_model import shard_csr
    g = index_of(nat, fit(parts[0]))
    docs = list(parts[0])
    model = None
    for p in parts[1:]:
        lo = len(docs)
        docs = docs + p
        model = fit(docs)
        term_ptr, post_doc, post_tf, idf, doc_len = model.to_csr()
        a_ptr, a_doc, a_tf, a_len = shard_csr(term_ptr, post_doc, post_tf, doc_len, lo, len(docs))
        g.add(a_ptr, a_doc, a_tf, idf, a_len, float(model.avgdl))
    return g, index_of(nat, model), model


def assert_same_state(g, f, adds):
    gi, fi = g.info(), f.info()
    assert gi[:3] == fi[:3] and gi[4] == fi[4] and gi[5] == fi[5] == 0 and gi[3] == adds and fi[3] == 0, (gi, fi)
    assert (g.n_docs, g.n_terms) == (f.n_docs, f.n_terms) == gi[:2]
    same_arrays(g.read(), f.read())


# base documents, adds: the smallest index; one arg-max slab of 2 048 becomes two; two adds in a row over that edge; the
# 4 096 staged slab
@pytest.mark.parametrize("n_base,adds", [(1, (1,)), (1500, (600,)), (2040, (8, 37)), (4090, (10,))],
                         ids=["1+1", "1500+600", "2040+8+37", "4090+10"])
def test_grown_equals_fresh(nat, n_base, adds):
    parts = parts_of(n_base, n_base, adds)
    g, f, model = grow(nat, parts)
    assert_same_state(g, f, len(adds))
    vocab = model.vocab()
    assert vocab["all"] == 0 and g.read()[0][1] == g.n_docs  # the term of every document
    n_old_terms = len(fit(parts[0]).idf)
    assert vocab["single"] >= n_old_terms and vocab["new4" if sum(adds) >= 5 else "new0"] >= n_old_terms
    tp = g.read()[0]
    assert tp[vocab["single"] + 1] - tp[vocab["single"]] == len(adds)  # one posting per add
    assert g.read()[1][tp[vocab["oldonly"]]:tp[vocab["oldonly"] + 1]].max() < n_base
    qs = queries_for(np.random.default_rng(1), len(vocab))
    assert_same_results(nat, g, f, qs, n_base)  # the seam
    assert_same_serving_step(nat, g, f, qs)
    g.close()
    f.close()


def test_every_add_size_changes_the_tile_residue(nat):
    """64 base documents + 1 ... 40: nnz takes many residues of the merge tile, every list grows at its tail."""
    rng = np.random.default_rng(64)
    base = make_docs(rng, 64, old_lead)
    pool = make_docs(rng, 40, add_lead)
    residues = set()
    for n_add in range(1, 41):
        g, f, model = grow(nat, [base, pool[:n_add]])
        assert_same_state(g, f, 1)
        residues.add(g.info()[2] % g.info()[4])
        qs = queries_for(rng, g.n_terms, 7)
        same_pair(g.search(qs, 10), f.search(qs, 10), n_add)
        if n_add in (1, 40):  # one slab: the serving step is ONE launch here
            assert_same_serving_step(nat, g, f, qs)
        g.close()
        f.close()
    assert len(residues) >= 30


def random_lists(rng, n_docs, dfs):
    """Term-major CSR with the given list lengths: random ascending documents, tf 1-9."""
    ptr = np.concatenate([[0], np.cumsum(dfs)]).astype(np.int64)
    doc = np.concatenate([np.sort(rng.choice(n_docs, size=int(df), replace=False)) for df in dfs] +
                         [np.zeros(0, np.int64)]).astype(np.int32)
    return ptr, doc, rng.integers(1, 10, size=doc.size).astype(np.int32)


def concat_csr(old, add, n_old):
    """The concatenated index, term by term: the old list, then the add's with n_old added."""
    (optr, odoc, otf), (aptr, adoc, atf) = old, add
    docs, tfs, ptr = [], [], [0]
    for t in range(len(aptr) - 1):
        lo, hi = (optr[t], optr[t + 1]) if t < len(optr) - 1 else (0, 0)
        docs += [odoc[lo:hi], adoc[aptr[t]:aptr[t + 1]] + n_old]
        tfs += [otf[lo:hi], atf[aptr[t]:aptr[t + 1]]]
        ptr.append(ptr[-1] + int(hi - lo) + int(aptr[t + 1] - aptr[t]))
    return np.asarray(ptr, np.int64), np.concatenate(docs).astype(np.int32), np.concatenate(tfs).astype(np.int32)


@pytest.mark.parametrize("extra,empty_terms", [(0, 0), (1, 0), (0, 2100)], ids=["tile-multiple", "one-more", "wide-window"])
def test_total_at_a_multiple_of_the_tile(nat, extra, empty_terms):
    """nnz_new is exactly 3 tiles (amdr_bm25_info's tile length), and one more; terms without postings are stepped over —
    2 100 of them in a row widen a tile's window of the term table beyond the kernel's LDS room."""
    rng = np.random.default_rng(7 + extra + empty_terms)
    n_old, n_add = 3000, 400
    old_dfs = [3000, 700, 50, 7, 0, 1]
    old = random_lists(rng, n_old, old_dfs)
    probe = nat.BM25Index(old[0], old[1], old[2], np.ones(6), np.full(n_old, 5, np.int32), 5.0)
    tile = probe.info()[4]
    probe.close()
    assert tile > 0
    add_dfs = [400, 0, 13, 40, 0, 2] + [0] * empty_terms + [5, 1]
    rest = 3 * tile + extra - sum(old_dfs) - sum(add_dfs)
    assert rest > 0
    while rest > 0:  # further new terms until the total is reached
        add_dfs.append(min(n_add, rest))
        rest -= add_dfs[-1]
    add = random_lists(rng, n_add, add_dfs)
    V = len(add_dfs)
    idf_old, idf_new = rng.uniform(0.1, 6.0, size=6), rng.uniform(0.1, 6.0, size=V)
    len_old = rng.choice(LENS, size=n_old).astype(np.int32)
    len_add = rng.choice(LENS, size=n_add).astype(np.int32)
    g = nat.BM25Index(old[0], old[1], old[2], idf_old, len_old, 21.5)
    g.add(add[0], add[1], add[2], idf_new, len_add, 19.25)
    whole = concat_csr(old, add, n_old)
    f = nat.BM25Index(whole[0], whole[1], whole[2], idf_new, np.concatenate([len_old, len_add]), 19.25)
    assert g.info()[2] == 3 * tile + extra
    assert_same_state(g, f, 1)
    qs = queries_for(rng, V, 9)
    same_pair(g.search(qs, 17), f.search(qs, 17), "search")
    g.close()
    f.close()


def test_scores_equal_the_oracle(nat):
    from oracle import bm25 as OB
    parts = parts_of(1500, 1500, (600,))
    g, f, model = grow(nat, parts)
    f.close()
    ob = OB.BM25Okapi(parts[0] + parts[1])
    queries = [["all", "z0", "new1"], ["z3", "z3", "z3", "z1"], ["nowhere", "z2"], ["single"], ["oldonly", "new0", "z7"],
               ["z0", "all", "z0", "all"], [], ["z399", "z12", "new4", "z5", "z1", "z0"]]
    got = g.get_scores([model.term_ids(q) for q in queries])
    for j, q in enumerate(queries):
        exp = np.asarray(ob.get_scores(q), dtype=np.float64)
        assert got[j].tobytes() == exp.tobytes(), (j, q)
    g.close()


def test_add_documents_appends_to_the_resident_index(nat):
    """The host model's own route: BM25Okapi.add_documents on an object with a resident index."""
    parts = parts_of(3, 300, (30, 1))
    m = fit(parts[0])
    g = m.gpu(0)
    m.add_documents(parts[1])
    m.add_documents(parts[2])
    assert m.gpu(0) is g
    whole = fit(parts[0] + parts[1] + parts[2])
    f = index_of(nat, whole)
    assert_same_state(g, f, 2)
    q = ["all", "new0", "z1", "single", "nowhere"]
    a, b = m.top_k(q, 10), whole.top_k(q, 10)
    assert np.array_equal(a[1], b[1]) and a[0].tobytes() == b[0].tobytes()
    assert_same_serving_step(nat, g, f, queries_for(np.random.default_rng(2), g.n_terms, 4))
    f.close()


def test_bad_arguments_leave_the_handle_unchanged(nat):
    lib = nat.load()
    rng = np.random.default_rng(5)
    old = random_lists(rng, 50, [50, 20, 3])
    g = nat.BM25Index(old[0], old[1], old[2], np.asarray([0.3, 1.0, 2.5]), np.full(50, 7, np.int32), 7.0)
    before = g.read()
    assert g.add_kernel_ms() == -1.0  # no add yet
    ptr = np.asarray([0, 2, 2, 3, 4], np.int64)
    doc = np.asarray([0, 1, 1, 0], np.int32)
    tf = np.asarray([1, 2, 3, 1], np.int32)
    idf = np.asarray([0.3, 1.1, 2.0, 4.0])
    dl = np.asarray([4, 5], np.int32)

    def call(h=None, ptr=ptr, doc=doc, tf=tf, idf=idf, dl=dl, n_terms=4, n_add=2, avgdl=6.5):
        p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
        return lib.amdr_bm25_add(g._h if h is None else h, p(ptr, C.c_int64), p(doc, C.c_int32), p(tf, C.c_int32),
                                 p(idf, C.c_double), p(dl, C.c_int32), C.c_int64(n_terms), C.c_int64(n_add), C.c_double(avgdl))

    i64 = lambda *v: np.asarray(v, np.int64)  # noqa: E731
    i32 = lambda *v: np.asarray(v, np.int32)  # noqa: E731
    bad = {
        "null handle": dict(h=C.c_void_p()),
        "null term_ptr_add": dict(ptr=None), "null post_doc_add": dict(doc=None), "null post_tf_add": dict(tf=None),
        "null idf": dict(idf=None), "null doc_len_add": dict(dl=None),
        "n_add < 0": dict(n_add=-1),
        "n_terms below the handle's": dict(ptr=i64(0, 2, 3), idf=idf[:2].copy(), n_terms=2),
        "term_ptr_add[0] != 0": dict(ptr=i64(1, 2, 2, 3, 4)),
        "term_ptr_add not monotone": dict(ptr=i64(0, 2, 1, 3, 4)),
        "document n_add": dict(doc=i32(0, 2, 1, 0)), "document -1": dict(doc=i32(-1, 1, 1, 0)),
        "a repeated document": dict(doc=i32(1, 1, 1, 0)), "descending documents": dict(doc=i32(1, 0, 1, 0)),
        "infinite idf": dict(idf=np.asarray([0.3, np.inf, 2.0, 4.0])), "NaN idf": dict(idf=np.asarray([0.3, 1.1, 2.0, np.nan])),
        "avgdl 0": dict(avgdl=0.0), "avgdl < 0": dict(avgdl=-3.0), "avgdl inf": dict(avgdl=np.inf), "avgdl NaN": dict(avgdl=np.nan),
        "2^31 documents": dict(n_add=(1 << 31) - 50),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert nat.load().amdr_last_error(), what
        same_arrays(g.read(), before)
        assert g.info()[3] == 0, what
    # n_add == 0 reads nothing
    assert call(ptr=None, doc=None, tf=None, idf=None, dl=None, n_add=0) == 0
    same_arrays(g.read(), before)
    assert g.info()[:4] == (50, 3, 73, 0) and g.add_kernel_ms() == -1.0
    s0 = g.search([[0, 1, 2]], 5)
    # and the good add goes through afterwards: the handle was left searchable
    assert call() == 0
    assert g.info()[:4] == (52, 4, 77, 1) and g.add_kernel_ms() > 0
    whole = concat_csr(old, (ptr, doc, tf), 50)
    f = nat.BM25Index(whole[0], whole[1], whole[2], idf, np.concatenate([np.full(50, 7, np.int32), dl]), 6.5)
    same_arrays(g.read(), f.read())
    assert s0[1].shape == (1, 5)
    g.close()
    f.close()

"""amdr_bm25_replace: after a replace a BM25 handle is what amdr_bm25_create makes of the edited index — the six resident
arrays byte for byte, hence the same ids and score BITS from every entry point (csrc/bm25_update.hip,
csrc/bm25_replace_rule.hpp).  `edited` is created from the whole corpus and replaced in, `fresh` from the re-fit of the
edited corpus in its original order (or, for hand-built lists, from a brute-force merge).  The replace's arguments come
from the re-fit itself (its idf vector, avgdl, vocabulary), not from the code that replace_documents uses; one test goes
through replace_documents itself."""
import ctypes as C

import numpy as np
import pytest

from bm25_update_cases import (LENS, assert_same_results, assert_same_serving_step, fit, index_of, make_docs, nat,  # noqa: F401
                               queries_for, same_arrays, same_pair)
from legal_rag_amd.bm25_model import docs_csr

pytestmark = pytest.mark.gpu


def only_lead(i):
    """Terms that live in one document each (they vanish with it), one in every 40th, and one in documents 100 .. 110."""
    return ([f"only{i}"] if i % 7 == 0 else []) + (["forty"] if i % 40 == 0 else []) + (["mid"] if 100 <= i <= 110 else [])


def put(docs, ids, new):
    out = list(docs)
    for i, d in zip(ids, new):
        out[i] = d
    return out


def freqs_of(doc):
    f = {}
    for w in doc:
        f[w] = f.get(w, 0) + 1
    return f


def replace_in(g, old_model, docs, ids, new):
    """Replace documents `ids` (ascending) of handle g (which holds old_model = the fit of docs) by `new`, with the
    re-fit's statistics; returns the edited documents and their fit."""
    assert list(ids) == sorted(ids)
    after = put(docs, ids, new)
    model = fit(after)
    nv = model.vocab()
    tm = np.asarray([nv.get(w, -1) for w in old_model.vocab()], dtype=np.int32)
    tp, pd, pt = docs_csr([freqs_of(d) for d in new], nv)
    g.replace(np.asarray(ids, np.int64), tp, pd, pt, np.asarray([len(d) for d in new], np.int32), model.to_csr()[3],
              float(model.avgdl), term_map=tm)
    return after, model


def assert_same_state(g, f, replaces, adds=0, removes=0):
    gi, fi = g.info(), f.info()
    assert gi[:3] == fi[:3] and gi[4] == fi[4] and gi[3] == adds and gi[5] == removes and fi[3] == fi[5] == 0, (gi, fi)
    assert g.replaces() == replaces and f.replaces() == 0
    assert (g.n_docs, g.n_terms) == (f.n_docs, f.n_terms) == gi[:2]
    same_arrays(g.read(), f.read())
    tp, pd = g.read()[:2]
    for t in range(len(tp) - 1):  # each list ascending
        assert np.all(np.diff(pd[tp[t]:tp[t + 1]]) > 0), t


def new_docs(rng, count, lead=lambda i: ()):
    return make_docs(rng, count, lead)


@pytest.mark.parametrize("n,ids", [(1, [0]), (1500, [700]), (1500, sorted(np.random.default_rng(1).choice(1500, 37, replace=False).tolist())),
                                   (300, list(range(300))), (2049, [0, 2048])],
                         ids=["1-of-1", "1-of-1500", "37-of-1500", "all-300", "2049-ends"])
def test_edited_equals_fresh(nat, n, ids):
    rng = np.random.default_rng(n + len(ids))
    docs = make_docs(rng, n, only_lead)
    new = new_docs(rng, len(ids), lambda i: ([f"new{i % 5}"] if i % 2 == 0 else []) + (["mid"] if i in (0, len(ids) - 1) else []))
    whole = fit(docs)
    g = index_of(nat, whole)
    assert g.replace_kernel_ms() == -1.0 and g.replaces() == 0
    after, model = replace_in(g, whole, docs, ids, new)
    assert g.replace_kernel_ms() >= 0.0
    f = index_of(nat, model)
    assert_same_state(g, f, 1)
    assert "new0" in model.vocab() and "new0" not in whole.vocab()  # a new term
    qs = queries_for(np.random.default_rng(1), len(model.vocab()))
    assert_same_results(nat, g, f, qs, ids[0])
    assert_same_serving_step(nat, g, f, qs)
    g.close()
    f.close()


def test_a_head_list_across_three_tiles_with_replacements_at_the_tile_edges(nat):
    """"all" is in every document, so its list is postings 0 .. n-1 and spans three tiles and more; the replaced documents
    sit at the first and the last posting of every tile.  Half of the new documents keep "all", half lose it (those are
    one-token documents); "mid" lives in documents 100 .. 110, and the new documents 0 and n-1 bring it: an add posting
    before the list's first and one after its last old posting."""
    probe = index_of(nat, fit([["a"]]))
    tile = probe.info()[4]
    probe.close()
    n = 3 * tile + 100
    rng = np.random.default_rng(3)
    docs = make_docs(rng, n, only_lead)
    ids = [0, tile - 1, tile, 2 * tile - 1, 2 * tile, 3 * tile - 1, 3 * tile, n - 1]
    new = [["all", "mid", "z1"], ["solo-token"], ["all", "z0", "z0"], ["z2"], ["all"], ["all", "fresh", "fresh"], ["z0"],
           ["all", "z3", "mid"]]
    whole = fit(docs)
    g = index_of(nat, whole)
    after, model = replace_in(g, whole, docs, ids, new)
    f = index_of(nat, model)
    assert_same_state(g, f, 1)
    tp, pd = g.read()[:2]
    v = model.vocab()
    assert v["all"] == 0 and tp[1] == n - 3 and tp[1] > 3 * tile - 3  # three of the new documents lost "all"
    mid = pd[tp[v["mid"]]:tp[v["mid"] + 1]]
    assert mid[0] == 0 and mid[-1] == n - 1 and mid.size == 13
    qs = queries_for(np.random.default_rng(2), g.n_terms, 9)
    qs[3] = [v["mid"], v["all"], v["fresh"]]
    same_pair(g.search(qs, 17), f.search(qs, 17), "search")
    assert g.get_scores(qs[:4]).tobytes() == f.get_scores(qs[:4]).tobytes()
    g.close()
    f.close()


def merged(old, ids, add_pre, new_of, V_new):
    """The edited index, plainly: per pre-map term the surviving old (document, tf) pairs and the add's pairs at
    ids[local], sorted by document; the terms placed at their new ids."""
    optr, odoc, otf = old
    gone = np.zeros(int(odoc.max(initial=0)) + int(ids.max()) + 2, dtype=bool)
    gone[ids] = True
    lists = [(np.zeros(0, np.int64), np.zeros(0, np.int64))] * V_new
    for t, (loc, tf) in enumerate(add_pre):
        d, f = np.zeros(0, np.int64), np.zeros(0, np.int64)
        if t < len(optr) - 1:
            d, f = odoc[optr[t]:optr[t + 1]].astype(np.int64), otf[optr[t]:optr[t + 1]].astype(np.int64)
            keep = ~gone[d]
            d, f = d[keep], f[keep]
        d, f = np.concatenate([d, ids[loc]]), np.concatenate([f, tf])
        order = np.argsort(d, kind="stable")
        if new_of[t] >= 0:
            lists[new_of[t]] = (d[order], f[order])
        else:
            assert d.size == 0
    ptr = np.concatenate([[0], np.cumsum([len(x[0]) for x in lists])]).astype(np.int64)
    return (ptr, np.concatenate([x[0] for x in lists]).astype(np.int32), np.concatenate([x[1] for x in lists]).astype(np.int32))


@pytest.mark.parametrize("null_map", [False, True], ids=["permuted-map", "null-map"])
@pytest.mark.parametrize("shape", ["tile-1", "tile", "tile+1", "3-tiles+5", "empty-run"])
def test_hand_built_lists(nat, shape, null_map):
    """nnz_old is exactly a tile less one, a tile, a tile and one, three tiles and five (amdr_bm25_info's tile length);
    2 100 consecutive terms without postings widen a tile's window of the old AND of the add's term table beyond the
    kernels' LDS room.  Term 1's documents are all replaced and no new document holds it: emptied — it keeps its id with
    an empty list under the null map and is dropped by the other, which also reverses the order of all terms (new terms
    in front).  Term 2's documents are all replaced and new documents hold it: its list comes from the add alone.  Term 3
    holds documents 100 .. 199 and gets add postings at documents 3 and n - 1: before its first and after its last."""
    rng = np.random.default_rng(11 + len(shape) + 10 * null_map)
    probe = index_of(nat, fit([["a"]]))
    tile = probe.info()[4]
    probe.close()
    n = 700
    ids = np.asarray(sorted({3, n - 1} | set(rng.choice(n, size=60, replace=False).tolist())), dtype=np.int64)
    n_rep = ids.size
    local_of = {int(d): i for i, d in enumerate(ids)}
    stay = np.setdiff1d(np.arange(n), ids)
    olists = [np.arange(n), rng.choice(ids, size=9, replace=False), rng.choice(ids, size=5, replace=False), np.arange(100, 200),
              rng.choice(n, size=300, replace=False)]
    if shape == "empty-run":
        olists += [np.zeros(0, np.int64)] * 2100 + [rng.choice(n, size=40, replace=False), rng.choice(stay, size=3, replace=False)]
    else:
        want = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "3-tiles+5": 3 * tile + 5}[shape]
        rest = want - sum(len(x) for x in olists)
        assert rest > 0
        while rest > 0:
            olists.append(rng.choice(n, size=min(rest, int(rng.integers(1, 500))), replace=False))
            rest -= len(olists[-1])
    olists = [np.sort(np.asarray(x, dtype=np.int64)) for x in olists]
    V_old = len(olists)
    optr = np.concatenate([[0], np.cumsum([x.size for x in olists])]).astype(np.int64)
    odoc = np.concatenate(olists).astype(np.int32)
    otf = rng.integers(1, 10, size=odoc.size).astype(np.int32)
    if shape != "empty-run":
        assert optr[-1] == want
    # the add over the pre-map terms: the old ones and 4 new ones (the last of them unused)
    fresh_terms = 4
    V_pre = V_old + fresh_terms
    picks = {0: rng.choice(n_rep, size=n_rep // 2, replace=False), 2: rng.choice(n_rep, size=7, replace=False),
             3: np.asarray([local_of[3], local_of[n - 1]]), 4: rng.choice(n_rep, size=20, replace=False),
             V_old - 1: rng.choice(n_rep, size=3, replace=False), V_old: rng.choice(n_rep, size=n_rep // 3, replace=False),
             V_old + 1: np.asarray([0]), V_old + 2: np.asarray([n_rep - 1])}
    add_pre = []
    for t in range(V_pre):
        loc = np.sort(np.asarray(picks.get(t, []), dtype=np.int64))
        add_pre.append((loc, rng.integers(1, 10, size=loc.size).astype(np.int64)))
    alive = np.asarray([(t < V_old and np.setdiff1d(olists[t], ids).size > 0) or add_pre[t][0].size > 0 for t in range(V_pre)])
    assert not alive[1] and alive[2] and not alive[V_pre - 1]
    if null_map:
        new_of, V_new, term_map = np.arange(V_pre), V_pre, None
    else:
        V_new = int(alive.sum())
        new_of = np.where(alive, V_new - np.cumsum(alive), -1)
        term_map = new_of[:V_old].astype(np.int32)
    pre_of = np.full(V_new, -1)
    pre_of[new_of[new_of >= 0]] = np.nonzero(new_of >= 0)[0]
    add_ptr = np.concatenate([[0], np.cumsum([add_pre[t][0].size for t in pre_of])]).astype(np.int64)
    add_doc = np.concatenate([add_pre[t][0] for t in pre_of]).astype(np.int32)
    add_tf = np.concatenate([add_pre[t][1] for t in pre_of]).astype(np.int32)
    idf_old, idf_new = rng.uniform(0.1, 6.0, size=V_old), rng.uniform(0.1, 6.0, size=V_new)
    len_old = rng.choice(LENS, size=n).astype(np.int32)
    len_add = rng.choice(LENS, size=n_rep).astype(np.int32)
    len_new = len_old.copy()
    len_new[ids] = len_add
    g = nat.BM25Index(optr, odoc, otf, idf_old, len_old, 21.5)
    g.replace(ids, add_ptr, add_doc, add_tf, len_add, idf_new, 19.25, term_map=term_map)
    eptr, edoc, etf = merged((optr, odoc, otf), ids, add_pre, new_of, V_new)
    f = nat.BM25Index(eptr, edoc, etf, idf_new, len_new, 19.25)
    assert_same_state(g, f, 1)
    tp = g.read()[0]
    if null_map:
        assert tp[2] == tp[1] and tp[V_pre] == tp[V_pre - 1]  # the emptied term and the unused new term: empty lists
    assert tp[new_of[2] + 1] - tp[new_of[2]] == 7  # from the add alone
    pd = g.read()[1]
    l3 = pd[tp[new_of[3]]:tp[new_of[3] + 1]]
    assert l3[0] == 3 and l3[-1] == n - 1
    qs = queries_for(rng, V_new, 9)
    qs[3] = [int(new_of[2]), int(new_of[3]), int(new_of[V_old])]
    same_pair(g.search(qs, 17), f.search(qs, 17), "search")
    assert g.get_scores(qs[:4]).tobytes() == f.get_scores(qs[:4]).tobytes()
    g.close()
    f.close()


def test_replace_after_add_after_remove_and_twice(nat):
    rng = np.random.default_rng(5)
    docs = make_docs(rng, 400, only_lead)
    more = make_docs(rng, 60, lambda i: ["added", f"m{i}"])
    m = fit(docs)
    g = m.gpu(0)
    m.add_documents(more)
    docs = docs + more
    ids = [0, 7, 399, 400, 459]
    new = new_docs(rng, 5, lambda i: [f"r{i}"])
    assert m.replace_documents(ids, new) == 5  # the host model's own route
    docs = put(docs, ids, new)
    f = index_of(nat, fit(docs))
    assert m.gpu(0) is g
    assert_same_state(g, f, 1, adds=1)
    f.close()
    m.remove_documents([0, 400])
    docs = [d for i, d in enumerate(docs) if i not in (0, 400)]
    ids2 = [457, 0, 6]  # unsorted; document 6 was replaced before (old id 7)
    new2 = [["all", "r0", "again"], ["one"], ["all", "again", "again", "z0"]]
    m.replace_documents(ids2, new2)
    m.replace_documents([6], [["all", "third"]])  # two replaces in a row
    docs = put(put(docs, ids2, new2), [6], [["all", "third"]])
    whole = fit(docs)
    f = index_of(nat, whole)
    assert_same_state(g, f, 3, adds=1, removes=1)
    assert "only0" not in whole.vocab() and "third" in whole.vocab() and "again" in whole.vocab()
    qs = queries_for(np.random.default_rng(6), g.n_terms)
    assert_same_results(nat, g, f, qs, 6)
    q = ["all", "again", "z1", "third", "nowhere"]
    a, b = m.top_k(q, 10), whole.top_k(q, 10)
    assert np.array_equal(a[1], b[1]) and a[0].tobytes() == b[0].tobytes()
    f.close()


def test_scores_equal_the_oracle(nat):
    from oracle import bm25 as OB
    rng = np.random.default_rng(8)
    docs = make_docs(rng, 1500, only_lead)
    ids = sorted(np.random.default_rng(9).choice(1500, 200, replace=False).tolist()) + [1499]
    ids = sorted(set(ids) | {0})
    new = new_docs(rng, len(ids), lambda i: [f"new{i % 5}", "mid"] if i % 4 == 0 else [])
    whole = fit(docs)
    g = index_of(nat, whole)
    after, model = replace_in(g, whole, docs, ids, new)
    ob = OB.BM25Okapi(after)
    queries = [["all", "z0", "new1"], ["z3", "z3", "z3", "z1"], ["nowhere", "z2"], ["mid"], ["only0", "new0", "z7"],
               ["z0", "all", "z0", "all"], [], ["z399", "z12", "new4", "z5", "z1", "z0"]]
    got = g.get_scores([model.term_ids(q) for q in queries])
    for j, q in enumerate(queries):
        exp = np.asarray(ob.get_scores(q), dtype=np.float64)
        assert got[j].tobytes() == exp.tobytes(), (j, q)
    s, i = g.search([model.term_ids(q) for q in queries], 10)
    for j, q in enumerate(queries):
        exp = OB.search(ob, q, 10)
        assert i[j].tolist() == [d for d, _ in exp] and s[j].tobytes() == np.asarray([x for _, x in exp]).tobytes(), (j, q)
    g.close()


def test_bad_arguments_leave_the_handle_as_it_was(nat):
    """Every AMDR_EINVAL of the header, the device-detected one included: amdr_bm25_read is unchanged afterwards."""
    optr = np.asarray([0, 2, 3, 4], np.int64)
    odoc = np.asarray([0, 1, 0, 3], np.int32)
    otf = np.asarray([1, 1, 2, 1], np.int32)
    g = nat.BM25Index(optr, odoc, otf, np.asarray([1.0, 0.5, 2.0]), np.asarray([3, 3, 3, 3, 3], np.int32), 3.0)
    before = g.read()
    lib = nat.load()
    good = dict(ids=[1, 3], ptr=[0, 1, 3, 3], doc=[0, 0, 1], tf=[2, 1, 1], lens=[4, 5], map=[1, 0, -1], vn=3,
                idf=[1.0, 0.5, 2.0], avgdl=4.5, n_rep=2, h=g._h)

    def raw(**kw):
        a = dict(good, **kw)
        arr = lambda x, t: None if x is None else np.ascontiguousarray(x, dtype=t)  # noqa: E731
        ids, ptr, doc, tf = arr(a["ids"], np.int64), arr(a["ptr"], np.int64), arr(a["doc"], np.int32), arr(a["tf"], np.int32)
        lens, tm, idf = arr(a["lens"], np.int32), arr(a["map"], np.int32), arr(a["idf"], np.float64)
        p = lambda x, t: None if x is None else x.ctypes.data_as(C.POINTER(t))  # noqa: E731
        nat._check(lib.amdr_bm25_replace(a["h"], p(ids, C.c_int64), C.c_int64(a["n_rep"]), p(ptr, C.c_int64), p(doc, C.c_int32),
                                         p(tf, C.c_int32), p(lens, C.c_int32), p(tm, C.c_int32), C.c_int64(a["vn"]),
                                         p(idf, C.c_double), C.c_double(a["avgdl"])), "amdr_bm25_replace")

    inf, nan = float("inf"), float("nan")
    bad = [dict(h=None), dict(n_rep=-1), dict(ids=None), dict(ptr=None), dict(doc=None), dict(tf=None), dict(lens=None),
           dict(idf=None), dict(n_rep=6, ids=[0, 1, 2, 3, 4, 5]), dict(ids=[1, 5]), dict(ids=[-1, 3]), dict(ids=[3, 3]),
           dict(ids=[3, 1]), dict(vn=-1), dict(map=None, vn=2, idf=[1.0, 0.5], ptr=[0, 1, 3]), dict(map=[1, 3, 0]),
           dict(map=[1, -2, 0]), dict(map=[1, 1, 0]), dict(ptr=[1, 1, 3, 3]), dict(ptr=[0, 2, 1, 3]), dict(doc=[0, 0, 2]),
           dict(doc=[0, -1, 1]), dict(doc=[0, 1, 1]), dict(doc=[0, 1, 0]), dict(idf=[1.0, inf, 1.0]), dict(idf=[nan, 0.5, 1.0]),
           dict(avgdl=0.0), dict(avgdl=-1.0), dict(avgdl=inf), dict(avgdl=nan),
           # what only the device sees: term 1 is mapped to -1 but document 0 survives in its list
           dict(map=[1, -1, 0])]
    for kw in bad:
        with pytest.raises(nat.NativeError, match="status -1"):
            raw(**kw)
        same_arrays(g.read(), before)
        assert g.replaces() == 0 and g.replace_kernel_ms() == -1.0
    raw(n_rep=0, ids=None, ptr=None, doc=None, tf=None, lens=None, idf=None, map=None)  # a no-op that reads nothing
    same_arrays(g.read(), before)
    raw()  # and the good call goes through: term 2's only document (3) is replaced
    # new term 0 = old term 1's survivor (document 0) + document 1; new term 1 = old term 0's survivor + documents 1, 3;
    # new term 2 has no old term and no posting
    f = nat.BM25Index(np.asarray([0, 2, 5, 5], np.int64), np.asarray([0, 1, 0, 1, 3], np.int32),
                      np.asarray([2, 2, 1, 1, 1], np.int32), np.asarray([1.0, 0.5, 2.0]), np.asarray([3, 4, 3, 5, 3], np.int32), 4.5)
    same_arrays(g.read(), f.read())
    assert g.replaces() == 1
    g.close()
    f.close()

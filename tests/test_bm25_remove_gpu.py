"""amdr_bm25_remove: after any sequence of adds and removes a BM25 handle is what amdr_bm25_create makes of the surviving
documents' index — the six resident arrays byte for byte, hence the same ids and score BITS from every entry point
(csrc/bm25_update.hip).  `shrunk` is created from the whole corpus and removed from, `fresh` from the survivors' re-fit.
The remove's arguments come from the re-fit itself (its idf vector, avgdl and the map old vocabulary -> its vocabulary),
not from the code that remove_documents uses; one test goes through remove_documents itself."""
import ctypes as C

import numpy as np
import pytest

from bm25_update_cases import (LENS, assert_same_results, assert_same_serving_step, fit, index_of, make_docs, nat,  # noqa: F401
                               queries_for, same_arrays, same_pair)

pytestmark = pytest.mark.gpu


def only_lead(i):
    """Terms that live in one document each (they vanish with it), and one in every 40th."""
    return ([f"only{i}"] if i % 7 == 0 else []) + (["forty"] if i % 40 == 0 else [])


def survivors(docs, ids):
    gone = set(int(i) for i in ids)
    return [d for i, d in enumerate(docs) if i not in gone]


def term_map_of(old_vocab, new_vocab):
    tm = np.full(len(old_vocab), -1, dtype=np.int32)
    for w, t in new_vocab.items():
        tm[old_vocab[w]] = t
    return tm


def remove_from(g, old_model, docs, ids):
    """Remove `ids` from handle g (which holds old_model = the fit of docs) with the re-fit's statistics; returns the
    surviving documents, their fit and the term map."""
    left = survivors(docs, ids)
    model = fit(left)
    tm = term_map_of(old_model.vocab(), model.vocab())
    g.remove(np.asarray(sorted(ids), np.int64), model.to_csr()[3], float(model.avgdl), term_map=tm)
    return left, model, tm


def shrink(nat, docs, ids):
    """(shrunk, fresh, model of the survivors, term map)."""
    whole = fit(docs)
    g = index_of(nat, whole)
    left, model, tm = remove_from(g, whole, docs, ids)
    return g, index_of(nat, model), model, tm


def assert_same_state(g, f, removes, adds=0):
    gi, fi = g.info(), f.info()
    assert gi[:3] == fi[:3] and gi[4] == fi[4] and gi[5] == removes and fi[5] == 0 and gi[3] == adds and fi[3] == 0, (gi, fi)
    assert (g.n_docs, g.n_terms) == (f.n_docs, f.n_terms) == gi[:2]
    same_arrays(g.read(), f.read())
    tp, pd = g.read()[:2]
    for t in range(len(tp) - 1):  # each list ascending
        assert np.all(np.diff(pd[tp[t]:tp[t + 1]]) > 0), t


def first_gap(ids):
    """New id of the first survivor behind the first removed document."""
    return int(min(ids))


def spread(n, count, seed):
    return sorted(np.random.default_rng(seed).choice(n, size=count, replace=False).tolist())


# the smallest index; a removal spread over the corpus; 2 049 -> 2 048 (the arg-max slab edge) and 4 097 -> 4 096 (the
# staged slab edge)
@pytest.mark.parametrize("n,ids", [(2, [0]), (1500, spread(1500, 600, 1)), (2049, [1024]), (4097, [4096])],
                         ids=["2-1", "1500-600", "2049-1", "4097-1"])
def test_shrunk_equals_fresh(nat, n, ids):
    docs = make_docs(np.random.default_rng(n), n, only_lead)
    g, f, model, tm = shrink(nat, docs, ids)
    assert_same_state(g, f, 1)
    vocab = model.vocab()
    assert vocab["all"] == 0 and g.read()[0][1] == g.n_docs == n - len(ids)  # the term of every document
    if 0 in ids:
        assert "only0" not in vocab and (tm == -1).sum() >= 1  # a term that left with its only document
    qs = queries_for(np.random.default_rng(1), len(vocab))
    assert_same_results(nat, g, f, qs, first_gap(ids))
    assert_same_serving_step(nat, g, f, qs)
    g.close()
    f.close()


def test_every_remove_size_changes_the_tile_residue(nat):
    """64 documents, the first 1 ... 40 removed: nnz takes many residues of the tile, every list shrinks at its head, the
    vocabulary's first-seen order changes."""
    rng = np.random.default_rng(64)
    docs = make_docs(rng, 64, only_lead)
    residues, not_monotone = set(), 0
    for k in range(1, 41):
        g, f, model, tm = shrink(nat, docs, list(range(k)))
        assert_same_state(g, f, 1)
        residues.add(g.info()[2] % g.info()[4])
        kept = tm[tm >= 0]
        not_monotone += int(not np.all(np.diff(kept) > 0))
        qs = queries_for(rng, g.n_terms, 7)
        same_pair(g.search(qs, 10), f.search(qs, 10), k)
        if k in (1, 40):  # one slab: the serving step is ONE launch here
            assert_same_serving_step(nat, g, f, qs)
        g.close()
        f.close()
    assert len(residues) >= 30 and not_monotone >= 1


@pytest.mark.parametrize("which", ["every-other", "first-2100", "last"])
def test_a_list_across_two_tile_borders(nat, which):
    """4 100 documents: the list of "all" is postings 0 .. 4 099, across the tile borders at 2 048 and 4 096.  Removing
    documents 0 .. 2 099 leaves its whole first tile without a survivor."""
    n = 4100
    docs = make_docs(np.random.default_rng(41), n, only_lead)
    ids = {"every-other": list(range(1, n, 2)), "first-2100": list(range(2100)), "last": [n - 1]}[which]
    g, f, model, tm = shrink(nat, docs, ids)
    tile = g.info()[4]
    assert 2 * tile < n
    assert_same_state(g, f, 1)
    tp = g.read()[0]
    assert tp[0] == 0 and tp[1] == n - len(ids)
    qs = queries_for(np.random.default_rng(2), g.n_terms, 9)
    same_pair(g.search(qs, 17), f.search(qs, 17), "search")
    assert g.get_scores(qs[:3]).tobytes() == f.get_scores(qs[:3]).tobytes()
    g.close()
    f.close()


def lists_with(rng, kept_pool, gone_pool, kept_counts, gone_counts):
    """Term-major CSR (random_lists style): list t holds kept_counts[t] random documents of kept_pool and gone_counts[t]
    of gone_pool, ascending, tf 1-9."""
    docs = [np.sort(np.concatenate([rng.choice(kept_pool, size=int(a), replace=False),
                                    rng.choice(gone_pool, size=int(b), replace=False)]))
            for a, b in zip(kept_counts, gone_counts)]
    ptr = np.concatenate([[0], np.cumsum([d.size for d in docs])]).astype(np.int64)
    doc = np.concatenate(docs + [np.zeros(0, np.int64)]).astype(np.int32)
    return ptr, doc, rng.integers(1, 10, size=doc.size).astype(np.int32)


def filtered_csr(old, doc_new, term_map, n_terms_new):
    """The survivors' index, plainly: per old term the kept postings with renumbered documents, then a stable reorder by
    new term id."""
    optr, odoc, otf = old
    lists = [None] * n_terms_new
    for t in range(len(optr) - 1):
        d, tf = odoc[optr[t]:optr[t + 1]], otf[optr[t]:optr[t + 1]]
        keep = doc_new[d] >= 0
        if term_map[t] >= 0:
            lists[term_map[t]] = (doc_new[d[keep]], tf[keep])
        else:
            assert not keep.any()
    ptr = np.concatenate([[0], np.cumsum([len(x[0]) for x in lists])]).astype(np.int64)
    return (ptr, np.concatenate([x[0] for x in lists] + [np.zeros(0, np.int32)]).astype(np.int32),
            np.concatenate([x[1] for x in lists] + [np.zeros(0, np.int32)]).astype(np.int32))


@pytest.mark.parametrize("null_map", [False, True], ids=["permuted-map", "null-map"])
@pytest.mark.parametrize("extra,emptied", [(0, 0), (1, 0), (0, 2100)], ids=["3-tiles", "one-more", "emptied-run"])
def test_hand_built_lists(nat, extra, emptied, null_map):
    """nnz_old is exactly 3 tiles (amdr_bm25_info's tile length), and one more, with nnz_new exactly 2 tiles; 2 100
    consecutive terms without postings widen a tile's window of the OLD term table beyond the kernel's LDS room, and
    2 100 consecutive terms that lose their only posting leave such a run behind (null map) or are dropped by a
    non-monotone map."""
    rng = np.random.default_rng(7 + extra + emptied + 10 * null_map)
    n_old = 3000
    all_docs = np.arange(n_old)
    gone_pool, kept_pool = all_docs[all_docs % 3 == 2], all_docs[all_docs % 3 != 2]
    probe = nat.BM25Index(np.asarray([0, 1], np.int64), np.zeros(1, np.int32), np.ones(1, np.int32), np.ones(1),
                          np.full(1, 5, np.int32), 5.0)
    tile = probe.info()[4]
    probe.close()
    assert tile > 0
    kept_counts = [2000, 1000, 50, 0, 7, 0, 1] + [0] * 2100 + [5, 1]
    gone_counts = [1000, 700, 0, 13, 0, 0, 2] + [0] * 2100 + [0, 1]
    if emptied:  # a run of terms whose only posting is in a removed document
        kept_counts += [0] * emptied + [3]
        gone_counts += [1] * emptied + [0]
        rest_k, rest_g = 0, 0
    else:  # further terms until nnz_old = 3 tiles (+ extra) and nnz_new = 2 tiles
        rest_k, rest_g = 2 * tile - sum(kept_counts), tile + extra - sum(gone_counts)
        assert rest_k > 0 and rest_g > 0
    while rest_k > 0 or rest_g > 0:
        a, b = min(rest_k, len(kept_pool)), min(rest_g, len(gone_pool))
        kept_counts.append(a)
        gone_counts.append(b)
        rest_k, rest_g = rest_k - a, rest_g - b
    old = lists_with(rng, kept_pool, gone_pool, kept_counts, gone_counts)
    V_old = len(kept_counts)
    doc_new = np.where(all_docs % 3 == 2, -1, np.cumsum(all_docs % 3 != 2) - 1).astype(np.int32)
    if null_map:
        term_map, V_new = np.arange(V_old, dtype=np.int32), V_old
    else:  # terms without a survivor dropped, the rest in reverse order
        alive = np.asarray(kept_counts) > 0
        V_new = int(alive.sum())
        term_map = np.where(alive, V_new - np.cumsum(alive), -1).astype(np.int32)
        assert sorted(term_map[alive].tolist()) == list(range(V_new)) and not np.all(np.diff(term_map[alive]) > 0)
    idf_old, idf_new = rng.uniform(0.1, 6.0, size=V_old), rng.uniform(0.1, 6.0, size=V_new)
    len_old = rng.choice(LENS, size=n_old).astype(np.int32)
    g = nat.BM25Index(old[0], old[1], old[2], idf_old, len_old, 21.5)
    if not emptied:
        assert g.info()[2] == 3 * tile + extra
    g.remove(gone_pool.astype(np.int64), idf_new, 19.25, term_map=None if null_map else term_map)
    new = filtered_csr(old, doc_new, term_map, V_new)
    f = nat.BM25Index(new[0], new[1], new[2], idf_new, len_old[all_docs % 3 != 2], 19.25)
    if not emptied:
        assert g.info()[2] == 2 * tile
    assert_same_state(g, f, 1)
    qs = queries_for(rng, V_new, 9)
    same_pair(g.search(qs, 17), f.search(qs, 17), "search")
    g.close()
    f.close()


def test_remove_add_remove_on_one_handle(nat):
    from legal_rag_amd.bm25_model import shard_csr
    rng = np.random.default_rng(3)
    docs = make_docs(rng, 300, only_lead)
    more = make_docs(rng, 30, lambda i: ["new", f"more{i % 4}"])
    whole = fit(docs)
    g = index_of(nat, whole)
    docs, model, _ = remove_from(g, whole, docs, [0, 1, 14, 150, 299])
    lo = len(docs)
    docs = docs + more
    grown = fit(docs)
    term_ptr, post_doc, post_tf, idf, doc_len = grown.to_csr()
    a_ptr, a_doc, a_tf, a_len = shard_csr(term_ptr, post_doc, post_tf, doc_len, lo, len(docs))
    g.add(a_ptr, a_doc, a_tf, idf, a_len, float(grown.avgdl))
    docs, model, _ = remove_from(g, grown, docs, [2, lo - 1, lo, lo + 7, len(docs) - 1])
    f = index_of(nat, model)
    assert_same_state(g, f, 2, adds=1)
    qs = queries_for(rng, g.n_terms)
    assert_same_results(nat, g, f, qs, 2)
    assert_same_serving_step(nat, g, f, qs)
    g.close()
    f.close()


def test_scores_equal_the_oracle(nat):
    from oracle import bm25 as OB
    docs = make_docs(np.random.default_rng(1500), 1500, only_lead)
    ids = spread(1500, 600, 9)
    g, f, model, _ = shrink(nat, docs, ids)
    f.close()
    ob = OB.BM25Okapi(survivors(docs, ids))
    left_only = next(w for w in model.vocab() if w.startswith("only"))
    queries = [["all", "z0", "forty"], ["z3", "z3", "z3", "z1"], ["nowhere", "z2"], [left_only], [f"only{ids[0] - ids[0] % 7}", "z7"],
               ["z0", "all", "z0", "all"], [], ["z399", "z12", "forty", "z5", "z1", "z0"]]
    got = g.get_scores([model.term_ids(q) for q in queries])
    for j, q in enumerate(queries):
        exp = np.asarray(ob.get_scores(q), dtype=np.float64)
        assert got[j].tobytes() == exp.tobytes(), (j, q)
    g.close()


def test_remove_documents_shrinks_the_resident_index(nat):
    """The host model's own route: BM25Okapi.remove_documents on an object with a resident index."""
    docs = make_docs(np.random.default_rng(5), 300, only_lead)
    m = fit(docs)
    g = m.gpu(0)
    assert m.remove_documents([7, 0, 299, 7]) == 3
    assert m.remove_documents([100]) == 1
    assert m.gpu(0) is g
    left = survivors(survivors(docs, [0, 7, 299]), [100])
    whole = fit(left)
    f = index_of(nat, whole)
    assert_same_state(g, f, 2)
    q = ["all", "forty", "z1", "only14", "nowhere"]
    a, b = m.top_k(q, 10), whole.top_k(q, 10)
    assert np.array_equal(a[1], b[1]) and a[0].tobytes() == b[0].tobytes()
    assert_same_serving_step(nat, g, f, queries_for(np.random.default_rng(2), g.n_terms, 4))
    f.close()


def test_bad_arguments_leave_the_handle_unchanged(nat):
    lib = nat.load()
    rng = np.random.default_rng(5)
    pool = np.arange(50)
    old = lists_with(rng, pool[pool % 5 != 0], pool[pool % 5 == 0], [40, 20, 0, 3], [10, 2, 4, 0])
    g = nat.BM25Index(old[0], old[1], old[2], np.asarray([0.3, 1.0, 2.5, 0.7]), np.full(50, 7, np.int32), 7.0)
    before, info = g.read(), g.info()
    ids = pool[pool % 5 == 0].astype(np.int64)  # 10 documents; term 2 loses every posting
    tmap = np.asarray([2, 0, -1, 1], np.int32)
    idf = np.asarray([1.1, 2.0, 0.3])

    def call(h=None, ids=ids, n_remove=None, tmap=tmap, n_terms_new=3, idf=idf, avgdl=6.5):
        p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
        n_remove = (0 if ids is None else len(ids)) if n_remove is None else n_remove
        return lib.amdr_bm25_remove(g._h if h is None else h, p(ids, C.c_int64), C.c_int64(n_remove), p(tmap, C.c_int32),
                                    C.c_int64(n_terms_new), p(idf, C.c_double), C.c_double(avgdl))

    i64 = lambda *v: np.asarray(v, np.int64)  # noqa: E731
    i32 = lambda *v: np.asarray(v, np.int32)  # noqa: E731
    bad = {
        "null handle": dict(h=C.c_void_p()),
        "null remove_ids": dict(ids=None, n_remove=10), "null idf": dict(idf=None),
        "n_remove < 0": dict(n_remove=-1),
        "id n_docs": dict(ids=i64(0, 5, 50)), "id -1": dict(ids=i64(-1, 5, 10)),
        "a repeated id": dict(ids=i64(0, 5, 5)), "descending ids": dict(ids=i64(0, 10, 5)),
        "n_remove == n_docs": dict(ids=np.arange(50, dtype=np.int64)),
        "infinite idf": dict(idf=np.asarray([1.1, np.inf, 0.3])), "NaN idf": dict(idf=np.asarray([np.nan, 2.0, 0.3])),
        "avgdl 0": dict(avgdl=0.0), "avgdl < 0": dict(avgdl=-3.0), "avgdl inf": dict(avgdl=np.inf), "avgdl NaN": dict(avgdl=np.nan),
        "null map, n_terms_new != n_terms": dict(tmap=None),
        "map value n_terms_new": dict(tmap=i32(2, 0, -1, 3)), "map value -2": dict(tmap=i32(2, 0, -2, 1)),
        "two terms on one new id": dict(tmap=i32(2, 0, 0, 1), n_terms_new=3),
        "a new id no term maps to": dict(tmap=i32(2, -1, -1, 1)),
        "n_terms_new above n_terms": dict(n_terms_new=5, idf=np.ones(5)),
        # only the device sees this one: term 1 keeps 20 postings but has no new id
        "a dropped term with a surviving posting": dict(tmap=i32(1, -1, -1, 0), n_terms_new=2, idf=idf[:2].copy()),
    }
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert nat.load().amdr_last_error(), what
        same_arrays(g.read(), before)
        assert g.info() == info and info[5] == 0, what
    # n_remove == 0 reads nothing
    assert call(ids=None, tmap=None, idf=None, n_remove=0) == 0
    same_arrays(g.read(), before)
    assert g.info()[:4] == (50, 4, 79, 0) and g.remove_kernel_ms() == -1.0
    s0 = g.search([[0, 1, 2]], 5)
    # and the good remove goes through afterwards: the handle was left searchable
    assert call() == 0
    assert g.info() == (40, 3, 63, 0, info[4], 1) and g.remove_kernel_ms() > 0
    doc_new = np.where(pool % 5 == 0, -1, np.cumsum(pool % 5 != 0) - 1).astype(np.int32)
    new = filtered_csr(old, doc_new, tmap, 3)
    f = nat.BM25Index(new[0], new[1], new[2], idf, np.full(40, 7, np.int32), 6.5)
    same_arrays(g.read(), f.read())
    same_pair(g.search([[0, 1, 2]], 5), f.search([[0, 1, 2]], 5), "after the good remove")
    assert s0[1].shape == (1, 5)
    g.close()
    f.close()


def test_builder_removes_from_a_live_retriever(nat, tmp_path):
    """IncrementalBM25Builder.remove_ids with a live BM25Retriever: the same host object and native handle afterwards,
    shrunk in place, equal to a retriever that loads the rewritten file — arrays, term ids of a batch, hits."""
    import json
    from conftest import GOLDEN
    from legal_rag_amd.config import AppConfig
    from legal_rag_amd.retrieval.bm25_retriever import BM25Retriever
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    questions = ["what warranty does a merchant give that goods are merchantable", "Short Titles",
                 "statute of frauds signed writing sale of goods price of $500", "risk of loss passes to the buyer"]
    chunks = load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")[:60]
    cfg = AppConfig.for_data_dir(str(tmp_path), "en")
    first = tmp_path / "first.jsonl"
    first.write_text("".join(json.dumps(c.model_dump(), ensure_ascii=False) + "\n" for c in chunks), encoding="utf-8")
    assert IncrementalBM25Builder(cfg).add_jsonl(first) == 60
    r = BM25Retriever(cfg)
    r.load()
    handle, model = r.gpu_index(), r.bm25
    r.term_ids_batch(questions)  # the native tokeniser over the old vocabulary exists
    target = chunks[20]
    assert r.search(target.text[:200], 3)[0][0].id == target.id
    assert IncrementalBM25Builder(cfg).remove_ids([chunks[0].id, target.id, chunks[59].id, "no-such-id"]) == 3
    hits = r.search(target.text[:200], 10)
    assert r.bm25 is model and r.gpu_index() is handle and r.appends == 1 and len(r.chunks) == 57
    assert handle.info()[0] == 57 and handle.info()[3] == 0 and handle.info()[5] == 1
    assert len(hits) == 10 and all(c.id != target.id for c, _ in hits)
    rw = BM25Retriever(cfg)  # loads the rewritten file
    rw.load()
    assert rw.bm25 is not model and rw.gpu_index().info()[:3] == handle.info()[:3]
    same_arrays(handle.read(), rw.gpu_index().read())
    for a, b in zip(r.term_ids_batch(questions), rw.term_ids_batch(questions)):
        assert np.array_equal(a, b)
    for q in questions + [target.text[:200]]:
        got, exp = r.search(q, 10), rw.search(q, 10)
        assert [(c.id, s) for c, s in got] == [(c.id, s) for c, s in exp] and len(exp) == 10

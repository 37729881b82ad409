"""Scoped search on the GPU (csrc/scope.hip): each channel's top-k among a query's OWN rows has the score bits and the
order of the unscoped channel restricted to the scope; the scoped step fuses those lists; validation, reserve, capture
and the public interface."""
import copy
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from helpers import assert_hits_equal_mod_ties

pytestmark = pytest.mark.gpu

TOL = 1e-4
DEV = torch.device("cuda", 0)
FLT_MAX = float(np.finfo(np.float32).max)
DBL_MAX = float(np.finfo(np.float64).max)


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


@pytest.fixture(params=[None, "64"], ids=["default-slabs", "slab-64"])
def slab(request, monkeypatch):
    """AMDR_SCOPE_SLAB unset / 64: with 64 every scope beyond 64 rows spans several slabs and goes through the merge."""
    if request.param is None:
        monkeypatch.delenv("AMDR_SCOPE_SLAB", raising=False)
    else:
        monkeypatch.setenv("AMDR_SCOPE_SLAB", request.param)
    return request.param


def unit_rows(rng, n, d):
    X = rng.standard_normal((n, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X


def make_table(row_lists):
    ptr = np.zeros(len(row_lists) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in row_lists], out=ptr[1:])
    rows = np.concatenate([np.asarray(r, dtype=np.int64) for r in row_lists]) if row_lists else np.zeros(0, np.int64)
    return ptr, rows.astype(np.int64)


def ranked(scores, rows, k, pad):
    """The channel's order of (scores[j], rows[j]): score descending (-0.0 as +0.0, NaN last), ties -> lower id; the
    first k, padded with (pad, -1)."""
    scores = np.asarray(scores)
    key = scores + 0.0
    nan = np.isnan(key)
    order = np.lexsort((rows, np.where(nan, 0.0, -key), nan))  # last key first: not-NaN, then score desc, then id
    order = order[:k]
    s = np.full(k, pad, dtype=scores.dtype)
    i = np.full(k, -1, dtype=np.int64)
    s[:order.size] = key[order]
    i[:order.size] = np.asarray(rows)[order]
    return s, i


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    both_nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all((a.view(u) == b.view(u)) | both_nan))


# ---- dense -------------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 63, 64, 65, 300]


def dense_case(nat, X, Q, row_lists, qscope, ks):
    from oracle import dense as OD
    idx = nat.DenseIndex(X)
    ws = nat.ScopeWorkspace()
    ptr, rows = make_table(row_lists)
    ref = OD.flatip_scores(np.nan_to_num(X), Q)
    for k in ks:
        s, i = ws.dense_search(idx, Q, ptr, rows, qscope, k)
        assert s.shape == (len(qscope), k) and s.dtype == np.float32 and i.dtype == np.int64
        for q, sc in enumerate(qscope):
            if not 0 <= sc < len(row_lists) or len(row_lists[sc]) == 0:
                assert np.all(i[q] == -1) and np.all(s[q] == -FLT_MAX), (k, q)  # all padding
                continue
            r = np.asarray(row_lists[sc], dtype=np.int64)
            bits = idx.score_rows(Q[q], r[None])[0]  # the unscoped channel's score of each row
            es, ei = ranked(bits, r, k, np.float32(-FLT_MAX))
            assert np.array_equal(i[q], ei), (k, q)
            assert same_bits(s[q], es), (k, q)
            m = min(k, r.size)
            fin = ~np.isnan(s[q, :m])
            o = np.sort(ref[q, r[~np.isnan(bits)]])[::-1]  # the oracle's scores of the scope, sorted (ids are NOT compared)
            assert not fin.any() or np.max(np.abs(s[q, :m][fin] - o[:int(fin.sum())])) <= TOL
    ws.close()
    idx.close()


@pytest.mark.parametrize("d", [4, 260, 768, 1024])
def test_dense_scoped_topk_has_the_bits_and_order_of_score_rows(nat, slab, d):
    rng = np.random.default_rng(100 + d)
    n = 300
    X, Q = unit_rows(rng, n, d), unit_rows(rng, 8, d)
    row_lists = [np.sort(rng.choice(n, size=m, replace=False)) for m in SIZES]
    qscope = np.asarray([5, 0, 4, 1, 3, 2, len(SIZES), -1], dtype=np.int32)  # the last two: outside [0, n_scopes)
    dense_case(nat, X, Q, row_lists, qscope, (1, 10, 256))


def test_dense_scoped_ties_take_the_lower_id_and_nan_ranks_last(nat, slab):
    rng = np.random.default_rng(7)
    base = unit_rows(rng, 60, 64)
    X = np.tile(base, (5, 1))  # rows r, r + 60, ...: exactly tied scores
    X[123] = np.nan
    Q = unit_rows(rng, 3, 64)
    some = np.sort(np.concatenate([[123], rng.choice(np.delete(np.arange(300), 123), size=99, replace=False)]))
    dense_case(nat, X, Q, [np.arange(300), some, np.asarray([123])], np.asarray([0, 1, 2], dtype=np.int32), (10, 256))
    idx, ws = nat.DenseIndex(X), nat.ScopeWorkspace()
    s, i = ws.dense_search(idx, Q[:1], [0, 100], some, [0], 256)
    assert i[0, 99] == 123 and math.isnan(s[0, 99]) and i[0, 100] == -1  # NaN: behind every real score, before the padding
    s, i = ws.dense_search(idx, Q[:1], [0, 300], np.arange(300), [0], 10)
    groups = {}
    for sc, r in zip(s[0].tolist(), i[0].tolist()):
        groups.setdefault(sc, []).append(r)
    assert all(g == sorted(g) for g in groups.values()) and any(len(g) > 1 for g in groups.values())


# ---- BM25 --------------------------------------------------------------------------------------------------------------
def bm25_pair(nat, docs):
    from oracle import bm25 as OB
    ob = OB.BM25Okapi(docs)
    csr = OB.to_csr(ob)
    gi = nat.BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"], csr["doc_len"], ob.avgdl, ob.k1, ob.b)
    return ob, csr, gi


def bm25_case(nat, ob, csr, gi, queries, row_lists, qscope, ks):
    """queries: token lists.  Scores and ids bit-equal to the ranking of get_scores restricted to the scope, and to
    the oracle's scores."""
    tids = [[csr["vocab"].get(t, -1) for t in q] for q in queries]
    full = gi.get_scores(tids)
    ws = nat.ScopeWorkspace()
    ptr, rows = make_table(row_lists)
    for k in ks:
        s, i = ws.bm25_search(gi, tids, ptr, rows, qscope, k)
        assert s.dtype == np.float64 and s.shape == (len(queries), k)
        for q, sc in enumerate(qscope):
            r = np.asarray(row_lists[sc], dtype=np.int64)
            es, ei = ranked(full[q, r], r, k, -DBL_MAX)
            assert np.array_equal(i[q], ei), (k, q)
            assert same_bits(s[q], es), (k, q)
            oracle = ob.get_scores(queries[q])[r]
            oes, oei = ranked(oracle, r, k, -DBL_MAX)
            assert np.array_equal(i[q], oei) and same_bits(s[q], oes), (k, q)
    ws.close()


def test_bm25_scoped_on_the_toy_golden(nat, slab):
    from oracle import bm25 as OB
    g = load_golden("bm25_toy.json")
    docs = [OB.tokenize_en(t) for t in g["docs"]]
    ob, csr, gi = bm25_pair(nat, docs)
    words = list(csr["vocab"])
    queries = [c["tokens"] for c in g["queries"]]
    queries.append([words[j % len(words)] for j in range(0, 3 * 37, 3)])  # 37 known tokens: crosses the 32-token group
    queries.append([words[1], words[1], "zzz", words[4], words[1], "qqq", words[4]])  # repeated and unknown tokens
    queries.append(["zzz", "qqq"])  # no known token: the first k scope rows at +0.0
    queries.append([])
    row_lists = [list(range(len(docs))), [1, 3, 6], [len(docs) - 1], []]
    qscope = np.asarray([j % 3 for j in range(len(queries))], dtype=np.int32)
    qscope[-1] = 0
    bm25_case(nat, ob, csr, gi, queries, row_lists, qscope, (1, 3, 10))
    ws = nat.ScopeWorkspace()
    tids = [[-1, -1]]
    s, i = ws.bm25_search(gi, tids, *make_table([[1, 3, 6]]), [0], 5)
    assert i[0].tolist() == [1, 3, 6, -1, -1] and s[0].tolist() == [0.0, 0.0, 0.0, -DBL_MAX, -DBL_MAX]
    assert not np.signbit(s[0, :3]).any()
    s, i = ws.bm25_search(gi, tids, *make_table([[1, 3, 6], []]), [1], 5)  # an empty scope: all padding
    assert np.all(i == -1) and np.all(s == -DBL_MAX)
    s, i = ws.bm25_search(gi, tids, *make_table([[1, 3, 6]]), [7], 5)  # qscope outside [0, n_scopes)
    assert np.all(i == -1) and np.all(s == -DBL_MAX)


@pytest.fixture(scope="module")
def en_chunks():
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    return load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")


def test_bm25_scoped_on_the_en_fixture_with_section_scopes(nat, slab, en_chunks):
    from legal_rag_amd.retrieval.scope import Scope, ScopeResolver
    from oracle import bm25 as OB
    docs = [OB.tokenize_en(c.text) for c in en_chunks]
    ob, csr, gi = bm25_pair(nat, docs)
    res = ScopeResolver(en_chunks)
    secs = sorted({c.section for c in en_chunks if c.section})
    scopes = [Scope(section=secs[3]), Scope(section=secs[20]), Scope(law_name=en_chunks[0].law_name),  # the last: every row
              Scope(section=secs[41])]
    row_lists = [res.rows(s) for s in scopes]
    assert row_lists[2].size == len(en_chunks) > 512
    queries = [OB.tokenize_en("warranty that the goods shall be merchantable is implied in a contract for their sale"),
               max(docs, key=len)[:40],  # >= 33 known tokens
               ["seller", "seller", "zzzunknown", "buyer", "seller"],
               OB.tokenize_en("risk of loss passes to the buyer on tender of delivery"),
               ["zzzunknown"]]
    assert len(queries[1]) >= 33
    qscope = np.asarray([0, 0, 1, 2, 3], dtype=np.int32)
    bm25_case(nat, ob, csr, gi, queries, row_lists, qscope, (1, 10, 256))


# ---- MaxSim ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maxsim_golden():
    g = np.load(GOLDEN / "maxsim_golden.npz")
    rng = np.random.default_rng(42)
    lens = rng.integers(1, 221, size=64)
    lens[0], lens[-1] = 1, 220
    assert np.array_equal(lens, g["lens"])
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    D = unit_rows(rng, int(ptr[-1]), 128)
    Q2 = unit_rows(rng, 64, 128).reshape(2, 32, 128)
    Q = np.concatenate([Q2, unit_rows(rng, 5 * 32, 128).reshape(5, 32, 128)])
    return lens, ptr, D, Q, g["scores"]


def doc_scopes(lens):
    short = np.flatnonzero(lens <= 16)
    mid = np.flatnonzero((lens > 16) & (lens <= 32))
    long_ = np.flatnonzero(lens > 32)
    assert short.size and mid.size and long_.size
    last = len(lens) - 1
    return [np.arange(len(lens)), np.sort(np.unique(np.concatenate([short[:2], mid[:2], long_[:3], [last]]))),
            np.asarray([last]), np.asarray([int(short[0])]), np.zeros(0, np.int64), np.sort(np.unique(np.concatenate([mid, [0]])))]


@pytest.mark.parametrize("nq", [1, 2, 7])
def test_maxsim_scoped_has_the_bits_of_the_pair_form(nat, slab, maxsim_golden, nq):
    from oracle import maxsim as OM
    lens, ptr, D, Q, gold = maxsim_golden
    idx = nat.MaxSimIndex(D, ptr)
    assert "maxsim_scores_h_kernel" in idx.plan_info(nq)  # the scores compared against ran the pair form
    full = idx.scores(Q[:nq])
    ref = OM.maxsim_scores(Q[:nq], D, ptr)
    if nq >= 2:
        assert np.allclose(ref[:2], gold, atol=1e-12)
    row_lists = doc_scopes(lens)
    qscope = np.asarray([(3 * q + 1) % len(row_lists) for q in range(nq)], dtype=np.int32)
    tp, tr = make_table(row_lists)
    ws = nat.ScopeWorkspace()
    for k in (1, 10, 256):
        for qs in (qscope, np.zeros(nq, np.int32)):
            s, i = ws.maxsim_search(idx, Q[:nq], tp, tr, qs, k)
            for q, sc in enumerate(qs):
                r = row_lists[sc]
                es, ei = ranked(full[q, r], r, k, np.float32(-FLT_MAX))
                assert np.array_equal(i[q], ei) and same_bits(s[q], es), (k, q)
                m = min(k, r.size)
                assert m == 0 or np.max(np.abs(s[q, :m] - ref[q, i[q, :m]])) <= TOL
    ws.close()
    idx.close()


def test_maxsim_scoped_refuses_the_fp32_input_pin_and_writes_nothing(nat, monkeypatch, maxsim_golden):
    lens, ptr, D, Q, _ = maxsim_golden
    idx, ws = nat.MaxSimIndex(D, ptr), nat.ScopeWorkspace()
    tp, tr = make_table([np.arange(10)])
    ws.reserve(2, 10, 64)
    sp, rw, qs = (torch.from_numpy(a).to(DEV) for a in (tp, tr, np.zeros(2, np.int32)))
    q = torch.from_numpy(Q[:2]).to(DEV)
    s = torch.full((2, 10), 123.0, dtype=torch.float32, device=DEV)
    i = torch.full((2, 10), 77, dtype=torch.int64, device=DEV)
    table = (sp.data_ptr(), rw.data_ptr(), qs.data_ptr(), 1, 10)
    monkeypatch.setenv("AMDR_MAXSIM_F16X3", "0")
    with pytest.raises(nat.NativeError, match="F16X3"):
        ws.maxsim_search_device(idx, q.data_ptr(), 32, table, 2, 10, s.data_ptr(), i.data_ptr(), 0)
    with pytest.raises(nat.NativeError, match="F16X3"):
        ws.maxsim_search(idx, Q[:2], tp, tr, [0, 0], 10)
    torch.cuda.synchronize()
    assert bool((s == 123.0).all()) and bool((i == 77).all())
    monkeypatch.setenv("AMDR_MAXSIM_F16X3", "1")
    ws.maxsim_search_device(idx, q.data_ptr(), 32, table, 2, 10, s.data_ptr(), i.data_ptr(), 0)
    torch.cuda.synchronize()
    es, ei = ws.maxsim_search(idx, Q[:2], tp, tr, [0, 0], 10)
    assert np.array_equal(i.cpu().numpy(), ei) and same_bits(s.cpu().numpy(), es)
    # a store holding an infinity has no split image
    Dn = D.copy()
    Dn[5, 3] = np.inf
    bad = nat.MaxSimIndex(Dn, ptr)
    with pytest.raises(nat.NativeError, match="split-fp16"):
        ws.maxsim_search(bad, Q[:1], tp, tr, [0], 10)


# ---- host-twin validation, the reserve ------------------------------------------------------------------------------------
def test_host_twins_validate_the_table(nat):
    rng = np.random.default_rng(3)
    idx, ws = nat.DenseIndex(unit_rows(rng, 50, 8)), nat.ScopeWorkspace()
    Q = unit_rows(rng, 1, 8)
    ok = ws.dense_search(idx, Q, [0, 3], [1, 5, 9], [0], 4)
    assert ok[1][0, 3] == -1 and sorted(ok[1][0, :3].tolist()) == [1, 5, 9]
    for ptr, rows, what in (([0, 3], [5, 1, 9], "ascending"),      # not ascending
                            ([0, 3], [1, 5, 5], "ascending"),      # duplicate
                            ([0, 3], [1, 5, 50], "outside"),       # row >= n
                            ([0, 3], [-1, 5, 9], "outside"),
                            ([0, 2, 1], [1, 5, 9], "monotone")):
        with pytest.raises(nat.NativeError, match=what):
            ws.dense_search(idx, Q, ptr, rows, [0], 4)
    with pytest.raises(nat.NativeError):
        ws.dense_search(idx, Q, [0, 3], [1, 5, 9], [0], nat.MAX_K + 1)
    # two scopes may hold the same row, and a later scope may start below the one before
    s, i = ws.dense_search(idx, np.repeat(Q, 2, 0), [0, 2, 4], [5, 9, 1, 5], [0, 1], 2)
    assert sorted(i[0].tolist()) == [5, 9] and sorted(i[1].tolist()) == [1, 5]


def test_device_call_beyond_the_reserve_is_refused_and_writes_nothing(nat, monkeypatch):
    monkeypatch.setenv("AMDR_SCOPE_SLAB", "64")
    rng = np.random.default_rng(4)
    n, d = 300, 32
    X, Q = unit_rows(rng, n, d), unit_rows(rng, 4, d)
    idx, ws = nat.DenseIndex(X), nat.ScopeWorkspace()
    ptr, rows = make_table([np.arange(200)])
    sp, rw, qs, q = (torch.from_numpy(a).to(DEV) for a in (ptr, rows, np.zeros(4, np.int32), Q))
    s = torch.full((4, 10), 123.0, dtype=torch.float32, device=DEV)
    i = torch.full((4, 10), 77, dtype=torch.int64, device=DEV)

    def call(nq, k, rows_max):
        ws.dense_search_device(idx, q.data_ptr(), (sp.data_ptr(), rw.data_ptr(), qs.data_ptr(), 1, rows_max), nq, k,
                               s.data_ptr(), i.data_ptr(), 0)
    with pytest.raises(nat.NativeError, match="reserve"):
        call(4, 10, 200)  # never reserved
    ws.reserve(2, 10, 200)
    for nq, k, rows_max in ((4, 10, 200), (2, 11, 200), (2, 10, 201)):
        with pytest.raises(nat.NativeError, match="reserve"):
            call(nq, k, rows_max)
    torch.cuda.synchronize()
    assert bool((s == 123.0).all()) and bool((i == 77).all())
    g0 = nat.workspace_growths()
    call(2, 10, 200)
    torch.cuda.synchronize()
    assert nat.workspace_growths() == g0
    es, ei = ws.dense_search(idx, Q[:2], ptr, rows, [0, 0], 10)
    assert np.array_equal(i[:2].cpu().numpy(), ei) and same_bits(s[:2].cpu().numpy(), es)
    assert bool((s[2:] == 123.0).all())
    assert "merge_parts_kernel" in ws.plan_info(2, 10, 200) and "(direct)" in ws.plan_info(2, 10, 64)


# ---- the scoped step -----------------------------------------------------------------------------------------------------
def exact_corpus(rng, n):
    """Three channels over n rows whose scores are exact in every arithmetic: dense / token components are multiples of
    1/8 in [-1, 1] (products multiples of 1/64, sums far inside 24 bits), so the fp64 oracle, the fp32 GEMV and the
    split-fp16 pair form give the same numbers and the oracle's lists can be compared exactly."""
    X = (rng.integers(-8, 9, size=(n, 64)) / 8.0).astype(np.float32)
    words = [f"w{j}" for j in range(120)]
    docs = [[words[j] for j in rng.integers(0, len(words), size=int(rng.integers(3, 30)))] for _ in range(n)]
    lens = rng.integers(1, 70, size=n)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    D = (rng.integers(-8, 9, size=(int(ptr[-1]), 128)) / 8.0).astype(np.float32)
    return X, words, docs, ptr, D


def fused_hits(ids, vals, mask, count, kn):
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    chunks = [SimpleNamespace(id=j) for j in range(int(ids.max()) + 2)]
    hits = HybridRetriever._hits_from_native(ids, vals, mask, int(count), kn, chunks)
    return [{"id": h.chunk.id, "score": float(h.score), "rank": h.rank, "source": h.source, "breakdown": h.score_breakdown}
            for h in hits]


@pytest.mark.parametrize("with_colbert", [False, True], ids=["dense+bm25", "dense+bm25+colbert"])
def test_scoped_step_fuses_the_scoped_lists(nat, slab, with_colbert):
    from legal_rag_amd.retrieval.engine import HybridEngine
    from oracle import bm25 as OB
    from oracle import dense as OD
    from oracle import fusion as OF
    from oracle import maxsim as OM
    rng = np.random.default_rng(11)
    n, nq, k = 300, 6, 10
    X, words, docs, ptr, D = exact_corpus(rng, n)
    ob, csr, gi = bm25_pair(nat, docs)
    di = nat.DenseIndex(X)
    mi = nat.MaxSimIndex(D, ptr) if with_colbert else None
    eng = HybridEngine(di, gi, mi)
    Q = (rng.integers(-8, 9, size=(nq, 64)) / 8.0).astype(np.float32)
    Qt = (rng.integers(-8, 9, size=(nq, 32, 128)) / 8.0).astype(np.float32)
    queries = [[words[j] for j in rng.integers(0, len(words), size=6)] for _ in range(nq)]
    # one table per channel's row space: they differ; scope 1 is shorter than k, scope 3 is empty
    tabs = []
    for c in range(3):
        lists = [np.sort(rng.choice(n, size=m, replace=False)) for m in (40 + c, 4, 130 + c, 0)]
        tabs.append((lists, np.asarray([0, 1, 2, 3, 1, 2], dtype=np.int32)))
    q_terms, q_ptr = nat.BM25Index.pack_queries([[csr["vocab"][t] for t in q] for q in queries])
    q_ptr_d, q_terms_d = eng.upload_csr(q_ptr, q_terms)
    dev_tabs = [eng.upload_scopes(*make_table(lists), qs, channel=c) for c, (lists, qs) in enumerate(tabs)]
    assert dev_tabs[0][3] == 4 and dev_tabs[0][4] == 130
    params = nat.make_fuse_params(method="rrf_norm_blend", rrf_k=60, alpha=0.5, w_dense=0.6, w_bm25=0.4, w_colbert=0.35,
                                  min_final_score=-math.inf)
    res = eng.search_batch(params, k, q_emb=torch.from_numpy(Q).to(DEV), q_terms=q_terms_d, q_ptr=q_ptr_d,
                           q_tok=torch.from_numpy(Qt).to(DEV) if with_colbert else None,
                           scopes=(dev_tabs[0], dev_tabs[1], dev_tabs[2] if with_colbert else None))
    ids, vals, mask, count = (a.copy() for a in res.to_host())
    chans = [(res.dense_ids.cpu().numpy(), res.dense_scores.cpu().numpy()),
             (res.bm25_ids.cpu().numpy(), res.bm25_scores.cpu().numpy())]
    if with_colbert:
        chans.append((res.colbert_ids.cpu().numpy(), res.colbert_scores.cpu().numpy()))
    # the channel lists are the host twins' (bits), the fused record is _native.fuse on the same lists (bits)
    ws = nat.ScopeWorkspace()
    twin = [ws.dense_search(di, Q, *make_table(tabs[0][0]), tabs[0][1], k),
            ws.bm25_search(gi, [[csr["vocab"][t] for t in q] for q in queries], *make_table(tabs[1][0]), tabs[1][1], k)]
    if with_colbert:
        twin.append(ws.maxsim_search(mi, Qt, *make_table(tabs[2][0]), tabs[2][1], k))
    for (ci, cs), (ts, ti) in zip(chans, twin):
        assert np.array_equal(ci, ti) and same_bits(cs, ts)
    fi, fv, fm, fc = nat.fuse(params, nq, *[(ci, cs.astype(np.float64)) for ci, cs in chans])
    assert np.array_equal(ids, fi) and np.array_equal(mask, fm) and np.array_equal(count, fc)
    assert np.array_equal(vals.view(np.uint64), fv.view(np.uint64))
    # ... and the oracle's fusion of the oracle's scoped lists
    refs = [OD.flatip_scores(X, Q).astype(np.float64), np.stack([ob.get_scores(q) for q in queries])]
    if with_colbert:
        refs.append(OM.maxsim_scores(Qt, D, ptr))
    kn = {"method": "rrf_norm_blend", "rrf_k": 60, "alpha": 0.5, "weights": {"dense": 0.6, "bm25": 0.4, "colbert": 0.35}}
    for q in range(nq):
        lists = []
        for c, ref in enumerate(refs):
            r = tabs[c][0][tabs[c][1][q]]
            es, ei = ranked(ref[q, r], r, k, -DBL_MAX)
            lists.append([(int(i), float(s)) for s, i in zip(es, ei) if i >= 0])
        while len(lists) < 3:
            lists.append([])
        exp = OF.fuse(*lists, {"dense_weight": 0.6, "bm25_weight": 0.4, "colbert_weight": 0.35, "rrf_alpha": 0.5, "rrf_k": 60,
                               "fusion_method": "rrf_norm_blend"})
        assert count[q] == len(exp)
        if tabs[0][1][q] == 3:
            assert len(exp) == 0 and np.all(ids[q] == -1)  # the empty scope
            continue
        if tabs[0][1][q] == 1:
            assert len(lists[0]) == 4 < k  # a scope shorter than k: padded lists
        assert_hits_equal_mod_ties(fused_hits(ids[q], vals[q], mask[q], count[q], kn), exp)


def test_scoped_step_on_a_sharded_engine_raises(nat):
    from legal_rag_amd.retrieval.engine import HybridEngine
    rng = np.random.default_rng(5)
    eng = HybridEngine(nat.DenseIndex(unit_rows(rng, 20, 8)), None, shard_offset=0)
    with pytest.raises(ValueError, match="shard"):
        eng.reserve(1, 5, rows_max=10)
    tb = (torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
          torch.zeros(1, dtype=torch.int32, device=DEV), 1, 1)
    with pytest.raises(ValueError, match="shard"):
        eng.search_batch(nat.make_fuse_params(), 5, q_emb=torch.zeros((1, 8), device=DEV), scopes=(tb, None, None))


def test_captured_scoped_step_replays_with_the_table_rewritten_in_place(nat, monkeypatch):
    from legal_rag_amd.retrieval.engine import HybridEngine
    monkeypatch.setenv("AMDR_SCOPE_SLAB", "64")  # several slabs: the captured step holds the merges too
    rng = np.random.default_rng(21)
    n, nq, k = 300, 5, 10
    X, words, docs, ptr, D = exact_corpus(rng, n)
    ob, csr, gi = bm25_pair(nat, docs)
    eng = HybridEngine(nat.DenseIndex(X), gi, nat.MaxSimIndex(D, ptr))
    params = nat.make_fuse_params(min_final_score=0.0)
    Q = torch.from_numpy(unit_rows(rng, nq, 64)).to(DEV)
    Qt = torch.from_numpy(unit_rows(rng, nq * 32, 128).reshape(nq, 32, 128)).to(DEV)
    q_terms, q_ptr = nat.BM25Index.pack_queries([[int(t) for t in rng.integers(0, len(words), size=5)] for _ in range(nq)])
    q_terms_d, q_ptr_d = torch.from_numpy(q_terms).to(DEV), torch.from_numpy(q_ptr).to(DEV)

    def host_table(seed):
        r = np.random.default_rng(seed)
        lists = [np.sort(r.choice(n, size=int(m), replace=False)) for m in r.integers(1, 150, size=3)]
        return make_table(lists) + (r.integers(0, 4, size=nq).astype(np.int32),)  # (qscope 3: outside -> padding)
    cap_rows, rows_max = 3 * 150, 150
    sp = torch.zeros(4, dtype=torch.int64, device=DEV)
    rw = torch.zeros(cap_rows, dtype=torch.int64, device=DEV)
    qs = torch.zeros(nq, dtype=torch.int32, device=DEV)
    table = (sp, rw, qs, 3, rows_max)

    def write(seed):
        p, r, s = host_table(seed)
        sp.copy_(torch.from_numpy(p))
        rw[:r.size].copy_(torch.from_numpy(r))
        qs.copy_(torch.from_numpy(s))

    def snapshot(res):
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (res.ids, res.vals, res.mask, res.count, res.dense_ids, res.dense_scores,
                                                 res.bm25_ids, res.bm25_scores, res.colbert_ids, res.colbert_scores)]
    kw = dict(q_emb=Q, q_terms=q_terms_d, q_ptr=q_ptr_d, q_tok=Qt, scopes=(table, table, table))
    write(1)
    graph, gres = eng.capture(params, k, **kw)
    g0 = nat.workspace_growths()
    for seed in (2, 3):
        write(seed)
        graph.replay()
        got = snapshot(gres)
        assert nat.workspace_growths() == g0
        exp = snapshot(eng.search_batch(params, k, **kw))  # the eager call on the same table
        assert nat.workspace_growths() == g0
        for a, b in zip(got, exp):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert (got[0] >= 0).any()


# ---- the public interface ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ucc_index(tmp_path_factory):
    """The UCC-en indexes built with the product builders (stand-in encoders), ColBERT included."""
    from legal_rag_amd.config import AppConfig
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.colbert_builder import build_colbert_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    data = tmp_path_factory.mktemp("scope_data")
    cfg = AppConfig.for_data_dir(str(data), "en")
    cfg.retrieval.encoder_backend = "hashing"
    cfg.retrieval.enable_rerank = False
    chunks = load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")[:200]
    build_faiss_index(cfg, chunks)
    build_bm25_index(cfg, chunks)
    build_colbert_index(cfg, chunks)
    return cfg, chunks


def dump(h):
    return {"id": h.chunk.id, "score": float(h.score), "rank": h.rank, "source": h.source, "breakdown": h.score_breakdown}


QUESTIONS = ["what warranty does a merchant give that goods are merchantable", "Short Titles",
             "statute of frauds signed writing sale of goods price of $500", "risk of loss passes to the buyer"]


def test_search_with_a_scope_returns_only_the_scope(ucc_index):
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from legal_rag_amd.retrieval.scope import Scope
    cfg, chunks = ucc_index
    r = HybridRetriever(cfg)
    assert r.colbert is not None and r.colbert.enabled
    sizes = {}
    for c in chunks:
        sizes[c.section] = sizes.get(c.section, 0) + 1
    big = max(sizes, key=sizes.get)
    small = min((s for s in sizes if s), key=sizes.get)
    for q in QUESTIONS[:2]:
        plain = [dump(h) for h in r.search(q, top_k=10)]
        assert [dump(h) for h in r.search(q, top_k=10, scope=None)] == plain  # None: today's path
        for sec in (big, small):
            hits = r.search(q, top_k=10, scope=Scope(section=sec))
            assert hits and all(h.chunk.section == sec for h in hits) and len(hits) <= min(10, sizes[sec])
            assert [h.rank for h in hits] == list(range(1, len(hits) + 1))
            again = r.search_batch([q], top_k=10, scopes=[Scope(section=sec)])[0]
            assert [dump(h) for h in again] == [dump(h) for h in hits]
    # a narrow scope still fills the list: every one of its chunks is a candidate in every channel
    cfg2 = copy.deepcopy(cfg)
    cfg2.retrieval.min_final_score = -1.0
    r2 = HybridRetriever(cfg2)
    hits = r2.search(QUESTIONS[0], top_k=10, scope=Scope(section=small))
    assert len(hits) == min(10, sizes[small]) and all(h.chunk.section == small for h in hits)
    assert r.search(QUESTIONS[0], top_k=10, scope=Scope(section="no such section")) == []
    with pytest.raises(ValueError, match="graph"):
        r.search(QUESTIONS[0], top_k=10, decision=SimpleNamespace(mode="GRAPH_AUGMENTED"), scope=Scope(section=big))


def test_per_channel_searches_take_a_scope(ucc_index):
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from legal_rag_amd.retrieval.scope import Scope
    cfg, chunks = ucc_index
    r = HybridRetriever(cfg)
    sec = chunks[60].section
    inside = {c.id for c in chunks if c.section == sec}
    q = QUESTIONS[0]
    for fn, tol in ((r.search_dense, 2e-5), (r.search_bm25, 0.0), (r.search_colbert, 2e-5)):
        whole = {h.chunk.id: h.score for h in fn(q, 200)}
        got = fn(q, 10, scope=Scope(section=sec))
        assert len(got) == min(10, len(inside)) and all(h.chunk.id in inside for h in got)
        assert [h.rank for h in got] == list(range(1, len(got) + 1))
        # the scores are the unscoped channel's (dense / ColBERT: a deep unscoped search takes another kernel form)
        assert all(abs(h.score - whole[h.chunk.id]) <= tol for h in got)
        best = sorted((s for i, s in whole.items() if i in inside), reverse=True)[:len(got)]
        assert np.allclose([h.score for h in got], best, rtol=0, atol=tol)
        assert fn(q, 10, scope=Scope(section="no such section")) == []


def test_mixed_batch_is_re_interleaved(ucc_index):
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from legal_rag_amd.retrieval.scope import Scope
    cfg, chunks = ucc_index
    r = HybridRetriever(cfg)
    s1, s2 = Scope(section=chunks[10].section), Scope(section=chunks[150].section)
    assert s1 != s2
    scopes = [None, s1, None, Scope(section="no such section"), s2, s1]
    qs = [QUESTIONS[j % len(QUESTIONS)] for j in range(len(scopes))]
    out = r.search_batch(qs, top_k=10, scopes=scopes)
    plain = r.search_batch([qs[0], qs[2]], top_k=10)
    assert [dump(h) for h in out[0]] == [dump(h) for h in plain[0]]
    assert [dump(h) for h in out[2]] == [dump(h) for h in plain[1]]
    assert out[3] == []
    for j in (1, 4, 5):
        exp = r.search(qs[j], top_k=10, scope=scopes[j])
        assert [dump(h) for h in out[j]] == [dump(h) for h in exp] and exp
        assert all(h.chunk.section == scopes[j].section for h in out[j])
    assert [dump(h) for h in r.search_batch(qs, top_k=10, scopes=[None] * len(qs))[1]] == \
        [dump(h) for h in r.search_batch(qs, top_k=10)[1]]
    with pytest.raises(ValueError, match="graph"):
        r.search_batch(qs[:2], top_k=10, scopes=[None, s1], decisions=[None, SimpleNamespace(mode="GRAPH_AUGMENTED")])
    # the columnar form: the same rows and scores
    arr = r.search_batch_arrays(qs, top_k=10, scopes=scopes)
    for j, hits in enumerate(out):
        assert arr["count"][j] == len(hits)
        assert [arr["chunks"][int(x)].id for x in arr["rows"][j, :len(hits)]] == [h.chunk.id for h in hits]
        assert arr["scores"][j, :len(hits)].tolist() == [h.score for h in hits]
        assert np.all(arr["rows"][j, len(hits):] == -1)
    lean = r.search_batch_arrays(qs, top_k=10, scopes=scopes, values=False)
    assert np.array_equal(lean["rows"], arr["rows"]) and np.array_equal(lean["count"], arr["count"])


def test_mixed_batch_reranks_once_and_equals_each_question_alone(ucc_index, monkeypatch):
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from legal_rag_amd.retrieval.scope import Scope
    cfg, chunks = ucc_index
    cfg2 = copy.deepcopy(cfg)
    cfg2.retrieval.enable_rerank = True
    cfg2.retrieval.rerank_ce_model = "hashing"  # the stand-in cross-encoder
    r = HybridRetriever(cfg2)
    s1, s2 = Scope(section=chunks[10].section), Scope(section=chunks[150].section)
    scopes = [None, s1, None, Scope(section="no such section"), s2, s1]
    qs = [QUESTIONS[j % len(QUESTIONS)] for j in range(len(scopes))]
    calls, stage = [], HybridRetriever._rerank_stage

    def counted(self, questions, *args, **kw):
        calls.append(len(questions))
        return stage(self, questions, *args, **kw)
    monkeypatch.setattr(HybridRetriever, "_rerank_stage", counted)
    out = r.search_batch(qs, top_k=10, scopes=scopes)
    assert calls == [len(qs)]  # ONE stage over the whole batch: one pass through the cross-encoder, one blend launch
    assert out[3] == []
    for j, hits in enumerate(out):
        exp = r.search(qs[j], top_k=10, scope=scopes[j])
        assert [dump(h) for h in hits] == [dump(h) for h in exp], j
        assert j == 3 or any(h.source == "rerank" for h in hits)


def test_blank_questions_run_apart_with_and_without_a_scope(ucc_index):
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from legal_rag_amd.retrieval.scope import Scope
    cfg, chunks = ucc_index
    r = HybridRetriever(cfg)
    assert r.colbert is not None and r.colbert.enabled
    s1 = Scope(section=chunks[10].section)
    qs, scopes = ["", "  ", QUESTIONS[0], QUESTIONS[3]], [None, s1, None, s1]
    out = r.search_batch(qs, top_k=10, scopes=scopes)
    for j, hits in enumerate(out):
        exp = r.search(qs[j], top_k=10, scope=scopes[j])
        assert [dump(h) for h in hits] == [dump(h) for h in exp], j
    assert all("colbert" in h.score_breakdown["channel"] for h in out[3][:1]) and out[2] and out[3]
    assert not any("colbert" in h.score_breakdown["channel"] for j in (0, 1) for h in out[j])
    for values in (True, False):
        with pytest.raises(ValueError, match="empty questions are not supported in the columnar form"):
            r.search_batch_arrays(qs, top_k=10, scopes=scopes, values=values)


def test_graph_and_scopes_in_one_columnar_call(tmp_path):
    from legal_rag_amd.retrieval.hybrid_retriever import COLUMNS
    from legal_rag_amd.retrieval.scope import Scope
    from test_graph_device_gpu import ucc_retriever
    hr, chunks = ucc_retriever(tmp_path, "device")
    s1, s2 = Scope(section=chunks[10].section), Scope(section=chunks[150].section)
    graph, other = SimpleNamespace(mode="GRAPH_AUGMENTED"), SimpleNamespace(mode="HYBRID")
    qs = QUESTIONS + QUESTIONS[:2]
    scopes = [None, s1, None, s2, None, None]
    decisions = [graph, None, other, None, graph, None]
    for values in (True, False):
        arr = hr.search_batch_arrays(qs, top_k=10, values=values, decisions=decisions, scopes=scopes)
        alone = hr.search_batch_arrays([qs[0], qs[4]], top_k=10, values=values, decisions=[graph, graph])
        assert int(alone["graph_count"].min()) > 0 and arr["count"][1] > 0 and arr["count"][3] > 0
        assert arr["graph_relation_names"] == alone["graph_relation_names"]
        for name, dt, fill, hit in COLUMNS:
            if name.startswith("graph_"):
                assert arr[name].dtype == alone[name].dtype == dt
                assert arr[name].shape == ((6,) if hit is None else (6, 10))
                assert np.array_equal(arr[name][[0, 4]], alone[name]), name
                assert (arr[name][[1, 2, 3, 5]] == fill).all(), name
        assert arr["graph_count"][[1, 2, 3, 5]].tolist() == [0, 0, 0, 0]

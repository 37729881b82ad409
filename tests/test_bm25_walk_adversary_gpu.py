"""The BM25 scoring walk (bm25_block_query, csrc/bm25_core.hpp) and its scoped twin (scope_bm25_piece, csrc/scope.hip) on
the indexes of tests/bm25_walk_adversary.py: posting lists around one chunk, one prefetch window and nine chunks, token
boundaries at every window position, token groups with and without kept tokens, postings on both sides of every slab
border, slabs no token touches, sums that cancel.  tests/test_bm25_walk_adversary.py proves that the data reaches those
edges and that wrong walks would fail; here every result is compared with the numpy fp64 reference of
bm25_image_adversary (ref_scores, ref_topk) and with nothing else: ids exactly, scores bit for bit as uint64, the sign of
zero included, through get_scores, search (AMDR_BM25_SELECT=1 and =0), search_device (eager and replayed from a graph),
the scoped search, the scoped step in both phase orders, the one-launch serving step and the long-batch step."""
from types import SimpleNamespace

import numpy as np
import pytest

import bm25_image_adversary as IA
import bm25_walk_adversary as WA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    return _native


@pytest.fixture(scope="module")
def cases():
    return WA.all_cases()


@pytest.fixture(scope="module")
def indexes(nat):
    """One BM25Index per corpus for the whole module: index(csr)."""
    held = {}

    def index(csr):
        if id(csr) not in held:
            held[id(csr)] = (csr, nat.BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"], csr["doc_len"],
                                                csr["avgdl"], csr["k1"], csr["b"]))
        return held[id(csr)][1]
    yield index
    for _, gi in held.values():
        gi.close()


_REF = {}


def _rows(case):
    """ref_scores of the case's queries, computed once per (index, query list) and left unchanged."""
    key = (id(case.csr), id(case.queries))
    if key not in _REF:
        rows = IA.ref_scores(case.csr, case.queries)
        rows.setflags(write=False)
        _REF[key] = (case.csr, case.queries, rows)
    return _REF[key][2]


def _expected(case, k=None):
    top = [IA.ref_topk(r, case.k if k is None else k) for r in _rows(case)]
    return np.stack([t[0] for t in top]), np.stack([t[1] for t in top])


def _diff(name, q, ids, scores, ei, es):
    if np.array_equal(ids, ei) and np.array_equal(np.ascontiguousarray(scores).view(np.uint64), es.view(np.uint64)):
        return []
    at = int(np.nonzero((ids != ei) | (np.ascontiguousarray(scores).view(np.uint64) != es.view(np.uint64)))[0][0])
    return [f"{name} query {q}: rank {at}: returned ({int(ids[at])}, {float(scores[at])!r}), expected ({int(ei[at])}, {float(es[at])!r})"]


def _report(bad, total, what):
    print(f"{what}: {total - len(bad)} of {total} equal the fp64 reference")
    assert not bad, f"{what}: {len(bad)} of {total} differ from the fp64 reference; the first: {bad[0]}"


def _groups(cases, family):
    seen, out = set(), []
    for c in cases:
        if c.family == family and (id(c.csr), id(c.queries)) not in seen:
            seen.add((id(c.csr), id(c.queries)))
            out.append(c)
    return out


# ---- get_scores and search ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", WA.FAMILIES)
def test_get_scores_has_every_bit_of_the_reference(nat, cases, indexes, family):
    bad, total = [], 0
    for c in _groups(cases, family):
        rows = _rows(c)
        full = indexes(c.csr).get_scores(c.queries)
        assert full.shape == rows.shape
        for q in range(len(c.queries)):
            total += 1
            if not np.array_equal(full[q].view(np.uint64), rows[q].view(np.uint64)):
                d = int(np.nonzero(full[q].view(np.uint64) != rows[q].view(np.uint64))[0][0])
                bad.append(f"{c.family} {c.group} n={c.n} query {q}: document {d}: returned {float(full[q, d])!r}, expected {float(rows[q, d])!r}")
    _report(bad, total, f"{family} get_scores")


@pytest.mark.parametrize("family", WA.FAMILIES)
@pytest.mark.parametrize("select", ["1", "0"])
def test_search_at_every_depth(nat, cases, indexes, monkeypatch, select, family):
    monkeypatch.setenv("AMDR_BM25_SELECT", select)
    mine = [c for c in cases if c.family == family]
    assert {c.k for c in mine} == set(WA.DEPTHS)
    bad = []
    for c in mine:
        gi = indexes(c.csr)
        slabs, path = IA.plan_text(c.n, c.k)
        plan = gi.plan_info(len(c.queries), c.k)
        assert slabs in plan and path in plan, (c.name, plan)  # the slabs and the ranking the case was built for
        ei, es = _expected(c)
        s, i = gi.search(c.queries, c.k)
        mism = []
        for q in range(len(c.queries)):
            mism += _diff(c.name, q, i[q], s[q], ei[q], es[q])
        bad += mism[:1]
    _report(bad, len(mine), f"{family} AMDR_BM25_SELECT={select}")


@pytest.mark.parametrize("select", ["1", "0"])
def test_search_device_eager_and_replayed(nat, cases, indexes, monkeypatch, select):
    import torch
    monkeypatch.setenv("AMDR_BM25_SELECT", select)
    dev = torch.device("cuda", 0)
    a = next(c for c in cases if c.family == "W2" and c.group == "boundary" and c.k == 10)
    b = next(c for c in cases if c.family == "W4" and c.group == "borders" and c.n == 4097 and c.k == 16)  # three slabs + merge
    for c in (a, b):
        ei, es = _expected(c)
        gi = indexes(c.csr)
        nq, k = len(c.queries), c.k
        qt_h, qp_h = nat.BM25Index.pack_queries(c.queries)
        gi.reserve(nq, k, int(qp_h[-1]))
        qt, qp = torch.from_numpy(qt_h).to(dev), torch.from_numpy(qp_h).to(dev)
        s = torch.zeros((nq, k), dtype=torch.float64, device=dev)
        i = torch.zeros((nq, k), dtype=torch.int64, device=dev)

        def same(what):
            torch.cuda.synchronize()
            assert np.array_equal(i.cpu().numpy(), ei), (c.name, what)
            assert np.array_equal(s.cpu().numpy().view(np.uint64), es.view(np.uint64)), (c.name, what)

        gi.search_device(qt.data_ptr(), qp.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(),
                         int(torch.cuda.current_stream().cuda_stream))
        same("eager")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            gi.search_device(qt.data_ptr(), qp.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(),
                             int(torch.cuda.current_stream().cuda_stream))
        for _ in range(2):
            s.zero_()
            i.zero_()
            g.replay()
            same("replay")
        del g


# ---- the scoped twin ---------------------------------------------------------------------------------------------------
def _table(row_lists):
    ptr = np.zeros(len(row_lists) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in row_lists], out=ptr[1:])
    rows = np.concatenate([np.asarray(r, dtype=np.int64) for r in row_lists]) if row_lists else np.zeros(0, np.int64)
    return ptr, rows.astype(np.int64)


def _pick(case, count):
    """`count` queries of the case, evenly spread, the longest among them."""
    qs = case.queries
    idx = sorted(set(np.linspace(0, len(qs) - 1, min(count, len(qs))).astype(int).tolist()) | {max(range(len(qs)), key=lambda j: len(qs[j]))})
    return idx


@pytest.fixture(params=[None, "64"], ids=["default-slabs", "slab-64"])
def scope_slab(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("AMDR_SCOPE_SLAB", raising=False)
    else:
        monkeypatch.setenv("AMDR_SCOPE_SLAB", request.param)
    return request.param


@pytest.mark.parametrize("which", ["W4 borders 4097", "W4 zero-slabs 4100", "W3 empty-groups 2100", "W2 boundary 1024", "W1 L=1025 1100"])
def test_scoped_search_has_the_bits_of_the_reference(nat, cases, indexes, scope_slab, which):
    family, group, n = which.split()
    c = next(c for c in cases if c.family == family and c.group == group and c.n == int(n))
    lists = WA.scope_lists(c.n, WA.borders_of(4097) + WA.borders_of(c.n))  # the 8 documents on each side of every W4 border
    assert {len(r) for r in lists} >= {c.n, 0, 1, 64, 65} and (c.n < 1025 or {1024, 1025} <= {len(r) for r in lists})
    rows_all = _rows(c)
    pick = _pick(c, 10)
    queries = [c.queries[j] for j in pick for _ in lists]
    qscope = np.asarray([s for _ in pick for s in range(len(lists))], dtype=np.int32)
    ptr, rows = _table(lists)
    gi = indexes(c.csr)
    ws = nat.ScopeWorkspace()
    bad, total = [], 0
    for k in (1, 10, 97):
        s, i = ws.bm25_search(gi, queries, ptr, rows, qscope, k)
        for x, (j, sc) in enumerate((j, sc) for j in pick for sc in range(len(lists))):
            ei, es = WA.ref_scoped_topk(rows_all[j], lists[sc], k)
            total += 1
            bad += _diff(f"{which} k={k} scope of {len(lists[sc])}", j, i[x], s[x], ei, es)
    ws.close()
    _report(bad, total, f"scoped search {which} AMDR_SCOPE_SLAB={scope_slab}")


@pytest.mark.parametrize("which", ["W2 boundary 1024", "W2 order 1024", "W3 all-kept 1100", "W3 empty-groups 1100", "W3 lane-0-and-31 300"])
def test_scoped_step_in_both_phase_orders(nat, cases, indexes, monkeypatch, which):
    """ScopeWorkspace.hybrid in one launch: BM25 scopes of 0, 1 and 64 documents run on wave 0 beside the dense rows
    (scope_bm25_piece<true>), 65 documents on all four waves (<false>); AMDR_SCOPE_OVERLAP=0 pins the second order."""
    import torch
    from test_scope_step_gpu import OUTS, host, run_step, same_bits
    for name in ("AMDR_SCOPE_SLAB", "AMDR_SCOPE_FUSED", "AMDR_SCOPE_OVERLAP"):
        monkeypatch.delenv(name, raising=False)
    dev = torch.device("cuda", 0)
    family, group, n = which.split()
    c = next(c for c in cases if c.family == family and c.group == group and c.n == int(n))
    rng = np.random.default_rng(c.n)
    X = rng.integers(-8, 9, size=(c.n, 4)).astype(np.float32)  # small integers: the dense channel is exact whatever the order
    lists = [np.sort(rng.choice(c.n, size=m, replace=False)).astype(np.int64) for m in (0, 1, 64, 65)]
    lists[2][0] = 0  # document 0 is in every W2 list
    pick = _pick(c, 8)
    queries = [c.queries[j] for j in pick for _ in lists]
    nq = len(queries)
    qs_h = np.asarray([s for _ in pick for s in range(len(lists))], dtype=np.int32)
    ptr, rows = _table(lists)
    qt_h, qp_h = nat.BM25Index.pack_queries(queries)
    Q = torch.from_numpy(rng.integers(-8, 9, size=(nq, 4)).astype(np.float32)).to(dev)
    qt = torch.from_numpy(np.concatenate([qt_h, np.zeros(1, np.int32)])).to(dev)
    qp = torch.from_numpy(qp_h).to(dev)
    tab = (torch.from_numpy(ptr).to(dev), torch.from_numpy(rows).to(dev), torch.from_numpy(qs_h).to(dev), len(lists), 65)
    w = SimpleNamespace(map=None, ws=nat.ScopeWorkspace(), dense=nat.DenseIndex(X), bm25=indexes(c.csr))
    params = nat.make_fuse_params()
    rows_all = _rows(c)
    bad, total = [], 0
    for kd, kb in ((10, 10), (1, 1), (16, 16)):
        assert nat.hybrid_scope_plan(nq, kd, kb, 0, 65, 65)[0]  # the one launch
        a = host(run_step(w, params, Q, qt, qp, tab, tab, nq, kd, kb))
        monkeypatch.setenv("AMDR_SCOPE_OVERLAP", "0")
        b = host(run_step(w, params, Q, qt, qp, tab, tab, nq, kd, kb))
        monkeypatch.delenv("AMDR_SCOPE_OVERLAP")
        for name in OUTS:
            assert same_bits(a[name], b[name]), (which, kd, kb, name)
        for x, (j, sc) in enumerate((j, sc) for j in pick for sc in range(len(lists))):
            ei, es = WA.ref_scoped_topk(rows_all[j], lists[sc], kb)
            total += 1
            bad += _diff(f"{which} kb={kb} scope of {len(lists[sc])}", j, a["bm25_ids"][x], a["bm25_scores"][x], ei, es)
    w.ws.close()
    w.dense.close()
    _report(bad, total, f"scoped step {which}")


# ---- the serving step and the long-batch step --------------------------------------------------------------------------
@pytest.mark.parametrize("family,n", [("W1", 1100), ("W2", 1024), ("W3", 300), ("W3", 1100), ("W5", 300), ("W5", 700)])
def test_the_one_launch_serving_step(nat, cases, indexes, family, n):
    """HybridEngine.search_batch of 1-4 queries (hybrid_small_kernel calls bm25_block_query from inside another kernel)
    against the reference, and AMDR_HYBRID_SMALL=1 against =0 in every field."""
    import torch
    from legal_rag_amd.retrieval.engine import HybridEngine
    from test_hybrid_small_gpu import _run, _same
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(n)
    d = 64
    X = rng.standard_normal((n, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    groups = [c for c in _groups(cases, family) if c.n == n]
    assert groups and n <= 2048
    dense = nat.DenseIndex(X)
    eng = HybridEngine(dense, indexes(groups[0].csr), None)
    params = nat.make_fuse_params()
    bad, total, call = [], 0, 0
    for c in groups:
        assert c.csr is groups[0].csr
        rows_all = _rows(c)
        pick = _pick(c, 9 if family == "W1" else 16)
        at = 0
        while at < len(pick):
            nq = 1 + call % 4
            k = (10, 16, 1)[call % 3]
            call += 1
            js = pick[at:at + nq]
            at += nq
            queries = [c.queries[j] for j in js]
            top = [IA.ref_topk(rows_all[j], k) for j in js]
            ei, es = np.stack([t[0] for t in top]), np.stack([t[1] for t in top])
            q = rng.standard_normal((len(js), d)).astype(np.float32)
            qt_h, qp_h = nat.BM25Index.pack_queries(queries)
            Q, qt, qp = torch.from_numpy(q).to(dev), torch.from_numpy(qt_h).to(dev), torch.from_numpy(qp_h).to(dev)
            a = _run(eng, params, k, Q, qt, qp, True)
            b = _run(eng, params, k, Q, qt, qp, False)
            for r, what in ((a, "one launch"), (b, "separate launches")):
                total += 1
                mism = []
                for x, j in enumerate(js):
                    mism += _diff(f"{family} {c.group} n={n} k={k} {what}", j, r["bm25_ids"][x], r["bm25_scores"][x], ei[x], es[x])
                bad += mism[:1]
            _same(a, b, (family, c.group, n, k, js))
    dense.close()
    assert total >= 16
    _report(bad, total, f"serving step {family} n={n}")


def test_the_long_batch_step_on_a_w2_index(nat, cases, indexes, monkeypatch):
    """hybrid_batch_device at its minimum batch: BM25 on the side stream beside the second dense pass against
    AMDR_HYBRID_BATCH=0, all five outputs, and the BM25 lists against the reference."""
    import torch
    import test_hybrid_batch_gpu as HB
    monkeypatch.setenv("AMDR_DENSE_SMALL_HI_MIN", str(HB.MIN_NQ))
    monkeypatch.delenv("AMDR_HYBRID_BATCH", raising=False)
    dev = torch.device("cuda", 0)
    groups = _groups(cases, "W2")
    assert groups[0].n == 1024
    pool = [(c, j) for c in groups for j in range(len(c.queries))]
    nq, kd, kb = HB.MIN_NQ, 10, 10
    take = [pool[x % len(pool)] for x in range(nq)]  # the family's queries, tiled to the batch
    rng = np.random.default_rng(7)
    X = rng.standard_normal((1024, HB.D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    dense = nat.DenseIndex(X)
    assert "dsh_scores_kernel" in dense.plan_info(nq, kd)
    q = rng.standard_normal((nq, HB.D)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    qt_h, qp_h = nat.BM25Index.pack_queries([c.queries[j] for c, j in take])
    inputs = (torch.from_numpy(q).to(dev), torch.from_numpy(np.concatenate([qt_h, np.zeros(1, np.int32)])).to(dev),
              torch.from_numpy(qp_h).to(dev))
    params = nat.make_fuse_params(min_final_score=0.1)
    bm = indexes(groups[0].csr)
    a = HB._run(dense, bm, params, inputs, kd, kb, False)
    b = HB._run(dense, bm, params, inputs, kd, kb, True)
    HB._same(a, b, "W2 overlapped against serial")
    bad = []
    for x, (c, j) in enumerate(take):
        ei, es = IA.ref_topk(_rows(c)[j], kb)
        bad += _diff(f"W2 {c.group} long batch", j, a["bm25_ids"][x], a["bm25_scores"][x], ei, es)
    dense.close()
    _report(bad, nq, "long-batch step W2")

"""The BM25 ranking on the corpora of tests/bm25_image_adversary.py: fp64 scores whose fp32 images tie across the cut, the
larger score on the higher id behind k + 1 or more equal ones (the overflow branch included), and scores outside the
fp32 range (images +-inf, +-0, subnormal).  tests/test_bm25_image_adversary.py proves that the data reaches the check
of bm25_select_f32; here every result is compared with the numpy fp64 reference of that module and with nothing else:
ids exactly, scores bit for bit, under AMDR_BM25_SELECT=1 and =0, through search, search_device (eager and replayed from
a graph) and the one-launch serving step.  No tolerance anywhere."""
import os

import numpy as np
import pytest

import bm25_image_adversary as IA

pytestmark = pytest.mark.gpu

FAMILIES = ("F1", "F2", "F3a", "F3b", "F4", "control")


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    return _native


@pytest.fixture(scope="module")
def cases():
    return IA.hand_made()


def _index(nat, csr):
    return nat.BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"], csr["doc_len"], csr["avgdl"],
                         csr["k1"], csr["b"])


def _expected(case, rows=None):
    rows = IA.ref_scores(case.csr, case.queries) if rows is None else rows
    top = [IA.ref_topk(r, case.k) for r in rows]
    return rows, np.stack([t[0] for t in top]), np.stack([t[1] for t in top])


def _check(nat, case, gi=None):
    """plan_info and get_scores are asserted on the spot; returns the queries whose ranking differs from the reference."""
    own = gi is None
    gi = _index(nat, case.csr) if own else gi
    nq = len(case.queries)
    slabs, path = IA.plan_text(case.n, case.k)
    plan = gi.plan_info(nq, case.k)
    assert slabs in plan and path in plan, (case.name, plan)
    rows, ei, es = _expected(case)
    full = gi.get_scores(case.queries)
    assert np.array_equal(full.view(np.uint64), rows.view(np.uint64)), case.name
    s, i = gi.search(case.queries, case.k)
    if own:
        gi.close()
    bad = []
    for q in range(nq):
        if not (np.array_equal(i[q], ei[q]) and np.array_equal(s[q].view(np.uint64), es[q].view(np.uint64))):
            bad.append(f"{case.name} query {q}: n={case.n} k={case.k} returned ids {i[q].tolist()} scores {s[q].tolist()}, "
                       f"expected ids {ei[q].tolist()} scores {es[q].tolist()}")
    return bad


def _report(bad, total, what):
    print(f"{what}: {total - len(bad)} of {total} equal the fp64 reference")
    assert not bad, f"{what}: {len(bad)} of {total} differ from the fp64 reference; the first: {bad[0]}"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("select", ["1", "0"])
def test_hand_made_runs_across_the_cut(nat, cases, monkeypatch, select, family):
    monkeypatch.setenv("AMDR_BM25_SELECT", select)
    mine = [c for c in cases if c.family == family]
    assert len(mine) >= 20
    bad = []
    for c in mine:
        bad += _check(nat, c)
    _report(bad, len(mine), f"{family} AMDR_BM25_SELECT={select}")


@pytest.mark.parametrize("select", ["1", "0"])
def test_fuzz_batches(nat, monkeypatch, select):
    monkeypatch.setenv("AMDR_BM25_SELECT", select)
    bad, total, gi, csr = [], 0, None, None
    for c in IA.fuzz():
        if c.csr is not csr:  # one corpus per size, one search call per depth
            if gi is not None:
                gi.close()
            gi, csr = _index(nat, c.csr), c.csr
        bad += _check(nat, c, gi)
        total += len(c.queries)
    gi.close()
    assert total >= 300
    _report(bad, total, f"F5 AMDR_BM25_SELECT={select}")


def _two_f1(cases):
    pick = [c for c in cases if c.family == "F1" and c.reach and (c.n, c.k) in ((591, 10), (9000, 16))]
    a = next(c for c in pick if c.n == 591 and "register>0" in c.name)
    b = next(c for c in pick if c.n == 9000 and c.slab_ix == 2)
    return a, b


@pytest.mark.parametrize("select", ["1", "0"])
def test_search_device_eager_and_replayed(nat, cases, monkeypatch, select):
    import torch
    monkeypatch.setenv("AMDR_BM25_SELECT", select)
    dev = torch.device("cuda", 0)
    for c in _two_f1(cases):
        q0 = c.queries[0]
        queries = [q0, q0[::-1], [t for t in q0 if t not in c.high]]
        probe = IA.Case(c.family, c.name, c.n, c.k, c.csr, queries)
        _, ei, es = _expected(probe)
        gi = _index(nat, c.csr)
        nq, k = len(queries), c.k
        qt_h, qp_h = nat.BM25Index.pack_queries(queries)
        gi.reserve(nq, k, int(qp_h[-1]))
        qt, qp = torch.from_numpy(qt_h).to(dev), torch.from_numpy(qp_h).to(dev)
        s = torch.zeros((nq, k), dtype=torch.float64, device=dev)
        i = torch.zeros((nq, k), dtype=torch.int64, device=dev)

        def same(what):
            torch.cuda.synchronize()
            assert np.array_equal(i.cpu().numpy(), ei), (c.name, what, i.cpu().numpy().tolist(), ei.tolist())
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
        gi.close()


@pytest.mark.parametrize("n", [591, 2048])
@pytest.mark.parametrize("select", ["1", "0"])
def test_the_one_launch_step(nat, cases, monkeypatch, select, n):
    """HybridEngine.search_batch of 1-4 queries (hybrid_small_kernel calls the same ranking) against the reference, and
    AMDR_HYBRID_SMALL=1 against =0 in every field."""
    import torch
    from legal_rag_amd.retrieval.engine import HybridEngine
    from test_hybrid_small_gpu import _run, _same
    monkeypatch.setenv("AMDR_BM25_SELECT", select)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(n)
    d = 64
    X = rng.standard_normal((n, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    mine = [c for c in cases if c.n == n and c.k in (1, 10, 16) and ((c.family == "F1" and c.reach) or c.family == "F4")]
    assert sum(c.family == "F1" for c in mine) >= 10 and sum(c.family == "F4" for c in mine) >= 10
    bad, total = [], 0
    for c in mine:
        q0 = c.queries[0]
        queries = [q0, [t for t in q0 if t not in c.high], q0[::-1] + [-1, 2 * c.n + 5], q0 + q0[:3]]
        eng = HybridEngine(nat.DenseIndex(X), _index(nat, c.csr), None)
        params = nat.make_fuse_params()
        for nq in (1, 2, 3, 4):
            probe = IA.Case(c.family, c.name, c.n, c.k, c.csr, queries[:nq])
            _, ei, es = _expected(probe)
            q = rng.standard_normal((nq, d)).astype(np.float32)
            qt_h, qp_h = nat.BM25Index.pack_queries(queries[:nq])
            Q, qt, qp = torch.from_numpy(q).to(dev), torch.from_numpy(qt_h).to(dev), torch.from_numpy(qp_h).to(dev)
            a = _run(eng, params, c.k, Q, qt, qp, True)
            b = _run(eng, params, c.k, Q, qt, qp, False)
            total += 1
            for r, what in ((a, "one launch"), (b, "separate launches")):
                if not (np.array_equal(r["bm25_ids"], ei) and np.array_equal(r["bm25_scores"].view(np.uint64), es.view(np.uint64))):
                    bad.append(f"{c.name} nq={nq} {what}: returned ids {r['bm25_ids'].tolist()}, expected {ei.tolist()}")
            _same(a, b, (c.name, nq))
        eng.bm25.close()
        eng.dense.close()
    _report(bad, 2 * total, f"one-launch step n={n} AMDR_BM25_SELECT={select}")


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_non_finite_idf_is_refused(nat, value):
    """The arg-max rounds use -inf as "no document" and the staged selector ranks -inf above NaN: neither order is what a
    caller could mean, and rank_bm25 produces no such idf, so amdr_bm25_create refuses the index."""
    sc = np.linspace(1.0, 2.0, 40)
    sc[17] = value
    csr = IA.csr_per_document(sc)
    with pytest.raises(nat.NativeError, match="idf of term 17 is not finite"):
        _index(nat, csr)
    sc[17] = 1.5
    gi = _index(nat, IA.csr_per_document(sc))  # the same arrays with a finite value are accepted
    assert gi.search([[17, 3]], 2)[1].tolist() == [[17, 3]]
    gi.close()

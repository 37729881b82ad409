"""The long-batch hybrid step as ONE native call (amdr_hybrid_batch_device, csrc/dense.hip): where the dense channel takes
its two-pass form, BM25 runs on the dense handle's side stream beside the second dense pass, forked from and joined to
the caller's stream inside the call.  Checked against the serial calls of the same entry (AMDR_HYBRID_BATCH=0:
amdr_bm25_search_device + amdr_dense_search_fuse_device) in the same process — every byte of every output: dense lists,
BM25 lists, fused ids, vals, mask, count.  AMDR_DENSE_SMALL_HI_MIN is lowered so that batches of a few hundred queries
take the two-pass form; d = 128 keeps every case at a fraction of a second."""
import functools
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu

D = 128
MIN_NQ = 200  # AMDR_DENSE_SMALL_HI_MIN of these tests
GROUP = 2048  # queries per 8 query groups of dsh_scores_kernel's grid (its XCD mapping walks them together)
FIELDS = ("dense_scores", "dense_ids", "bm25_scores", "bm25_ids", "ids", "vals", "mask", "count")


@pytest.fixture(autouse=True)
def _two_pass_from_200(monkeypatch):
    monkeypatch.setenv("AMDR_DENSE_SMALL_HI_MIN", str(MIN_NQ))
    monkeypatch.delenv("AMDR_HYBRID_BATCH", raising=False)


@functools.lru_cache(maxsize=None)
def _index(n, dup=False):
    """(X, dense index, BM25 index, vocabulary size) of a corpus of n rows; dup: rows 10-49 are one row (ties)."""
    from legal_rag_amd import _native
    from oracle import bm25 as OB
    rng = np.random.default_rng(1000 + n)
    X = rng.standard_normal((n, D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    if dup:
        X[10:50] = X[10]
    words = [f"w{i}" for i in range(120)]
    docs = [[words[j] for j in rng.integers(0, 120, size=int(rng.integers(3, 30)))] for _ in range(n)]
    ob = OB.BM25Okapi(docs)
    csr = OB.to_csr(ob)
    bm = _native.BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"], csr["doc_len"], ob.avgdl, ob.k1, ob.b)
    return X, _native.DenseIndex(X), bm, len(csr["vocab"])


def _queries(rng, X, V, nq, seams=()):
    """Device inputs (Q, q_terms, q_ptr) of nq random queries.  At every index of `seams` and the one before it: a query
    with no known token, then a query with an empty CSR range."""
    import torch
    from legal_rag_amd import _native
    q = rng.standard_normal((nq, D)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    toks = [[int(t) for t in rng.integers(-1, V, size=int(rng.integers(1, 12)))] for _ in range(nq)]
    for s in seams:
        if 1 <= s < nq:
            toks[s - 1] = [-1, -1, -1]
            toks[s] = []
    qt, qp = _native.BM25Index.pack_queries(toks)
    dev = torch.device("cuda", 0)
    return (torch.from_numpy(q).to(dev), torch.from_numpy(np.concatenate([qt, np.zeros(1, np.int32)])).to(dev),
            torch.from_numpy(qp).to(dev))


def _outputs(nq, kd, kb):
    import torch
    from legal_rag_amd import _native
    dev = torch.device("cuda", 0)
    mo = kd + kb
    return dict(dense_scores=torch.zeros((nq, kd), dtype=torch.float32, device=dev),
                dense_ids=torch.zeros((nq, kd), dtype=torch.int64, device=dev),
                bm25_scores=torch.zeros((nq, kb), dtype=torch.float64, device=dev),
                bm25_ids=torch.zeros((nq, kb), dtype=torch.int64, device=dev),
                ids=torch.zeros((nq, mo), dtype=torch.int64, device=dev),
                vals=torch.zeros((nq, mo, _native.FUSE_NVALS), dtype=torch.float64, device=dev),
                mask=torch.zeros((nq, mo), dtype=torch.int32, device=dev), count=torch.zeros((nq,), dtype=torch.int32, device=dev))


def _enqueue(dense, bm, params, inputs, kd, kb, out, maps=(None, None), stream=None):
    """One amdr_hybrid_batch_device call on `stream` (None: the current one); no synchronisation."""
    import torch
    from legal_rag_amd import _native
    Q, qt, qp = inputs
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    m0, m1 = (m.data_ptr() if m is not None else 0 for m in maps)
    _native.hybrid_batch_device(dense, bm, params, Q.data_ptr(), qt.data_ptr(), qp.data_ptr(), int(Q.shape[0]), kd, kb, m0, m1,
                                *(out[f].data_ptr() for f in FIELDS), st)


def _host(out):
    import torch
    torch.cuda.synchronize()
    return {f: out[f].cpu().numpy().copy() for f in FIELDS}


def _run(dense, bm, params, inputs, kd, kb, serial, maps=(None, None)):
    old = os.environ.pop("AMDR_HYBRID_BATCH", None)
    if serial:
        os.environ["AMDR_HYBRID_BATCH"] = "0"
    try:
        out = _outputs(int(inputs[0].shape[0]), kd, kb)
        _enqueue(dense, bm, params, inputs, kd, kb, out, maps)
        return _host(out)
    finally:
        os.environ.pop("AMDR_HYBRID_BATCH", None)
        if old is not None:
            os.environ["AMDR_HYBRID_BATCH"] = old


def _same(a, b, what):
    for f in FIELDS:
        assert a[f].shape == b[f].shape and np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)), (what, f)


def test_the_route_and_the_binding_without_a_gpu():
    from legal_rag_amd import _native
    from legal_rag_amd.retrieval import engine as E
    assert E.step_form(True, True, False, False, 5, 10, True) == (E.BM25_THEN_FUSED, False)
    assert E.step_form(True, True, False, False, 37376, 10, False) == (E.BM25_THEN_FUSED, False)
    assert E.step_form(True, True, False, False, 4, 10, True) == (E.ONE_LAUNCH, False)
    assert E.step_form(True, True, True, False, 37376, 10, True) == (E.CHANNELS_SIDE, False)
    assert E.step_form(True, True, False, True, 37376, 10, True) == (E.CHANNELS, True)
    assert _native.SIGNATURES["amdr_hybrid_batch_device"] == _native.SIGNATURES["amdr_hybrid_small_device"]
    assert callable(E.HybridEngine.hybrid_batch)


# the batch sizes: around one and two groups of 2 048 queries (the scores kernel's grid is rounded up to them), less than
# one, odd, the form's minimum and one above it; 199 is below the minimum (the serial calls inside)
@gpu
@pytest.mark.parametrize("n", [33, 70, 591, 1024])
@pytest.mark.parametrize("nq", [GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 1, 300, 777, MIN_NQ, MIN_NQ + 1, MIN_NQ - 1])
def test_overlapped_equals_serial_at_the_batch_edges(n, nq):
    from legal_rag_amd import _native
    X, dense, bm, V = _index(n)
    assert ("dsh_scores_kernel" in dense.plan_info(nq, 10)) == (nq >= MIN_NQ)
    inputs = _queries(np.random.default_rng(n * 31 + nq), X, V, nq, seams=(1, GROUP, 2 * GROUP, nq - 1))
    params = _native.make_fuse_params(min_final_score=0.1)
    _same(_run(dense, bm, params, inputs, 10, 10, False), _run(dense, bm, params, inputs, 10, 10, True), (n, nq))


@gpu
@pytest.mark.parametrize("kd,kb", [(1, 3), (10, 7), (12, 5), (5, 12), (13, 10)])  # kd = 13: outside the two-pass form
def test_overlapped_equals_serial_at_every_depth(kd, kb):
    from legal_rag_amd import _native
    X, dense, bm, V = _index(591)
    assert ("dsh_scores_kernel" in dense.plan_info(GROUP + 77, kd)) == (kd <= 12)
    inputs = _queries(np.random.default_rng(kd * 100 + kb), X, V, GROUP + 77, seams=(GROUP,))
    for method in ("rrf_norm_blend", "weighted_sum", "rrf"):
        params = _native.make_fuse_params(method=method)
        _same(_run(dense, bm, params, inputs, kd, kb, False), _run(dense, bm, params, inputs, kd, kb, True), (kd, kb, method))


@gpu
@pytest.mark.parametrize("n", [70, 1024])
def test_content_at_the_seams(n, monkeypatch):
    import torch
    from legal_rag_amd import _native
    X, dense, bm, V = _index(n, True)
    nq = GROUP + 300
    Q, qt, qp = _queries(np.random.default_rng(n), X, V, nq, seams=(1, GROUP, nq - 1))
    Q[3] = torch.from_numpy(X[10]).to(Q.device)  # the duplicated rows are this query's best: ties at the cut
    Q[GROUP] = torch.from_numpy(X[10]).to(Q.device)
    Q[5, 17] = float("nan")  # no bound for this query: it re-scores its whole row
    Q[GROUP - 1, 0] = float("nan")
    rng = np.random.default_rng(n + 1)
    maps = tuple(torch.from_numpy(rng.permutation(4 * n)[:n].astype(np.int64)).to(Q.device) for _ in range(2))
    params = _native.make_fuse_params(min_final_score=0.05)
    for mp in ((None, None), maps, (maps[0], None)):
        a = _run(dense, bm, params, (Q, qt, qp), 10, 8, False, mp)
        _same(a, _run(dense, bm, params, (Q, qt, qp), 10, 8, True, mp), (n, "maps", mp[0] is not None, mp[1] is not None))
        if mp[0] is None:
            assert a["dense_ids"][3].tolist() == list(range(10, 20)) and a["dense_ids"][GROUP].tolist() == list(range(10, 20))
    before = dense.two_pass_fallbacks()
    monkeypatch.setenv("AMDR_DENSE_SMALL_HI_MARGIN", "1e9")  # every query takes the whole-row fallback
    a = _run(dense, bm, params, (Q, qt, qp), 10, 8, False, maps)
    assert dense.two_pass_fallbacks() - before == nq
    _same(a, _run(dense, bm, params, (Q, qt, qp), 10, 8, True, maps), (n, "whole-row fallback"))


@gpu
@pytest.mark.parametrize("own_stream", [False, True], ids=["default-stream", "own-stream"])
def test_three_calls_back_to_back_reuse_the_workspaces_in_order(own_stream):
    import torch
    from legal_rag_amd import _native
    X, dense, bm, V = _index(591)
    params = _native.make_fuse_params()
    sizes = (GROUP + 1, 2 * GROUP + 1, 777)
    inputs = [_queries(np.random.default_rng(70 + i), X, V, nq, seams=(GROUP,)) for i, nq in enumerate(sizes)]
    serial = [_run(dense, bm, params, inp, 10, 10, True) for inp in inputs]
    outs = [_outputs(nq, 10, 10) for nq in sizes]
    torch.cuda.synchronize()
    st = torch.cuda.Stream() if own_stream else None
    for _ in range(2):  # (the second round finds the side stream and the workspaces warm)
        for inp, out in zip(inputs, outs):
            _enqueue(dense, bm, params, inp, 10, 10, out, stream=st)
    for i, out in enumerate(outs):
        _same(_host(out), serial[i], (own_stream, i))


@gpu
def test_the_call_is_capturable_and_grows_no_workspace():
    import torch
    from legal_rag_amd import _native
    X, dense, bm, V = _index(1024)
    nq, kd, kb = GROUP + 513, 10, 10
    params = _native.make_fuse_params(min_final_score=0.1)
    Q, qt, qp = _queries(np.random.default_rng(3), X, V, nq)
    dense.reserve(nq, kd)
    bm.reserve(nq, kb, int(qt.shape[0]))
    growths = _native.workspace_growths()
    out = _outputs(nq, kd, kb)
    _enqueue(dense, bm, params, (Q, qt, qp), kd, kb, out)  # eager, inside the reserve
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _enqueue(dense, bm, params, (Q, qt, qp), kd, kb, out)
    for seed in (11, 12):
        Q2, qt2, qp2 = _queries(np.random.default_rng(seed), X, V, nq)
        Q.copy_(Q2)
        qt[:min(qt.shape[0], qt2.shape[0])].copy_(qt2[:min(qt.shape[0], qt2.shape[0])])
        qp.copy_(torch.clamp(qp2, max=qt.shape[0] - 1))  # (a shorter term array: the last queries lose their tail)
        g.replay()
        got = _host(out)
        assert _native.workspace_growths() == growths
        _same(got, _run(dense, bm, params, (Q, qt, qp), kd, kb, True), ("replay", seed))
    assert _native.workspace_growths() == growths

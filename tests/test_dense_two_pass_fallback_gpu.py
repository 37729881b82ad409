"""The whole-row exact fallback of the two-pass long-batch form (dense_tail.hip dense_hi_select_fuse_kernel) re-scores a query's
row over that query's own row of the approximate score matrix instead of a per-block LDS buffer.  Checked here: the
fallback's exact scores are the bits the candidate re-scoring computes for the same rows; mass ties among exact scores
(the staged selector reading the row back); a pair whose two halves take different paths; an odd batch whose last pair
is half empty; and the fused step with every query on the fallback against the exact form."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TWO = {"AMDR_DENSE_SMALL_HI": "1", "AMDR_DENSE_SMALL_HI_MIN": "96"}
FORCE = dict(TWO, AMDR_DENSE_SMALL_HI_MARGIN="1e9")  # every query of more than 32 rows: the whole-row fallback
TOL = 2e-6


def _with_env(env, fn):
    old = {n: os.environ.get(n) for n in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for n, v in old.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


def _search(idx, Q, k, env):
    import torch

    def go():
        dev = torch.device("cuda", 0)
        nq = Q.shape[0]
        Qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
        s = torch.empty((nq, k), dtype=torch.float32, device=dev)
        i = torch.empty((nq, k), dtype=torch.int64, device=dev)
        idx.search_device(Qd.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), int(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return s.cpu().numpy(), i.cpu().numpy(), idx.plan_info(nq, k)
    return _with_env(env, go)


def _unit(rng, rows, d):
    A = rng.standard_normal((rows, d)).astype(np.float32)
    return A / np.linalg.norm(A, axis=1, keepdims=True)


@pytest.mark.parametrize("n,d,nq,k", [(591, 768, 4097, 10), (1024, 128, 301, 12), (200, 384, 97, 7)])
def test_fallback_scores_are_the_candidate_rescoring_bits(n, d, nq, k):
    from legal_rag_amd import _native
    from oracle import dense as OD
    rng = np.random.default_rng(n * 7 + nq)
    X, Q = _unit(rng, n, d), _unit(rng, nq, d)
    idx = _native.DenseIndex(X, device=0)
    s2, i2, plan = _search(idx, Q, k, TWO)
    before = idx.two_pass_fallbacks()
    sf, i_f, _ = _search(idx, Q, k, FORCE)
    assert plan.startswith("dsh_scores_kernel")
    assert idx.two_pass_fallbacks() - before == nq
    es, ei = OD.flatip_topk(X, Q, k)
    assert np.array_equal(i_f, ei) and np.array_equal(i2, ei)
    # both paths sum a row with the same instructions: the same float bits, row for row
    assert np.array_equal(sf.view(np.uint32), s2.view(np.uint32))
    assert np.max(np.abs(sf - es)) <= TOL
    idx.close()


def test_fallback_mass_ties_and_mixed_pairs():
    from legal_rag_amd import _native
    rng = np.random.default_rng(5)
    d, k = 256, 10
    base = _unit(rng, 4, d)
    X = np.repeat(base, 40, axis=0)  # 40 exact copies of 4 rows: the exact scores tie in masses at every cut
    nq = 151
    Q = _unit(rng, nq, d)
    Q[1::3] *= np.float32(1e20)  # no usable bound: these halves take the fallback, their pair partners may not
    idx = _native.DenseIndex(X, device=0)
    s1, i1, _ = _search(idx, Q, k, {"AMDR_DENSE_SMALL_HI": "0"})
    for env in (TWO, FORCE):
        s2, i2, plan = _search(idx, Q, k, env)
        assert plan.startswith("dsh_scores_kernel")
        assert np.array_equal(i2, i1)  # copies: lower id first; the four blocks are far apart
        for b in range(nq):  # (summation-order noise scales with |q| |x|: unit rows, so with the query's norm)
            assert np.max(np.abs(s2[b] - s1[b])) <= TOL * max(1.0, float(np.linalg.norm(Q[b]))), b
    idx.close()


def test_fused_step_on_the_fallback_equals_exact_form():
    import torch
    from legal_rag_amd import _native
    from legal_rag_amd.retrieval.engine import HybridEngine
    from oracle import bm25 as OB
    rng = np.random.default_rng(9)
    n, d, nq, k = 591, 768, 4097, 10
    X = _unit(rng, n, d)
    words = [f"w{i}" for i in range(300)]
    docs = [[words[j] for j in rng.integers(0, 300, size=int(rng.integers(5, 60)))] for _ in range(n)]
    ob = OB.BM25Okapi(docs)
    csr = OB.to_csr(ob)
    dense = _native.DenseIndex(X)
    eng = HybridEngine(dense, _native.BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"], csr["doc_len"],
                                                ob.avgdl, ob.k1, ob.b), None)
    dev = torch.device("cuda", 0)
    Q = torch.from_numpy(_unit(rng, nq, d)).to(dev)
    qt_h, qp_h = _native.BM25Index.pack_queries([[int(t) for t in rng.integers(0, 300, size=6)] for _ in range(nq)])
    qt, qp = torch.from_numpy(qt_h).to(dev), torch.from_numpy(qp_h).to(dev)
    params = _native.make_fuse_params(min_final_score=0.2)
    fields = ("ids", "vals", "mask", "count", "dense_scores", "dense_ids", "bm25_scores", "bm25_ids")

    def step():
        r = eng.search_batch(params, k, q_emb=Q, q_terms=qt, q_ptr=qp)
        torch.cuda.synchronize()
        return {f: getattr(r, f).cpu().numpy().copy() for f in fields}
    before = dense.two_pass_fallbacks()
    a = _with_env({"AMDR_DENSE_SMALL_HI": "1", "AMDR_DENSE_SMALL_HI_MARGIN": "1e9"}, step)
    assert dense.two_pass_fallbacks() - before == nq
    t = _with_env({"AMDR_DENSE_SMALL_HI": "1"}, step)
    b = _with_env({"AMDR_DENSE_SMALL_HI": "0"}, step)
    for f in fields:  # the fallback and the candidate re-scoring: the same bits everywhere
        assert np.array_equal(a[f], t[f]), f
    assert np.array_equal(a["dense_ids"], b["dense_ids"]) and np.max(np.abs(a["dense_scores"] - b["dense_scores"])) <= TOL
    assert np.array_equal(a["count"], b["count"])
    for qi in range(nq):
        c = int(a["count"][qi])
        assert np.array_equal(a["ids"][qi, :c], b["ids"][qi, :c]) and np.array_equal(a["mask"][qi, :c], b["mask"][qi, :c]), qi

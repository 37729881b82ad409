"""The fp16 first passes against worst-case rounding inputs (tests/rounding_adversary.py): every component of query and
row rounds by ~1/2 ulp in a chosen direction, so the first-pass error reaches a fixed fraction of the proven bound
instead of the random-walk ~1/5 that Gaussian vectors give.

- dense_small_hi.hip: the approximate scores stay inside eps, come within 0.7 of it on the coherent case (a bound half
  as large fails), and equal the CPU model (RNE fp16 operands, exact products) to fp32 accumulation noise — the
  components that round away from zero are where a truncating conversion leaves the model; cases with
  fp16-subnormal operands (one outlier row setting the matrix scale among them) show whether the matrix instruction
  honours subnormal inputs — a flushing MFMA exceeds eps there at d >= 768 and leaves the model at every d.
- The two-pass long-batch step, the dense_hi large scan (both callers of the one bound, csrc/dense_fp16.hpp) and the MaxSim
  two-pass top-k (every pass-1 variant, eps from norm_sum or computed by maxsim_select_kernel) on inversion corpora: the
  fp16 pass ranks competitors above the exact top-k, only the bound keeps the latter among the candidates; ids must
  equal the fp64 oracle's and the exact forms' (ids and score bits), with the fast paths — not a fallback — deciding."""
import numpy as np
import pytest

import rounding_adversary as RA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    return _native


def _approx(nat, X, Q):
    import torch
    dev = torch.device("cuda", 0)
    n, nq = X.shape[0], Q.shape[0]
    idx = nat.DenseIndex(X, device=0)
    ap = nat.DenseSmallApprox(idx)
    ld = (n + 31) // 32 * 32
    S = torch.full((nq, ld), float("nan"), dtype=torch.float32, device=dev)
    eps = torch.empty((nq,), dtype=torch.float32, device=dev)
    Qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    ap.approx_device(Qd.data_ptr(), nq, S.data_ptr(), ld, eps.data_ptr(), int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = S.cpu().numpy()[:, :n].astype(np.float64), eps.cpu().numpy().astype(np.float64)
    ap.close()
    idx.close()
    return out


@pytest.mark.parametrize("d", [128, 768, 1024])
def test_dense_small_first_pass_on_worst_case_rounding(nat, d):
    rng = np.random.default_rng(500 + d)
    cases = [("coherent",) + RA.dense_coherent(rng, d, 40), ("coherent-away",) + RA.dense_coherent(rng, d, 40, away=True),
             ("subnormal",) + RA.dense_subnormal(rng, d, 32),
             ("subnormal-mirror",) + RA.dense_subnormal(rng, d, 32, mirror=True), ("outlier",) + RA.dense_outlier(rng, d, 32)]
    for name, X, Q, row in cases:
        S, eps = _approx(nat, X, Q)
        exact = RA.exact_dense(X, Q)
        # the kernel's eps is the restated bound (fp32 arithmetic on the same terms)
        assert np.allclose(eps, RA.dense_eps(X, Q), rtol=1e-5, atol=0), name
        ratio = np.abs(S - exact) / eps[:, None]
        print(f"OBS dense_small d={d} {name}: max err/eps {ratio.max():.4f}, at the constructed pairs "
              f"{ratio[np.arange(len(Q)), row].min():.4f}..{ratio[np.arange(len(Q)), row].max():.4f}")
        assert ratio.max() <= 1.0, (name, ratio.max())
        if name.startswith("coherent"):
            assert ratio.max() >= 0.7, ratio.max()  # the bound is tight: half of it would not hold
        # the model: fp16 RNE of both scaled operands, exact products; what is left is the fp32 accumulation
        x_scale, q_scale, _ = RA.dense_scales(X, Q)
        qn = np.linalg.norm(Q.astype(np.float64) * q_scale[:, None], axis=1)
        xn = np.linalg.norm(X.astype(np.float64) * x_scale, axis=1)
        tol = 2 * (d + 8) * 2.0 ** -24 * np.outer(qn, xn) / (x_scale * q_scale[:, None])
        dev = np.abs(S - RA.model_dense_hi(X, Q))
        print(f"OBS dense_small d={d} {name}: max |S - model| / accumulation bound {(dev / tol).max():.4f}; "
              f"|S - model(ftz)| / bound at the pairs {(np.abs(S - RA.model_dense_hi(X, Q, ftz=True)) / tol)[np.arange(len(Q)), row].min():.1f}")
        assert np.all(dev <= tol), (name, float((dev / tol).max()))


def _search(idx, Q, k, env, monkeypatch):
    import torch
    for n_, v in env.items():
        monkeypatch.setenv(n_, v)
    dev = torch.device("cuda", 0)
    nq = Q.shape[0]
    Qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    s = torch.empty((nq, k), dtype=torch.float32, device=dev)
    i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    idx.search_device(Qd.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    plan = idx.plan_info(nq, k)
    for n_ in env:
        monkeypatch.delenv(n_)
    return s.cpu().numpy(), i.cpu().numpy(), plan


def _fp32_tol(X, Q, ids):
    """Two fp32 summation orders of the same dot products differ by at most 2 (d + 8) 2^-24 |q||x|."""
    d = X.shape[1]
    qn = np.linalg.norm(Q.astype(np.float64), axis=1)[:, None]
    return 2 * (d + 8) * 2.0 ** -24 * qn * np.linalg.norm(X.astype(np.float64), axis=1)[ids]


@pytest.mark.parametrize("d", [256, 768])
@pytest.mark.parametrize("k", [1, 10, 12])
def test_dense_two_pass_step_on_the_inversion_corpus(nat, monkeypatch, d, k):
    rng = np.random.default_rng(10 * d + k)
    case = RA.dense_inversion(rng, d, k, groups=24, reps=4)  # 96 queries, 24 (k + 20) rows
    X, Q, top = case["X"], case["Q"], case["top"]
    exact = RA.exact_dense(X, Q)
    assert np.array_equal(np.argsort(-exact, axis=1, kind="stable")[:, :k], top)
    idx = nat.DenseIndex(X, device=0)
    two = {"AMDR_DENSE_SMALL_HI": "1", "AMDR_DENSE_SMALL_HI_MIN": "96"}
    before = idx.two_pass_fallbacks()
    s2, i2, plan2 = _search(idx, Q, k, two, monkeypatch)
    assert idx.two_pass_fallbacks() == before  # the margin decided, not the in-kernel fallback
    assert plan2.startswith("dsh_scores_kernel"), plan2
    assert np.array_equal(i2, top)
    # the in-kernel fallback re-scores every row with the same instructions: the same bits
    sf, i_f, _ = _search(idx, Q, k, dict(two, AMDR_DENSE_SMALL_HI_MARGIN="1e9"), monkeypatch)
    assert np.array_equal(i_f, top) and np.array_equal(s2.view(np.uint32), sf.view(np.uint32))
    # the exact form (fp32 matrix instructions, another summation order)
    s1, i1, plan1 = _search(idx, Q, k, {"AMDR_DENSE_SMALL_HI": "0"}, monkeypatch)
    assert not plan1.startswith("dsh_scores_kernel")
    assert np.array_equal(i1, top)
    assert np.all(np.abs(s2.astype(np.float64) - s1) <= _fp32_tol(X, Q, i1))
    assert np.all(np.abs(s2.astype(np.float64) - np.take_along_axis(exact, top, axis=1)) <= _fp32_tol(X, Q, top))
    idx.close()


def test_fused_step_on_the_inversion_corpus(nat):
    import os
    import torch
    from legal_rag_amd.retrieval.engine import HybridEngine
    from oracle import bm25 as OB
    rng = np.random.default_rng(77)
    k = 10
    case = RA.dense_inversion(rng, 768, k, groups=24, reps=5)  # 120 queries, 720 rows
    X, Q, top = case["X"], case["Q"], case["top"]
    n, nq = X.shape[0], Q.shape[0]
    words = [f"w{i}" for i in range(300)]
    docs = [[words[j] for j in rng.integers(0, 300, size=int(rng.integers(5, 60)))] for _ in range(n)]
    ob = OB.BM25Okapi(docs)
    csr = OB.to_csr(ob)
    eng = HybridEngine(nat.DenseIndex(X), nat.BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"],
                                                       csr["doc_len"], ob.avgdl, ob.k1, ob.b), None)
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    qt_h, qp_h = nat.BM25Index.pack_queries([[int(t) for t in rng.integers(0, 300, size=6)] for _ in range(nq)])
    qt, qp = torch.from_numpy(qt_h).to(dev), torch.from_numpy(qp_h).to(dev)
    params = nat.make_fuse_params(min_final_score=0.2)
    two = {"AMDR_DENSE_SMALL_HI": "1", "AMDR_DENSE_SMALL_HI_MIN": "96"}
    out, moved = {}, {}
    for name, env in (("two", two), ("fallback", dict(two, AMDR_DENSE_SMALL_HI_MARGIN="1e9")),
                      ("exact", {"AMDR_DENSE_SMALL_HI": "0"})):
        fb = eng.dense.two_pass_fallbacks()
        os.environ.update(env)
        try:
            r = eng.search_batch(params, k, q_emb=Qd, q_terms=qt, q_ptr=qp)
            torch.cuda.synchronize()
            out[name] = {f: getattr(r, f).cpu().numpy().copy() for f in ("ids", "vals", "mask", "count", "dense_scores", "dense_ids")}
        finally:
            for n_ in env:
                os.environ.pop(n_, None)
        moved[name] = eng.dense.two_pass_fallbacks() - fb
    assert moved["two"] == 0 and moved["fallback"] == nq  # the margin decided; the hook really re-scored every row
    for name in out:
        assert np.array_equal(out[name]["dense_ids"], top), name
    # the fallback re-scores with the same instructions: the fused step's outputs are the same bits.  (Against the exact
    # form only the dense channel is compared: its fp32 summation order differs, and the min-max normalisation of ten
    # scores 1e-4 apart magnifies that noise in the fused values.)
    a, f = out["two"], out["fallback"]
    for fld in ("count", "dense_scores", "dense_ids"):
        assert np.array_equal(a[fld], f[fld]), fld
    for qi in range(nq):
        c = int(a["count"][qi])
        for fld in ("ids", "vals", "mask"):
            assert np.array_equal(a[fld][qi, :c], f[fld][qi, :c]), (fld, qi)
    a, b = out["two"], out["exact"]
    assert np.all(np.abs(a["dense_scores"].astype(np.float64) - b["dense_scores"]) <= _fp32_tol(X, Q, top))


@pytest.mark.parametrize("d", [256, 768])
@pytest.mark.parametrize("nq", [64, 130])
def test_dense_hi_large_scan_on_the_inversion_corpus(nat, monkeypatch, d, nq):
    k = 10
    groups, reps = (16, 4) if nq == 64 else (13, 10)
    rng = np.random.default_rng(d + nq)
    case = RA.dense_inversion(rng, d, k, groups=groups, reps=reps, n_total=9017, tiles=281)
    X, Q, top = case["X"], case["Q"], case["top"]
    assert np.array_equal(np.argsort(-RA.exact_dense(X, Q), axis=1, kind="stable")[:, :k], top)
    out = {}
    for name, hi, tl in (("hi", "1", "1"), ("exact", "0", "1"), ("full", "0", "0")):
        monkeypatch.setenv("AMDR_DENSE_HI", hi)
        monkeypatch.setenv("AMDR_DENSE_TWO_LEVEL", tl)
        idx = nat.DenseIndex(X)
        if name == "hi":
            assert "dense_hi_tilemax_kernel" in idx.plan_info(nq, k), idx.plan_info(nq, k)
        out[name] = idx.search(Q, k)
        if name == "hi":
            out["counters"] = idx.hi_counters()
        idx.close()
    took, bad, _, in_use = out["counters"][:4]
    assert (took, bad, in_use) == (nq, 0, True), out["counters"]  # the fp16 pass answered, not the exact chain
    assert np.array_equal(out["hi"][1], top)
    for other in ("exact", "full"):
        assert np.array_equal(out["hi"][1], out[other][1]), other
        assert np.array_equal(out["hi"][0].view(np.uint32), out[other][0].view(np.uint32)), other


# the driver of the MaxSim forms (one-pass ids == oracle ids; every two-pass variant: the same ids, the same score bits)
# lives beside the data: tests/test_maxsim_two_pass_edges_gpu.py runs it too
_MS_VARIANTS = RA.MS_VARIANTS
_ms_check = RA.ms_check


@pytest.mark.parametrize("k,nc", [(1, 4), (10, 12)])
def test_maxsim_two_pass_on_the_inversion_store(nat, monkeypatch, k, nc):
    rng = np.random.default_rng(900 + k)
    c = RA.maxsim_inversion(rng, 16, k, groups=8, reps=2, nc=nc)  # 16 queries of 16 tokens, 8 (k + nc) documents
    assert 4 * k <= len(c["doc_ptr"]) - 1
    _ms_check(nat, monkeypatch, c["D"], c["doc_ptr"], c["Q"], k, c["top"], _MS_VARIANTS)


def test_maxsim_two_pass_with_subnormal_query_tokens(nat, monkeypatch):
    rng = np.random.default_rng(9)
    c = RA.maxsim_subnormal(rng, 8, 24, 4, 60)
    _ms_check(nat, monkeypatch, c["D"], c["doc_ptr"], c["Q"], 4, None, [{}])

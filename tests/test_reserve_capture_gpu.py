"""The reserve / capture contract of the "_device" calls (include/amdretrieval.h): once amdr_*_reserve(nq_max, k_max) has
run, every call with nq <= nq_max and k <= k_max only enqueues and allocates nothing, so it can be captured into a
hipGraph.  No warm-up anywhere: each handle is created, reserved, and then called over a grid of (nq, k) around the
form boundaries, every form the dispatcher picks inside the reservation named through plan_info.  For every call, in
this order:
  1. no device workspace grew (amdr_workspace_growths, read on the host before anything is synchronised);
  2. the result equals the fp64 oracle (BM25 and fusion bit for bit; dense and MaxSim ids, scores within 1e-4);
  3. only then (dense, BM25, fusion) a subset is captured on a side stream (no eager call in between), replayed twice on
     new inputs written into the same tensors, and each replay compared bit for bit with an eager call and the oracle.
A graph is never replayed after a call that grew a workspace: the growth check fails first, on the host.

The back-to-back tests enqueue two batches through HybridEngine's pinned staging behind a sleeping stream and compare
both with the oracle: a refill of staging the GPU has not read yet would hand batch A batch B's queries."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
DEV = torch.device("cuda", 0)


def _nat():
    from legal_rag_amd import _native
    return _native


def _stream() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def nq_grid(nq_max, lo=1, hi=None):
    hi = nq_max if hi is None else min(hi, nq_max)
    return sorted({q for q in (1, 4, 5, 8, 9, nq_max - 1, nq_max) if lo <= q <= hi})


def k_grid(k_max, hi=None):
    hi = k_max if hi is None else min(hi, k_max)
    return sorted({k for k in (1, 9, 10, 16, 17, k_max - 1, k_max) if 1 <= k <= hi})


def enqueue(fn, what):
    """Run fn() (enqueues "_device" work) and assert that no workspace grew — before any synchronisation."""
    nat = _nat()
    g0 = nat.workspace_growths()
    fn()
    grew = nat.workspace_growths() - g0
    assert grew == 0, f"{what}: a call within the reserve (re)allocated {grew} workspace buffer(s)"


def capture(fn, what):
    """Record fn() on a non-blocking side stream; the growth check runs on the host before the graph exists."""
    nat = _nat()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    g0 = nat.workspace_growths()
    with torch.cuda.graph(g, stream=side):
        fn()
    grew = nat.workspace_growths() - g0
    assert grew == 0, f"{what}: the captured call (re)allocated {grew} workspace buffer(s); the graph is not replayed"
    return g


def unit(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def check_topk(S64, s, i, k, gap=TOL):
    """ids / scores of a top-k against exact fp64 scores S64 [nq, n]: valid distinct ids, each score within TOL of the
    exact score of its id, sorted, the oracle's clear hits present, the oracle's order wherever neighbours are
    separated, padding past n (check_dense / test_maxsim_matches_oracle, vectorised)."""
    nq, n = S64.shape
    kk = min(k, n)
    order = np.argsort(-S64, axis=1, kind="stable")[:, :kk]
    es = np.take_along_axis(S64, order, 1)
    got = i[:, :kk]
    assert got.min() >= 0 and got.max() < n
    assert np.all(np.diff(np.sort(got, axis=1), axis=1) != 0), "repeated id"
    ref = np.take_along_axis(S64, got, 1)
    assert np.max(np.abs(s[:, :kk].astype(np.float64) - ref)) <= TOL
    assert np.all(np.diff(s[:, :kk], axis=1) <= 0)
    kth = es[:, kk - 1:kk]
    assert np.all(ref >= kth - TOL)
    # a position is decided when the oracle's score there is separated from both neighbours — for the k-th, from the
    # (k+1)-th best too, which the top-k leaves out: a near-tie across the cut may go either way in fp32
    full = np.take_along_axis(S64, np.argsort(-S64, axis=1, kind="stable")[:, :kk + 1], 1)
    gaps_ok = np.abs(np.diff(full, axis=1)) > gap
    ones = np.ones((nq, 1), dtype=bool)
    right = gaps_ok[:, :kk] if kk < n else np.concatenate([gaps_ok, ones], 1)
    sep = np.concatenate([ones, gaps_ok[:, :kk - 1]], 1) & right
    assert np.all((got == order)[sep])
    for b in np.nonzero(np.any(got != order, axis=1))[0]:
        clear = es[b] > kth[b, 0] + TOL
        assert set(order[b][clear].tolist()) <= set(got[b].tolist()), b
    if k > n:
        assert np.all(i[:, n:] == -1) and np.all(s[:, n:] == -np.finfo(np.float32).max)


# ---- dense -------------------------------------------------------------------------------------------------------------
DENSE_CASES = {
    # name: (n, d, nq_max, k_max, env, {nq range: plan_info substring}[, depths beside k_grid(k_max)])
    "row-waves-tile-panel": (600, 768, 128, 64, {}, [((1, 4), "dense_all_scores_kernel"),
                                                     ((5, 95), "query-tiles-in-LDS"),
                                                     ((96, 128), "dense_panel_scores_kernel")]),
    "scan-two-level": (20_000, 128, 100, 64, {"AMDR_DENSE_TWO_LEVEL": "1", "AMDR_DENSE_HI": "0"},
                       [((1, 4), "dense_scan_topk_kernel"), ((5, 100), "two-level")]),
    "fp16-first-pass": (20_000, 128, 100, 64, {"AMDR_DENSE_TWO_LEVEL": "1", "AMDR_DENSE_HI": "1"},
                        [((1, 4), "dense_scan_topk_kernel"), ((5, 100), "dense_hi_tilemax_kernel")]),
    "small-corpus-two-pass": (1024, 768, 4096, 12, {}, [((1, 4), "dense_all_scores_kernel"),
                                                       ((5, 95), "query-tiles-in-LDS"),
                                                       ((96, 4095), "dense_panel_scores_kernel"),
                                                       ((4096, 4096), "dsh_scores_kernel")]),
    # the scan's slab lists grid_x(nq, k) * nq * k * 8 are monotone in neither argument: a dimension outside the MFMA
    # forms (every batch scans; 8 queries take 1 231 360 B, 9 take 720 000), and k = 192 against 256 (half the staging
    # capacity: four queries share a block, 625 row slabs against 313)
    "scan-only-dim": (200_000, 100, 9, 10, {}, [((1, 9), "dense_scan_topk_kernel")]),
    "scan-deep-k": (20_000, 128, 4, 256, {}, [((1, 4), "dense_scan_topk_kernel")], (191, 192, 193)),
}


@pytest.mark.parametrize("case", list(DENSE_CASES))
def test_dense_reserve_then_capture(case, monkeypatch):
    nat = _nat()
    n, d, nq_max, k_max, env, forms = DENSE_CASES[case][:6]
    ks = sorted(set(k_grid(k_max)).union(*DENSE_CASES[case][6:]))
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    rng = np.random.default_rng(len(case) * 31 + n)
    X = unit(rng, (n, d))
    X64 = X.astype(np.float64)
    idx = nat.DenseIndex(X)
    idx.reserve(nq_max, k_max)
    Qall = unit(rng, (nq_max, d))
    S_all = Qall.astype(np.float64) @ X64.T
    Qd = torch.from_numpy(Qall).to(DEV)
    seen = set()
    for nq in nq_grid(nq_max):
        for k in ks:
            plan = idx.plan_info(nq, k)
            want = [f for (lo, hi), f in forms if lo <= nq <= hi]
            assert len(want) == 1 and want[0] in plan, (case, nq, k, plan)
            seen.add(want[0])
            s = torch.empty((nq, k), dtype=torch.float32, device=DEV)
            i = torch.empty((nq, k), dtype=torch.int64, device=DEV)
            enqueue(lambda: idx.search_device(Qd.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), _stream()),
                    f"dense {case} nq={nq} k={k}")
            torch.cuda.synchronize()
            check_topk(S_all[:nq], s.cpu().numpy(), i.cpu().numpy(), k)
    assert seen == {f for _, f in forms}, (case, seen)
    print(f"dense {case}: forms {sorted(seen)} checked by plan_info and against the oracle, no workspace growth")
    # capture: the largest batch at a shallow and at the deepest k, the smallest at k_max
    for nq, k in ((nq_max, 10 if k_max >= 10 else k_max), (nq_max, k_max), (4, k_max)):
        Q = torch.empty((nq, d), dtype=torch.float32, device=DEV)
        s = torch.empty((nq, k), dtype=torch.float32, device=DEV)
        i = torch.empty((nq, k), dtype=torch.int64, device=DEV)
        g = capture(lambda: idx.search_device(Q.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), _stream()),
                    f"dense {case} nq={nq} k={k}")
        for seed in (1, 2):
            q = unit(np.random.default_rng(seed * 1000 + nq + k), (nq, d))
            Q.copy_(torch.from_numpy(q))
            g.replay()
            torch.cuda.synchronize()
            gs, gi = s.cpu().numpy(), i.cpu().numpy()
            es_ = torch.empty_like(s)
            ei_ = torch.empty_like(i)
            enqueue(lambda: idx.search_device(Q.data_ptr(), nq, k, es_.data_ptr(), ei_.data_ptr(), _stream()),
                    f"dense {case} eager nq={nq} k={k}")
            torch.cuda.synchronize()
            assert np.array_equal(gi, ei_.cpu().numpy()) and np.array_equal(gs.view(np.uint32),
                                                                            es_.cpu().numpy().view(np.uint32))
            check_topk(q.astype(np.float64) @ X64.T, gs, gi, k)
    print(f"dense {case}: captured nq={nq_max}/4 replays equal eager and the oracle")
    idx.close()


# ---- BM25 --------------------------------------------------------------------------------------------------------------
def _bm25_corpus(rng, n, vocab=300):
    from oracle import bm25 as OB
    words = [f"w{j}" for j in range(vocab)]
    docs = [[words[j] for j in rng.integers(0, vocab, size=int(rng.integers(3, 40)))] for _ in range(n)]
    ob = OB.BM25Okapi(docs)
    return ob, OB.to_csr(ob)


def _bm25_index(ob, csr):
    return _nat().BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"], csr["doc_len"], ob.avgdl,
                            ob.k1, ob.b)


def _bm25_queries(rng, csr, nq, t):
    """nq queries of exactly t term ids each (some unknown: -1), so q_ptr stays the same when new terms are written."""
    V = len(csr["vocab"])
    return rng.integers(-1, V, size=(nq, t)).astype(np.int32)


def _bm25_oracle(ob, csr, terms):
    """fp64 score rows of the reference expression (oracle/bm25.py) for term-id queries [nq, t]."""
    inv = list(csr["vocab"])
    return np.stack([ob.get_scores([inv[t] if t >= 0 else "<unk>" for t in row]) for row in terms])


def _bm25_check(S, s, i, k):
    order = np.argsort(-S, axis=1, kind="stable")[:, :k]  # stable sort: ties -> lower doc id
    assert np.array_equal(i, order)
    assert np.array_equal(s.view(np.uint64), np.take_along_axis(S, order, 1).view(np.uint64))


BM25_CASES = {
    # name: (n_docs, nq_max, k_max, {k range: plan_info substring})
    "one-slab": (591, 64, 64, [((1, 64), "slabs=1 ")]),
    "slabs-argmax-and-staged": (5000, 64, 18, [((1, 17), "arg-max"), ((18, 18), "staged selector")]),
    "2049-docs-reserve-29": (2049, 9, 29, [((1, 28), "slabs=2 "), ((29, 29), "slabs=1 ")]),
}


@pytest.mark.parametrize("case", list(BM25_CASES))
def test_bm25_reserve_then_capture(case):
    n, nq_max, k_max, forms = BM25_CASES[case]
    rng = np.random.default_rng(n + 7)
    ob, csr = _bm25_corpus(rng, n)
    idx = _bm25_index(ob, csr)
    T = 6
    idx.reserve(nq_max, k_max, nq_max * T)
    terms = _bm25_queries(rng, csr, nq_max, T)
    S = _bm25_oracle(ob, csr, terms)
    qt = torch.from_numpy(terms.reshape(-1).copy()).to(DEV)
    qp = torch.from_numpy(np.arange(nq_max + 1, dtype=np.int64) * T).to(DEV)
    seen = set()
    for nq in nq_grid(nq_max):
        for k in k_grid(k_max):
            plan = idx.plan_info(nq, k)
            want = [f for (lo, hi), f in forms if lo <= k <= hi]
            assert len(want) == 1 and want[0] in plan, (case, nq, k, plan)
            if n > 2048:
                assert "slabs=1 " not in plan or k == k_max, plan
            seen.add(want[0])
            s = torch.empty((nq, k), dtype=torch.float64, device=DEV)
            i = torch.empty((nq, k), dtype=torch.int64, device=DEV)
            enqueue(lambda: idx.search_device(qt.data_ptr(), qp.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), _stream()),
                    f"bm25 {case} nq={nq} k={k}")
            torch.cuda.synchronize()
            _bm25_check(S[:nq], s.cpu().numpy(), i.cpu().numpy(), k)
    assert seen == {f for _, f in forms}, (case, seen)
    print(f"bm25 {case}: forms {sorted(seen)} checked by plan_info and bit for bit against the oracle, no growth")
    for nq, k in ((nq_max, 9), (nq_max, k_max), (1, k_max - 1)):
        t_d = torch.empty((nq * T,), dtype=torch.int32, device=DEV)
        p_d = qp[: nq + 1].clone()
        s = torch.empty((nq, k), dtype=torch.float64, device=DEV)
        i = torch.empty((nq, k), dtype=torch.int64, device=DEV)
        g = capture(lambda: idx.search_device(t_d.data_ptr(), p_d.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(),
                                              _stream()), f"bm25 {case} nq={nq} k={k}")
        for seed in (1, 2):
            new = _bm25_queries(np.random.default_rng(seed * 100 + nq + k), csr, nq, T)
            t_d.copy_(torch.from_numpy(new.reshape(-1).copy()))
            g.replay()
            torch.cuda.synchronize()
            gs, gi = s.cpu().numpy(), i.cpu().numpy()
            es_, ei_ = torch.empty_like(s), torch.empty_like(i)
            enqueue(lambda: idx.search_device(t_d.data_ptr(), p_d.data_ptr(), nq, k, es_.data_ptr(), ei_.data_ptr(),
                                              _stream()), f"bm25 {case} eager nq={nq} k={k}")
            torch.cuda.synchronize()
            assert np.array_equal(gi, ei_.cpu().numpy()) and np.array_equal(gs.view(np.uint64),
                                                                            es_.cpu().numpy().view(np.uint64))
            _bm25_check(_bm25_oracle(ob, csr, new), gs, gi, k)
    print(f"bm25 {case}: captured replays equal eager and the oracle")
    idx.close()


# ---- MaxSim ------------------------------------------------------------------------------------------------------------
MAXSIM_CASES = {
    # name: (n_docs, nq_max, k_max): per-pair below 8 queries; from 8 the two-pass form while 4 k <= n_docs, else ring
    "74-docs-reserve-80": (74, 64, 80),
}


def _maxsim_form(nat, idx, n, nq, k):
    plan = idx.plan_info(nq)
    if nq < 8:
        assert "maxsim_scores_h_kernel" in plan, plan
        return "per-pair"
    two = nat.maxsim_workspace_plan(n, True, nq, k, nq, k)[1] > (nq * n * 4 + 255) // 256 * 256
    assert "two-pass" in plan and "maxsim_scores_ring_kernel" in plan, plan
    assert two == (4 * k <= n), (n, nq, k)
    return "two-pass" if two else "ring"


@pytest.mark.parametrize("case", list(MAXSIM_CASES))
def test_maxsim_reserve_then_call(case):
    """Every form inside reserve(64, 80) on 74 documents — per-pair, ring, and the two-pass form the old reserve did not
    cover — allocates nothing and matches the oracle.  (Eager calls only: no MaxSim capture here.)"""
    from oracle import maxsim as OM
    nat = _nat()
    n, nq_max, k_max = MAXSIM_CASES[case]
    rng = np.random.default_rng(n)
    lens = rng.integers(1, 65, size=n)
    lens[:4] = [1, 31, 32, 33]
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    D = unit(rng, (int(doc_ptr[-1]), 128))
    idx = nat.MaxSimIndex(D, doc_ptr)
    idx.reserve(nq_max, k_max)
    Qall = unit(rng, (nq_max, 32, 128))
    S = OM.maxsim_scores(Qall, D, doc_ptr)
    Qd = torch.from_numpy(Qall).to(DEV)
    seen = set()
    for nq in nq_grid(nq_max):
        for k in k_grid(k_max):
            seen.add(_maxsim_form(nat, idx, n, nq, k))
            s = torch.empty((nq, k), dtype=torch.float32, device=DEV)
            i = torch.empty((nq, k), dtype=torch.int64, device=DEV)
            enqueue(lambda: idx.search_device(Qd.data_ptr(), nq, 32, k, s.data_ptr(), i.data_ptr(), _stream()),
                    f"maxsim {case} nq={nq} k={k}")
            torch.cuda.synchronize()
            check_topk(S[:nq], s.cpu().numpy(), i.cpu().numpy(), k, gap=2 * TOL)
    assert seen == {"per-pair", "ring", "two-pass"}, seen
    print(f"maxsim {case}: forms {sorted(seen)} checked by plan_info and against the oracle, no workspace growth")
    idx.close()


# ---- fusion: dense + fuse as one call, and the one-launch serving step --------------------------------------------------
def _fused_oracle(ds, di, bs, bi, count, ids, vals):
    """The fusion of the kernel's own dense list and the BM25 list (bit-exact against the oracle already), bit for bit
    (oracle/fusion.py: the reference's _fuse with its default knobs = make_fuse_params' defaults)."""
    from oracle import fusion as OF
    for q in range(di.shape[0]):
        dl = [(int(x), float(v)) for x, v in zip(di[q], ds[q]) if x >= 0]
        bl = [(int(x), float(v)) for x, v in zip(bi[q], bs[q]) if x >= 0]
        exp = OF.fuse(dl, bl, [], {})
        c = int(count[q])
        assert c == len(exp), (q, c, len(exp))
        assert ids[q, :c].tolist() == [h["id"] for h in exp], q
        assert vals[q, :c, 0].tolist() == [h["score"] for h in exp], q


def test_fuse_and_hybrid_small_reserve_then_capture():
    nat = _nat()
    rng = np.random.default_rng(591)
    n, d, T, kb = 591, 384, 6, 10
    ob, csr = _bm25_corpus(rng, n)
    X = unit(rng, (n, d))
    dense = nat.DenseIndex(X)
    bm = _bm25_index(ob, csr)
    params = nat.make_fuse_params()
    nq_max, k_max = 64, 24
    dense.reserve(nq_max, k_max)
    bm.reserve(nq_max, kb, nq_max * T)
    Qall = unit(rng, (nq_max, d))
    S = Qall.astype(np.float64) @ X.astype(np.float64).T
    terms = _bm25_queries(rng, csr, nq_max, T)
    SB = _bm25_oracle(ob, csr, terms)
    Qd = torch.from_numpy(Qall).to(DEV)
    qt = torch.from_numpy(terms.reshape(-1).copy()).to(DEV)
    qp = torch.from_numpy(np.arange(nq_max + 1, dtype=np.int64) * T).to(DEV)

    def outs(nq, k):
        mo = k + kb
        return dict(ds=torch.empty((nq, k), dtype=torch.float32, device=DEV),
                    di=torch.empty((nq, k), dtype=torch.int64, device=DEV),
                    bs=torch.empty((nq, kb), dtype=torch.float64, device=DEV),
                    bi=torch.empty((nq, kb), dtype=torch.int64, device=DEV),
                    ids=torch.empty((nq, mo), dtype=torch.int64, device=DEV),
                    vals=torch.empty((nq, mo, nat.FUSE_NVALS), dtype=torch.float64, device=DEV),
                    mask=torch.empty((nq, mo), dtype=torch.int32, device=DEV),
                    count=torch.empty((nq,), dtype=torch.int32, device=DEV))

    def run_fuse(o, Q, t, p, nq, k):
        bm.search_device(t.data_ptr(), p.data_ptr(), nq, kb, o["bs"].data_ptr(), o["bi"].data_ptr(), _stream())
        dense.search_fuse_device(params, Q.data_ptr(), nq, k, (o["bi"].data_ptr(), o["bs"].data_ptr(), kb, 0), 0,
                                 o["ds"].data_ptr(), o["di"].data_ptr(), o["ids"].data_ptr(), o["vals"].data_ptr(),
                                 o["mask"].data_ptr(), o["count"].data_ptr(), _stream())

    def run_small(o, Q, t, p, nq, k):
        plan = nat.hybrid_small_plan(dense, bm, nq, k, kb, 0, 0, o["ds"].data_ptr(), o["di"].data_ptr(),
                                     o["bs"].data_ptr(), o["bi"].data_ptr(), o["ids"].data_ptr(), o["vals"].data_ptr(),
                                     o["mask"].data_ptr(), o["count"].data_ptr())
        nat.hybrid_small_device(plan, params, Q.data_ptr(), t.data_ptr(), p.data_ptr(), _stream())

    def check(o, S_, SB_, k):
        h = {f: v.cpu().numpy() for f, v in o.items()}
        check_topk(S_, h["ds"], h["di"], k)
        _bm25_check(SB_, h["bs"], h["bi"], kb)
        _fused_oracle(h["ds"], h["di"], h["bs"], h["bi"], h["count"], h["ids"], h["vals"])
        return h

    for name, run, nq_hi in (("search_fuse_device", run_fuse, nq_max), ("hybrid_small_device", run_small, 4)):
        for nq in nq_grid(nq_hi):
            for k in k_grid(k_max):
                o = outs(nq, k)
                enqueue(lambda: run(o, Qd, qt, qp, nq, k), f"{name} nq={nq} k={k}")
                torch.cuda.synchronize()
                check(o, S[:nq], SB[:nq], k)
        print(f"{name}: nq <= {nq_hi}, k <= {k_max} checked against the oracle (fusion bit for bit), no growth")
        for nq, k in ((nq_hi, 10), (1, k_max)):
            Q = torch.empty((nq, d), dtype=torch.float32, device=DEV)
            t_d = torch.empty((nq * T,), dtype=torch.int32, device=DEV)
            p_d = qp[: nq + 1].clone()
            o = outs(nq, k)
            g = capture(lambda: run(o, Q, t_d, p_d, nq, k), f"{name} nq={nq} k={k}")
            for seed in (1, 2):
                r = np.random.default_rng(seed * 77 + nq + k)
                q, new = unit(r, (nq, d)), _bm25_queries(r, csr, nq, T)
                Q.copy_(torch.from_numpy(q))
                t_d.copy_(torch.from_numpy(new.reshape(-1).copy()))
                g.replay()
                torch.cuda.synchronize()
                h = check(o, q.astype(np.float64) @ X.astype(np.float64).T, _bm25_oracle(ob, csr, new), k)
                e = outs(nq, k)
                enqueue(lambda: run(e, Q, t_d, p_d, nq, k), f"{name} eager nq={nq} k={k}")
                torch.cuda.synchronize()
                for f, v in e.items():
                    v = v.cpu().numpy()
                    if f in ("ids", "vals", "mask"):  # entries past count[q] are unspecified
                        for b in range(nq):
                            c = int(h["count"][b])
                            assert np.array_equal(v[b, :c].view(np.uint8), h[f][b, :c].view(np.uint8)), (name, f, b)
                    else:
                        assert np.array_equal(v.view(np.uint8), h[f].view(np.uint8)), (name, f)
        print(f"{name}: captured replays equal eager and the oracle")
    dense.close()
    bm.close()


# ---- back-to-back batches through the engine's pinned staging --------------------------------------------------------
def _engine_case(rng, n=591, d=384):
    from legal_rag_amd.retrieval.engine import HybridEngine
    nat = _nat()
    ob, csr = _bm25_corpus(rng, n)
    X = unit(rng, (n, d))
    eng = HybridEngine(nat.DenseIndex(X), _bm25_index(ob, csr), None, device=0,
                       tokenizer=nat.DeviceTokenizer(nat.Tokenizer(list(csr["vocab"]))))
    return eng, ob, csr, X


def _sleep_then(fn):
    """fn() enqueued behind ~50 ms of GPU sleep: the host runs ahead of every copy it enqueues."""
    torch.cuda._sleep(int(5e7))
    return fn()


def _check_batch(ob, csr, X, Q, words, res, k):
    from oracle import bm25 as OB
    from oracle import fusion as OF
    S = Q.astype(np.float64) @ X.astype(np.float64).T
    ds, di = res["dense_scores"], res["dense_ids"]
    check_topk(S, ds, di, k)
    for q, toks in enumerate(words):
        exp_b = OB.search(ob, toks, k)
        assert res["bm25_ids"][q].tolist() == [e[0] for e in exp_b], q
        assert res["bm25_scores"][q].tolist() == [e[1] for e in exp_b], q
        exp = OF.fuse([(int(x), float(v)) for x, v in zip(di[q], ds[q])], exp_b, [], {})
        c = int(res["count"][q])
        assert c == len(exp) and res["ids"][q, :c].tolist() == [h["id"] for h in exp], q


def _snap(torch_res):
    """Copies of a result's tensors, enqueued on the stream (the engine reuses its output buffers per batch)."""
    return {f: getattr(torch_res, f).clone() for f in
            ("ids", "count", "dense_scores", "dense_ids", "bm25_scores", "bm25_ids")}


@pytest.mark.parametrize("path", ["csr", "text"])
def test_back_to_back_batches_through_pinned_staging(path):
    from legal_rag_amd.text import jieba_cut
    nat = _nat()
    rng = np.random.default_rng(11 if path == "csr" else 12)
    eng, ob, csr, X = _engine_case(rng)
    inv = list(csr["vocab"])
    nq, k, T = 64, 10, 6
    params = nat.make_fuse_params()
    batches = []
    for b in range(2):
        Q = unit(rng, (nq, X.shape[1]))
        toks = [[inv[t] for t in rng.integers(0, len(inv), size=T)] for _ in range(nq)]
        texts = [" ".join(ws) for ws in toks]
        # the query side the BM25 channel scores: the term list, or the text's tokens (legal_rag_amd/text.py, the
        # executable specification of the device tokeniser: the spaces are tokens too, unknown to the vocabulary)
        words = toks if path == "csr" else [jieba_cut(t) for t in texts]
        batches.append((Q, words, texts, torch.from_numpy(Q).to(DEV)))
    torch.cuda.synchronize()
    snaps = []
    for b, (Q, words, texts, Qd) in enumerate(batches):
        def step():
            if path == "csr":
                qt, qp = nat.BM25Index.pack_queries([[csr["vocab"][w] for w in ws] for ws in words])
                qp_d, qt_d = eng.upload_csr(qp, qt)
                return eng.search_batch(params, k, q_emb=Qd, q_terms=qt_d, q_ptr=qp_d)
            ptrs, lens, total, _, keep = nat.utf8_views(texts)
            blob, offs = eng.upload_text(ptrs, lens, total)  # (packed into pinned staging on the host: texts may go)
            return eng.search_batch(params, k, q_emb=Qd, q_text=(blob, offs))
        # batch A is enqueued behind the sleep; batch B's staging is filled while A's copy has not run yet
        res = _sleep_then(step) if b == 0 else step()
        snaps.append(_snap(res))
    torch.cuda.synchronize()  # once, after both batches
    for (Q, words, _, _), snap in zip(batches, snaps):
        _check_batch(ob, csr, X, Q, words, {f: v.cpu().numpy() for f, v in snap.items()}, k)
    print(f"back-to-back {path}: both batches match the oracle")

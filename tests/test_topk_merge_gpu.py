"""The merge of per-part top-k lists (csrc/topk_merge.hip) where no other test reaches it directly: the C entries
amdr_merge_topk_f32/f64_device against oracle/dense.py merge_topk on hand-made edge inputs, and the packed-list
instantiations behind the dense forms and BM25 with ties that straddle a slab boundary.

Every case here passes at the commit before the merge kernels were made one (the file is coverage of a refactor)."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FLT_MAX = np.float32(np.finfo(np.float32).max)
DBL_MAX = np.float64(np.finfo(np.float64).max)
# The NaN the selector gives back for ANY NaN it ranked (key 1 of ord32 / ord64, topk.hpp): the inputs carry this one,
# so that "the bits that went in" can be asked of every hit.
NAN32 = np.array([0xFFFFFFFE], dtype=np.uint32).view(np.float32)[0]
NAN64 = np.array([0xFFFFFFFFFFFFFFFE], dtype=np.uint64).view(np.float64)[0]


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- A: merge_topk_device ----------------------------------------------------------------------------------------------
POOL = [-1.5, -1.0, -0.0, 0.0, 0.0, 0.5, 1.0, 1.0, 2.0, 1e30, -1e30]  # few values: equal scores in different parts


def merge_inputs(rng, W, nq, k_in, dt):
    """scores [W, nq, k_in], ids [W, nq, k_in] (unique per query, half of them above 2^32).  Per query: padding (-1,
    carrying a LARGE score) scattered through every part and closing every odd part, one NaN, a -0.0 / +0.0 pair in
    different parts where there are two; the last of three queries is all padding."""
    nan = NAN32 if dt == np.float32 else NAN64
    s = rng.choice(np.asarray(POOL, dtype=dt), size=(W, nq, k_in))
    some = rng.random((W, nq, k_in)) < 0.3
    s[some] = rng.standard_normal(int(some.sum())).astype(dt)
    ids = np.empty((W, nq, k_in), dtype=np.int64)
    for q in range(nq):
        p = rng.permutation(W * k_in).astype(np.int64)
        ids[:, q, :] = (3 * p + np.where(p % 2 == 1, 1 << 33, 0)).reshape(W, k_in)
    pad = rng.random((W, nq, k_in)) < 0.2
    pad[1::2, :, k_in - (k_in + 3) // 4:] = True
    if nq == 3:
        pad[:, 2, :] = True
    for q in range(nq):
        live = np.argwhere(~pad[:, q, :])
        if len(live) >= 2:
            w, j = live[rng.integers(len(live))]
            s[w, q, j] = nan
        if len(live) >= 4:
            a, b = live[0], live[-1]  # the first and the last part that have an entry
            if not (np.isnan(s[a[0], q, a[1]]) or np.isnan(s[b[0], q, b[1]])):
                s[a[0], q, a[1]], s[b[0], q, b[1]] = (-0.0, 0.0) if q % 2 == 0 else (0.0, -0.0)
    s[pad] = 9e9
    ids[pad] = -1
    return s, ids


@pytest.mark.parametrize("W", [1, 2, 5])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_merge_topk_device_matches_the_oracle(nat, dt, W):
    from oracle import dense as OD
    rng = np.random.default_rng(1000 + W + (0 if dt == np.float32 else 50))
    f64 = dt == np.float64
    seen_nan = seen_zero = seen_big = 0
    for nq in (1, 3):
        for k_in in (1, 10, 64, 65, 256):
            s, ids = merge_inputs(rng, W, nq, k_in, dt)
            ds, di = torch.from_numpy(s).to(DEV), torch.from_numpy(ids).to(DEV)
            for k_out in sorted({1, k_in, min(256, W * k_in)}):
                os_ = torch.empty((nq, k_out), dtype=ds.dtype, device=DEV)
                oi_ = torch.empty((nq, k_out), dtype=torch.int64, device=DEV)
                nat.merge_topk_device(ds.data_ptr(), di.data_ptr(), W, nq, k_in, k_out, os_.data_ptr(), oi_.data_ptr(),
                                      f64=f64, stream=torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                gs, gi = os_.cpu().numpy(), oi_.cpu().numpy()
                es, ei = OD.merge_topk(list(s), list(ids), k_out)
                case = (W, nq, k_in, k_out)
                assert np.array_equal(gi, ei), case
                hit = ei >= 0
                want = np.where(es == 0, dt(0.0), es)  # the one exception: -0.0 comes back as +0.0 (ord32 / ord64)
                assert np.array_equal(bits(gs)[hit], bits(want)[hit]), case
                assert np.all(gs[~hit] == (-DBL_MAX if f64 else -FLT_MAX)), case  # (the oracle pads fp64 with -inf)
                seen_nan += int(np.isnan(gs[hit]).sum())
                seen_zero += int((np.signbit(es) & (es == 0) & hit).sum())
                seen_big += int((gi >= (1 << 32)).sum())
    assert seen_nan and seen_zero and seen_big  # the edges were in the results, not only in the inputs


def test_merge_topk_device_any_nan_comes_back_a_nan(nat):
    """A NaN of another payload ranks the same (behind -1e30, ahead of padding); what comes back is A NaN."""
    s = np.array([[[np.nan, 1.0, 0.0]], [[-1e30, 0.0, 0.0]]], dtype=np.float32)
    ids = np.array([[[4, 6, -1]], [[2, -1, -1]]], dtype=np.int64)
    ds, di = torch.from_numpy(s).to(DEV), torch.from_numpy(ids).to(DEV)
    os_ = torch.empty((1, 5), dtype=torch.float32, device=DEV)
    oi_ = torch.empty((1, 5), dtype=torch.int64, device=DEV)
    nat.merge_topk_device(ds.data_ptr(), di.data_ptr(), 2, 1, 3, 5, os_.data_ptr(), oi_.data_ptr(), f64=False,
                          stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    gs, gi = os_.cpu().numpy()[0], oi_.cpu().numpy()[0]
    assert gi.tolist() == [6, 2, 4, -1, -1]
    assert gs[0] == 1.0 and gs[1] == np.float32(-1e30) and np.isnan(gs[2]) and np.all(gs[3:] == -FLT_MAX)


# ---- B: dense ties that straddle slabs --------------------------------------------------------------------------------
def small_int_rows(rng, distinct, n, d):
    """n rows of integers in -2 .. 2, row r = row r mod `distinct`: fp32 dots are exact in any order, and every score
    occurs again `distinct` rows further on — on both sides of any slab boundary."""
    base = rng.integers(-2, 3, size=(distinct, d)).astype(np.float32)
    return np.tile(base, ((n + distinct - 1) // distinct, 1))[:n].copy()


def assert_dense_equals_flatip(idx, X, Q, k):
    from oracle import dense as OD
    s, i = idx.search(Q, k)
    es, ei = OD.flatip_topk(X, Q, k)
    assert np.array_equal(i, ei), k
    assert np.all(s == es), k  # integer-valued: == on the scores
    m = min(k, X.shape[0])
    assert np.all(i[:, m:] == -1) and np.all(s[:, m:] == -FLT_MAX)
    assert np.all(i[:, :m] >= 0)


@pytest.mark.parametrize("nq", [1, 3, 5])
def test_dense_ties_across_slabs_300_rows(nat, nq):
    """n = 300, d = 64: whichever form the route gives these calls (plan_info), lists of several slabs or one."""
    rng = np.random.default_rng(300 + nq)
    X = small_int_rows(rng, 37, 300, 64)
    Q = rng.integers(-2, 3, size=(nq, 64)).astype(np.float32)
    idx = nat.DenseIndex(X)
    for k in (1, 10, 65, 256):
        assert_dense_equals_flatip(idx, X, Q, k)
    idx.close()
    idx = nat.DenseIndex(X[:200])  # k = 256 beyond the rows: the -1 / -FLT_MAX tail
    assert_dense_equals_flatip(idx, X[:200], Q, 256)
    idx.close()


@pytest.mark.parametrize("d,nq", [(64, 1), (64, 3), (32, 5)])
def test_dense_ties_across_slabs_gemv_scan(nat, d, nq):
    """The GEMV scan itself (dense_scan_topk_kernel: above 16 384 rows with fewer than five queries, or a dimension the
    matrix-instruction forms do not take) with its 1, 4 and 8 queries per block, many row slabs and the merge."""
    rng = np.random.default_rng(16448 + d + nq)
    n = 16448
    X = small_int_rows(rng, 500, n, d)
    Q = rng.integers(-2, 3, size=(nq, d)).astype(np.float32)
    idx = nat.DenseIndex(X)
    for k in (1, 10, 65, 256):
        info = idx.plan_info(nq, k)
        g = re.match(r"dense_scan_topk_kernel<NQ=(\d+)> grid=(\d+)x(\d+) \+ \w*merge\w*kernel", info)
        assert g and int(g.group(2)) > 1, info
        assert_dense_equals_flatip(idx, X, Q, k)
    idx.close()


@pytest.mark.parametrize("k", [10, 256])
def test_dense_ties_across_slabs_batched(nat, k):
    rng = np.random.default_rng(33000 + k)
    n, nq, d = 33000, 12, 64
    X = small_int_rows(rng, 500, n, d)
    Q = rng.integers(-2, 3, size=(nq, d)).astype(np.float32)
    idx = nat.DenseIndex(X)
    info = idx.plan_info(nq, k)
    assert re.search(r"scores_slab_topk_kernel \+ \w*merge\w*kernel", info), info  # more than one slab
    assert_dense_equals_flatip(idx, X, Q, k)
    idx.close()


# ---- C: BM25 across two slabs ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bm25_2049(nat):
    from oracle import bm25 as OB
    rng = np.random.default_rng(2049)
    words = [f"w{i}" for i in range(400)]
    p = 1.0 / np.arange(1, 401)
    p /= p.sum()
    docs = [[words[j] for j in rng.choice(400, size=int(rng.integers(1, 25)), p=p)] for _ in range(2049)]
    docs[2048] = ["w3", "w7", "w7", "w11", "w42"]
    docs[0] = list(docs[2048])     # identical documents in the first and in the last slab
    docs[2047] = list(docs[2048])  # ... and side by side
    ob = OB.BM25Okapi(docs)
    csr = OB.to_csr(ob)
    gi = nat.BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"], csr["doc_len"], ob.avgdl, ob.k1, ob.b)
    queries = [["w7", "w42"], ["w3", "w7", "w11", "w42", "w7"], ["w11"], ["w0", "w1"], ["nothing"], []]
    yield ob, csr, gi, queries
    gi.close()


@pytest.mark.parametrize("k", [10, 40])
def test_bm25_identical_documents_across_two_slabs(bm25_2049, k):
    """k = 10: two slabs (register arg-max rounds) and the merge of their packed lists.  k = 40: the plan takes one slab
    of 2 064 documents and the staged selector — the same lists through the direct store."""
    from oracle import bm25 as OB
    ob, csr, gi, queries = bm25_2049
    slabs = int(re.search(r"slabs=(\d+)", gi.plan_info(len(queries), k)).group(1))
    assert slabs == (2 if k == 10 else 1)
    tid = [[csr["vocab"].get(t, -1) for t in q] for q in queries]
    s, i = gi.search(tid, k)
    for qn, q in enumerate(queries):
        exp = OB.search(ob, q, k)
        assert i[qn].tolist() == [e[0] for e in exp], (k, q)
        assert bits(s[qn]).tolist() == bits(np.asarray([e[1] for e in exp], dtype=np.float64)).tolist(), (k, q)
    # the three copies lead the queries made of their words, the lower row first
    assert i[0, :3].tolist() == [0, 2047, 2048] and i[1, :3].tolist() == [0, 2047, 2048]
    assert s[0, 0] == s[0, 1] == s[0, 2] and s[1, 0] == s[1, 1] == s[1, 2]

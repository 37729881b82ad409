"""The resident fp16 image of the large dense scan's first pass (csrc/dense_hi_image.hpp, dense_hi_image.hip,
dense_hi.hip dense_hi_image_tilemax_kernel; amdr_dense_image_build / _drop / _info).

The image holds exactly the halves the fp16 first pass rounds in registers from the fp32 matrix, so the pass computes
the same tile maxima bit for bit and nothing behind it can tell: ids, score bits, counters, flags and fallbacks are those
of the image-less form (AMDR_DENSE_HI_IMAGE=0 on the same handle), of the exact two-level form and of the full score
matrix.  AMDR_DENSE_TWO_LEVEL=1 AMDR_DENSE_HI=1 pin the route at test sizes, as in test_dense_hi_gpu.py."""
import copy
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

pytestmark = pytest.mark.gpu

IMAGE_KERNEL = "dense_hi_image_tilemax_kernel"
PLAIN_KERNEL = "dense_hi_tilemax_kernel"


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    return _native


@pytest.fixture()
def hi(monkeypatch):
    monkeypatch.setenv("AMDR_DENSE_TWO_LEVEL", "1")
    monkeypatch.setenv("AMDR_DENSE_HI", "1")
    monkeypatch.delenv("AMDR_DENSE_HI_IMAGE", raising=False)
    return monkeypatch


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def same(a, b, what):
    assert np.array_equal(a[1], b[1]), (what, "ids")
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (what, "score bits")


def image_bytes(n, d):
    return (n + 31) // 32 * 32 * d * 2


def scale_exp(X):
    """e of the matrix scale 2^-e: the largest |component| is f 2^e with f in [1/2, 1)"""
    return int(np.frexp(np.nanmax(np.abs(X)))[1])


def with_and_without(idx, Q, k, mp, what):
    """Searches one handle with its image and with AMDR_DENSE_HI_IMAGE=0; the plans name the two kernels; the results
    are equal, ids and bits.  Returns them."""
    mp.delenv("AMDR_DENSE_HI_IMAGE", raising=False)
    assert idx.image_info()[0], what
    plan = idx.plan_info(len(Q), k)
    assert IMAGE_KERNEL in plan, (what, plan)
    got = idx.search(Q, k)
    mp.setenv("AMDR_DENSE_HI_IMAGE", "0")
    plan0 = idx.plan_info(len(Q), k)
    assert IMAGE_KERNEL not in plan0 and plan0.startswith(PLAIN_KERNEL + " fp16 first pass"), (what, plan0)
    plain = idx.search(Q, k)
    mp.delenv("AMDR_DENSE_HI_IMAGE")
    same(got, plain, what)
    return got


def other_forms(nat, mp, X, Q, k):
    out = {}
    for name, h, tl in (("exact", "0", "1"), ("full", "0", "0")):
        mp.setenv("AMDR_DENSE_HI", h)
        mp.setenv("AMDR_DENSE_TWO_LEVEL", tl)
        idx = nat.DenseIndex(X)
        assert "dense_hi" not in idx.plan_info(len(Q), k)
        out[name] = idx.search(Q, k)
        idx.close()
    mp.setenv("AMDR_DENSE_HI", "1")
    mp.setenv("AMDR_DENSE_TWO_LEVEL", "1")
    return out


# ---- 1 ----------------------------------------------------------------------------------------------------------------
CASES = [(9017, 128, 64, 10), (9024, 256, 5, 1), (7777, 384, 33, 10), (9017, 768, 70, 10), (8200, 1024, 130, 5),
         (12017, 512, 64, 80)]


@pytest.mark.parametrize("n, d, nq, k", CASES, ids=[f"{n}x{d}-q{nq}-k{k}" for n, d, nq, k in CASES])
def test_image_form_same_ids_and_score_bits(nat, hi, n, d, nq, k):
    """A ragged and a full last tile; one, two and three query tiles; the 48-query tile of d = 1 024; k to 80."""
    from oracle import dense as OD
    rng = np.random.default_rng(n + d)
    X, Q = unit_rows(rng, n, d), unit_rows(rng, nq, d)
    idx = nat.DenseIndex(X)
    assert PLAIN_KERNEL in idx.plan_info(nq, k) and IMAGE_KERNEL not in idx.plan_info(nq, k)
    assert idx.image_info() == (False, 0, 0, 0)
    idx.build_image()
    assert idx.image_info() == (True, image_bytes(n, d), n, scale_exp(X))
    got = with_and_without(idx, Q, k, hi, (n, d, nq, k))
    assert idx.hi_counters()[0] == 2 * nq
    idx.close()
    for name, ref in other_forms(nat, hi, X, Q, k).items():
        same(got, ref, (n, d, nq, k, name))
    _, ei = OD.flatip_topk(X, Q, k)
    assert np.array_equal(got[1], ei)


# ---- 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies, rows, nq", [(40, 300, 70), (150, 100, 64)], ids=["40-fold", "150-fold"])
def test_first_pass_is_the_same_first_pass(nat, hi, copies, rows, nq):
    """Rows repeated 40- and 150-fold: the bound cannot separate the cut, what the first pass hands on decides which
    queries raise the flag.  Bit-equal maxima show as EQUAL counters (queries taken, unresolved, level, in use, passes,
    flagged passes) on two fresh handles, one with the image; results equal the exact form."""
    rng = np.random.default_rng(77 + copies)
    base = unit_rows(rng, rows, 256)
    X = np.concatenate([base] * copies, axis=0)
    Q = unit_rows(rng, nq, 256)
    res, counters = {}, {}
    for form in ("image", "plain"):
        idx = nat.DenseIndex(X)
        if form == "image":
            idx.build_image()
        assert (IMAGE_KERNEL in idx.plan_info(nq, 10)) == (form == "image")
        res[form] = idx.search(Q, 10)
        counters[form] = idx.hi_counters()
        idx.close()
    assert counters["image"] == counters["plain"], counters
    assert counters["image"][0] == nq and counters["image"][1] > 0 and counters["image"][5] > 0  # the flag did go up
    same(res["image"], res["plain"], "plain")
    same(res["image"], other_forms(nat, hi, X, Q, 10)["exact"], "exact")
    top = np.argmax(base.astype(np.float64) @ Q.astype(np.float64).T, axis=0)
    assert np.array_equal(res["image"][1], top[:, None] + rows * np.arange(10)[None, :])


# ---- 3 ----------------------------------------------------------------------------------------------------------------
def test_image_scales_subnormals_and_non_finite_values(nat, hi):
    rng = np.random.default_rng(8)
    n, d, nq = 9017, 256, 40
    base, Qb = unit_rows(rng, n, d), unit_rows(rng, nq, d)
    for xe, qe in ((-20, 30), (10, -30), (-20, -30), (10, 30)):
        X = np.ldexp(base, xe).astype(np.float32)
        Q = np.ldexp(Qb, qe).astype(np.float32)
        Q[3] *= np.float32(1e-6)
        idx = nat.DenseIndex(X)
        idx.build_image()
        assert idx.image_info() == (True, image_bytes(n, d), n, scale_exp(X)), xe
        got = with_and_without(idx, Q, 10, hi, (xe, qe))
        idx.close()
        same(got, other_forms(nat, hi, X, Q, 10)["exact"], (xe, qe, "exact"))
    # components in fp16's subnormal range after the matrix scale (and below it: they round to zero), whole rows and
    # single components; one large row sets the scale
    X = base.copy()
    X[::3] *= np.ldexp(np.float32(1), -rng.integers(12, 26, size=(len(X[::3]), 1))).astype(np.float32)
    X[1::5, ::2] *= np.float32(2.0 ** -17)
    X[11] *= np.float32(7.0)
    idx = nat.DenseIndex(X)
    idx.build_image()
    got = with_and_without(idx, Qb, 10, hi, "subnormal halves")
    idx.close()
    same(got, other_forms(nat, hi, X, Qb, 10)["exact"], "subnormal halves, exact")
    # NaN rows: dropped from the statistics, which stay finite -> an image; their halves are NaN in both forms
    X = base.copy()
    X[::7] = np.nan
    X[5, 9] = np.nan
    Q = Qb.copy()
    Q[5, 3] = np.nan
    Q[6, 0] = np.inf
    idx = nat.DenseIndex(X)
    idx.build_image()
    assert idx.image_info() == (True, image_bytes(n, d), n, scale_exp(X))
    got = with_and_without(idx, Q, 10, hi, "nan rows, nan / inf queries")
    idx.close()
    same(got, other_forms(nat, hi, X, Q, 10)["exact"], "nan rows, exact")
    assert (got[1][5] == -1).all() and not (got[1][:5] % 7 == 0).any() and not np.isnan(got[0][:5]).any()
    # statistics that are not finite: an infinite component; a largest component outside 2^+-99
    for bad in ("inf", "huge", "tiny"):
        X = base.copy()
        if bad == "inf":
            X[100, 5] = np.inf
        else:
            X = np.ldexp(X, 110 if bad == "huge" else -110).astype(np.float32)
        idx = nat.DenseIndex(X)
        with pytest.raises(nat.NativeError, match="not finite"):
            idx.build_image()
        assert idx.image_info() == (False, 0, 0, 0)
        assert "dense_hi" not in idx.plan_info(nq, 10)
        a = idx.search(Qb, 10)
        hi.setenv("AMDR_DENSE_HI_IMAGE", "0")
        b = idx.search(Qb, 10)
        hi.delenv("AMDR_DENSE_HI_IMAGE")
        same(a, b, bad)
        idx.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------
def test_add_keeps_the_image_current(nat, hi):
    rng = np.random.default_rng(23)
    d, k = 256, 10
    X0 = unit_rows(rng, 9017, d)
    Q = unit_rows(rng, 70, d)
    idx = nat.DenseIndex(X0)
    idx.build_image()
    assert idx.image_info() == (True, image_bytes(9017, d), 9017, scale_exp(X0))
    X = X0

    def step(rows, what):
        nonlocal X
        idx.add(rows)
        X = np.concatenate([X, rows])
        present, nbytes, covered, e = idx.image_info()
        assert present and covered == idx.ntotal == len(X) and nbytes >= image_bytes(len(X), d), (what, nbytes, covered)
        assert e == scale_exp(X), (what, e)
        got = with_and_without(idx, Q, k, hi, what)
        hi.setenv("AMDR_DENSE_HI_IMAGE", "0")  # (a fresh index has no image anyway: the pin only says so)
        fresh = nat.DenseIndex(X)
        assert not fresh.image_info()[0]
        same(got, fresh.search(Q, k), (what, "fresh image-less index"))
        fresh.close()
        hi.delenv("AMDR_DENSE_HI_IMAGE")
        return nbytes, e

    # (a) 7 rows complete the partial tile (9 024 rows = 282 full tiles), 1 opens a tile, then 5 000.  The new rows are
    # longer than the old ones, so every query's best rows are among them: a tile the image did not take up, or whose
    # padding was left in place, changes the answer
    b1, _ = step(unit_rows(rng, 7, d) * np.float32(1.5), "add 7")
    assert b1 == image_bytes(9017, d)  # the image's last tile had room for them
    b2, _ = step(unit_rows(rng, 1, d) * np.float32(1.5), "add 1")
    assert b2 == image_bytes(2 * 9017, d)  # no room: a new image, sized like the matrix's new allocation (capacity 2 n)
    b3, _ = step(unit_rows(rng, 5000, d) * np.float32(1.5), "add 5000")
    assert b3 == b2  # room was there
    # (b) an add that forces the matrix to be reallocated: 14 025 + 5 000 rows > the capacity of 18 034
    b4, e4 = step(unit_rows(rng, 5000, d) * np.float32(1.5), "add past the capacity")
    assert b4 == image_bytes(2 * 18034, d)
    # (c) a component 8 x the previous maximum: the scale exponent moves by 3, every half of the image changes
    big = unit_rows(rng, 40, d)
    big[7, 3] = np.float32(8.0) * np.abs(X).max()
    _, e5 = step(big, "add rows that change the scale")
    assert e5 == e4 + 3
    # an add that leaves the statistics non-finite takes the first pass away, and the image with it
    bad = unit_rows(rng, 3, d)
    bad[1, 1] = np.inf
    idx.add(bad)
    assert idx.image_info() == (False, 0, 0, 0) and "dense_hi" not in idx.plan_info(70, k)
    idx.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------
def test_drop_pin_idempotence_and_unsupported_width(nat, hi):
    rng = np.random.default_rng(5)
    X, Q = unit_rows(rng, 9017, 384), unit_rows(rng, 33, 384)
    idx = nat.DenseIndex(X)
    before = idx.plan_info(33, 10)
    ref = idx.search(Q, 10)
    idx.build_image()
    info = idx.image_info()
    g0 = nat.workspace_growths()
    idx.build_image()  # a no-op: nothing allocated, nothing changed
    assert idx.image_info() == info == (True, image_bytes(9017, 384), 9017, scale_exp(X)) and nat.workspace_growths() == g0
    same(with_and_without(idx, Q, 10, hi, "pin"), ref, "pin")
    hi.setenv("AMDR_DENSE_HI_IMAGE", "0")
    assert idx.plan_info(33, 10) == before
    hi.setenv("AMDR_DENSE_HI_IMAGE", "1")
    assert IMAGE_KERNEL in idx.plan_info(33, 10)
    hi.delenv("AMDR_DENSE_HI_IMAGE")
    idx.drop_image()
    assert idx.image_info() == (False, 0, 0, 0) and idx.plan_info(33, 10) == before
    same(idx.search(Q, 10), ref, "dropped")
    idx.drop_image()  # nothing to drop
    idx.build_image()
    same(with_and_without(idx, Q, 10, hi, "built again"), ref, "built again")
    idx.close()
    # a width the fp16 first pass does not support
    X2, Q2 = unit_rows(rng, 9017, 200), unit_rows(rng, 33, 200)
    idx = nat.DenseIndex(X2)
    ref = idx.search(Q2, 10)
    with pytest.raises(nat.NativeError, match="d=200"):
        idx.build_image()
    assert idx.image_info() == (False, 0, 0, 0)
    same(idx.search(Q2, 10), ref, "d = 200")
    idx.close()
    # a handle over caller-owned device memory may have one too
    import torch
    Xd = torch.from_numpy(X).cuda()
    idx = nat.DenseIndex(device_ptr=Xd.data_ptr(), n=9017, dim=384, keepalive=Xd)
    idx.build_image()
    assert idx.image_info() == info
    same(with_and_without(idx, Q, 10, hi, "wrapped matrix"), nat.DenseIndex(X).search(Q, 10), "wrapped matrix")
    idx.close()


# ---- 6: reserve and capture (helpers as in test_reserve_capture_gpu.py) -----------------------------------------------------
TOL = 1e-4


def _stream() -> int:
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


def nq_grid(nq_max, lo=1, hi=None):
    hi = nq_max if hi is None else min(hi, nq_max)
    return sorted({q for q in (1, 4, 5, 8, 9, nq_max - 1, nq_max) if lo <= q <= hi})


def k_grid(k_max, hi=None):
    hi = k_max if hi is None else min(hi, k_max)
    return sorted({k for k in (1, 9, 10, 16, 17, k_max - 1, k_max) if 1 <= k <= hi})


def enqueue(nat, fn, what):
    """Run fn() (enqueues "_device" work) and assert that no workspace grew — before any synchronisation."""
    g0 = nat.workspace_growths()
    fn()
    grew = nat.workspace_growths() - g0
    assert grew == 0, f"{what}: a call within the reserve (re)allocated {grew} workspace buffer(s)"


def capture(nat, fn, what):
    """Record fn() on a non-blocking side stream; the growth check runs on the host before the graph exists."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    g0 = nat.workspace_growths()
    with torch.cuda.graph(g, stream=side):
        fn()
    grew = nat.workspace_growths() - g0
    assert grew == 0, f"{what}: the captured call (re)allocated {grew} workspace buffer(s); the graph is not replayed"
    return g


def check_topk(S64, s, i, k, gap=TOL):
    """ids / scores of a top-k against exact fp64 scores S64 [nq, n]: valid distinct ids, each score within TOL of the
    exact score of its id, sorted, the oracle's clear hits present, the oracle's order wherever neighbours are
    separated."""
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
    full = np.take_along_axis(S64, np.argsort(-S64, axis=1, kind="stable")[:, :kk + 1], 1)
    gaps_ok = np.abs(np.diff(full, axis=1)) > gap
    ones = np.ones((nq, 1), dtype=bool)
    right = gaps_ok[:, :kk] if kk < n else np.concatenate([gaps_ok, ones], 1)
    sep = np.concatenate([ones, gaps_ok[:, :kk - 1]], 1) & right
    assert np.all((got == order)[sep])
    for b in np.nonzero(np.any(got != order, axis=1))[0]:
        clear = es[b] > kth[b, 0] + TOL
        assert set(order[b][clear].tolist()) <= set(got[b].tolist()), b


def test_image_reserve_then_capture(nat, hi):
    """build_image, reserve, then "_device" calls over the (nq, k) grid: no workspace grows (read before any
    synchronise: the image is not workspace and no search builds it), results equal the oracle; one call captured on a
    side stream and replayed twice on new queries equals an eager call bit for bit."""
    import torch
    from oracle import dense as OD
    dev = torch.device("cuda", 0)
    n, d, nq_max, k_max = 20_000, 128, 100, 64
    rng = np.random.default_rng(20_000)
    X = unit_rows(rng, n, d)
    X64 = X.astype(np.float64)
    idx = nat.DenseIndex(X)
    idx.build_image()
    idx.reserve(nq_max, k_max)
    assert idx.image_info() == (True, image_bytes(n, d), n, scale_exp(X))
    Qall = unit_rows(rng, nq_max, d)
    S_all = Qall.astype(np.float64) @ X64.T
    Qd = torch.from_numpy(Qall).to(dev)
    seen = set()
    for nq in nq_grid(nq_max):
        for k in k_grid(k_max):
            plan = idx.plan_info(nq, k)
            want = "dense_scan_topk_kernel" if nq <= 4 else IMAGE_KERNEL
            assert want in plan, (nq, k, plan)
            seen.add(want)
            s = torch.empty((nq, k), dtype=torch.float32, device=dev)
            i = torch.empty((nq, k), dtype=torch.int64, device=dev)
            enqueue(nat, lambda: idx.search_device(Qd.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), _stream()),
                    f"nq={nq} k={k}")
            torch.cuda.synchronize()
            check_topk(S_all[:nq], s.cpu().numpy(), i.cpu().numpy(), k)
            if k == 10:
                assert np.array_equal(i.cpu().numpy(), OD.flatip_topk(X, Qall[:nq], k)[1])
    assert seen == {"dense_scan_topk_kernel", IMAGE_KERNEL}
    nq, k = nq_max, 10
    Q = torch.empty((nq, d), dtype=torch.float32, device=dev)
    s = torch.empty((nq, k), dtype=torch.float32, device=dev)
    i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    g = capture(nat, lambda: idx.search_device(Q.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), _stream()), "capture")
    for seed in (1, 2):
        q = unit_rows(np.random.default_rng(seed * 1000 + nq + k), nq, d)
        Q.copy_(torch.from_numpy(q))
        g.replay()
        torch.cuda.synchronize()
        gs, gi = s.cpu().numpy(), i.cpu().numpy()
        es_, ei_ = torch.empty_like(s), torch.empty_like(i)
        enqueue(nat, lambda: idx.search_device(Q.data_ptr(), nq, k, es_.data_ptr(), ei_.data_ptr(), _stream()), "eager")
        torch.cuda.synchronize()
        assert np.array_equal(gi, ei_.cpu().numpy()) and np.array_equal(gs.view(np.uint32), es_.cpu().numpy().view(np.uint32))
        check_topk(q.astype(np.float64) @ X64.T, gs, gi, k)
        assert np.array_equal(gi, OD.flatip_topk(X, q, k)[1])
    idx.close()


# ---- 7 ----------------------------------------------------------------------------------------------------------------
def test_staging_buffer_hooks_with_the_image(nat, hi):
    """A 64-entry staging buffer flushes after every emitting tile; a list too short for the candidates raises the flag
    and the exact chain takes over: same results as the exact form, same counters as without the image."""
    rng = np.random.default_rng(41)
    X, Q = unit_rows(rng, 20011, 256), unit_rows(rng, 64, 256)
    exact = other_forms(nat, hi, X, Q, 10)["exact"]
    for env, val, want in (("AMDR_DENSE_HI_WBUF", "64", (64, 0, 1, 0)), ("AMDR_DENSE_HI_CAP", "500", (64, 64, 1, 1))):
        hi.setenv(env, val)
        for form in ("image", "plain"):
            idx = nat.DenseIndex(X)
            if form == "image":
                idx.build_image()
            assert (IMAGE_KERNEL in idx.plan_info(64, 10)) == (form == "image")
            same(idx.search(Q, 10), exact, (env, form))
            c = idx.hi_counters()
            assert (c[0], c[1], c[4], c[5]) == want, (env, form, c)
            idx.close()
        hi.delenv(env)


# ---- 8 ----------------------------------------------------------------------------------------------------------------
def test_vector_store_and_retriever_with_the_image(nat, tmp_path, caplog):
    from conftest import GOLDEN
    from legal_rag_amd.config import AppConfig
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.builders.incremental_dense_builder import IncrementalDenseBuilder
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from legal_rag_amd.retrieval.vector_store import FlatIPIndex, VectorStore
    cfg = AppConfig.for_data_dir(str(tmp_path), "en")
    cfg.retrieval.encoder_backend = "hashing"
    cfg.retrieval.enable_colbert = False
    cfg.retrieval.enable_rerank = False
    chunks = load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")
    base, extra = chunks[:200], chunks[200:230]
    build_faiss_index(cfg, base)
    build_bm25_index(cfg, base)
    cfg16 = copy.deepcopy(cfg)
    cfg16.retrieval.dense_image = "fp16"
    plain, imaged = HybridRetriever(cfg), HybridRetriever(cfg16)
    questions = ["what warranty does a merchant give that goods are merchantable", "Short Titles",
                 "statute of frauds signed writing sale of goods price of $500", "What is § 2-314?",
                 "risk of loss passes to the buyer on tender of delivery"]
    for q in questions:
        a, b = plain.search(q, top_k=10), imaged.search(q, top_k=10)
        assert len(a) == len(b) > 0
        assert [(h.chunk.id, h.score, h.score_breakdown) for h in a] == [(h.chunk.id, h.score, h.score_breakdown) for h in b]
    vs, vs0 = VectorStore.from_config(cfg16), VectorStore.from_config(cfg)
    assert vs is not vs0
    d = vs.index.d
    assert vs.index.image_info() == (True, image_bytes(200, d), 200, vs.index.image_info()[3])
    assert vs0.index.image_info() == (False, 0, 0, 0)
    # an incremental add through the builder keeps the image current
    inc = tmp_path / "incoming.jsonl"
    inc.write_text("".join(json.dumps(c.model_dump(), ensure_ascii=False) + "\n" for c in extra), encoding="utf-8")
    assert IncrementalDenseBuilder(cfg16).add_jsonl(inc) == 30
    present, _, rows, _ = vs.index.image_info()
    assert present and rows == vs.index.ntotal == 230
    # an unknown mode raises; a width the pass does not support logs and serves without the image
    with pytest.raises(ValueError):
        FlatIPIndex(np.zeros((4, 128), dtype=np.float32), dense_image="fp8")
    with caplog.at_level("WARNING"):
        odd = FlatIPIndex(unit_rows(np.random.default_rng(1), 50, 200), dense_image="fp16")
    assert any("d=200" in r.getMessage() for r in caplog.records)
    assert odd.image_info() == (False, 0, 0, 0) and odd.search(np.ones((1, 200), dtype=np.float32), 3)[1].shape == (1, 3)

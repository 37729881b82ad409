"""Batches past 65 535 queries in every channel (include/amdretrieval.h: every batched call serves any nq an int32 holds).

A grid's y is sure to hold 65 535 blocks (the MI355X reports a maximum of 65 536), so a launch that carries the batch there
goes in pieces (csrc/common.hpp grid_y_pieces): the BM25 scoring kernel, the dense slab top-k, the dense scan, the MaxSim
pair forms and the scoped channels.  The others carry it in x.  Every case here runs at nq = 65 535 (one piece), 65 536 and
65 541 (odd, no multiple of 4, 8 or 32: the pair and packed kernels end on a partial wave) on a corpus small enough that
the batch is the only large thing.  What the cases pin is the RESULT of every row: the offsets of the later pieces, the
slab lists they share and the merge behind them.  (The ROCm runtime of the MI355X also accepts the unsplit launches at
these sizes, so the cases do not depend on a launch being refused.)

The batch is P = 257 distinct queries repeated in order — query q is distinct query q mod 257, a prime, so the period lines
up with no wave, tile or piece boundary — and the expected result of all of it is ONE oracle call on the 257.  Every row of
the big batch is compared, bit for bit: BM25 in fp64 against oracle/bm25.py, dense on integer data whose fp32 dot products
are exact (tests/dense_adversary.py), MaxSim on an exactly representable store (tests/maxsim_adversary.py), fusion against
oracle/fusion.py (tests/fusion_adversary.py).  The rows either side of the first piece boundary (65 534 ... 65 537) and the
last row are named in the assertion messages: a wrong offset in a later piece shows only there.

Each "_device" case runs behind a reserve sized for the batch and amdr_workspace_growths must not move: the pieces of one
call share the reserved workspace.  Each case asserts the form its plan_info reports, so a routing change cannot silently
empty it."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import dense_adversary as DA
import fusion_adversary as FA
import maxsim_adversary as MA

pytestmark = pytest.mark.gpu

P = 257
NQS = (65535, 65536, 65541)
GUARD = 64  # sentinel rows behind every device output
FLT_MAX = float(np.finfo(np.float32).max)
DBL_MAX = float(np.finfo(np.float64).max)
SENT = {np.dtype(np.float32): -123.25, np.dtype(np.float64): -123.25, np.dtype(np.int64): -777, np.dtype(np.int32): -777}


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


def dev():
    import torch
    return torch.device("cuda", 0)


def stream():
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(dev())  # (a copy: the cached inputs are read-only arrays)


def period(nq):
    return np.arange(nq) % P


def tiled_dev(a, nq):
    """Rows q mod 257 of a [257, ...] host array, on the device."""
    return to_dev(a)[to_dev(period(nq))].contiguous()


def named_rows(nq):
    return [r for r in (65534, 65535, 65536, 65537, nq - 1) if 0 <= r < nq]


def bits(a):
    """Bit patterns, the two zeros counted as equal."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = a + a.dtype.type(0.0)
        return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
    return a


def assert_tiled(got, exp, what, index=None):
    """got[q] == exp[index[q]] (index: q mod 257) for EVERY row q of the batch, by bit pattern."""
    got, exp = np.asarray(got), np.asarray(exp)
    nq = got.shape[0]
    index = period(nq) if index is None else index
    assert got.dtype == exp.dtype and got.shape[1:] == exp.shape[1:], (what, got.dtype, got.shape, exp.dtype, exp.shape)
    g, e = bits(got).reshape(nq, -1), bits(exp).reshape(exp.shape[0], -1)
    ok = np.empty(nq, dtype=bool)
    for lo in range(0, nq, 8192):
        hi = min(nq, lo + 8192)
        ok[lo:hi] = (g[lo:hi] == e[index[lo:hi]]).all(axis=1)
    for r in named_rows(nq):
        assert ok[r], f"{what}: row {r} of {nq} (distinct query {index[r]}) differs: got {got[r]}, expected {exp[index[r]]}"
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, f"{what}: {bad.size} of {nq} rows differ, the first at {bad[:8].tolist()}"


class Out:
    """A device output of `rows` rows with GUARD sentinel rows behind it."""

    def __init__(self, rows, shape, dtype):
        import torch
        self.rows, self.dtype = rows, np.dtype(dtype)
        self.t = torch.full((rows + GUARD,) + tuple(shape), SENT[self.dtype], dtype=getattr(torch, self.dtype.name), device=dev())

    def ptr(self):
        return self.t.data_ptr()

    def host(self, what):
        a = self.t.cpu().numpy()
        assert (a[self.rows:] == SENT[self.dtype]).all(), (what, "wrote past the end of an output")
        return a[:self.rows]


def reserved(nat, call, what):
    """call() enqueues "_device" work behind a reserve sized for it: no workspace of the library grows."""
    import torch
    g0 = nat.workspace_growths()
    call()
    grew = nat.workspace_growths() - g0  # read on the host before anything is synchronised
    torch.cuda.synchronize()
    assert grew == 0, (what, "a reserved call grew a workspace", grew)


def set_pins(monkeypatch, names, pins):
    for name in names:
        monkeypatch.delenv(name, raising=False)
    for name, v in pins.items():
        monkeypatch.setenv(name, v)


# ---- dense --------------------------------------------------------------------------------------------------------------
PAIR, SLAB = "scores_pair_topk_kernel", "scores_slab_topk_kernel"
DENSE_PINS = DA.PIN_NAMES + ("AMDR_TOPK_PAIR",)
# (name, n, d, k, pins, the form of the scores and the top-k kernel plan_info must name).  d = 64 is outside the fp16
# two-pass form (d % 128 != 0), so the default route there IS the exact pair form; the sixth case is the default route of a
# shape the two-pass form takes (both of its launches carry the batch in x).
DENSE_CASES = (
    ("default", 40, 64, 10, {}, DA.PANEL, PAIR),
    ("exact-pair", 40, 64, 10, {"AMDR_DENSE_SMALL_HI": "0"}, DA.PANEL, PAIR),
    ("slab-k40", 40, 64, 40, {}, DA.PANEL, SLAB),
    ("slab-pair-off", 40, 64, 10, {"AMDR_TOPK_PAIR": "0"}, DA.PANEL, SLAB),
    ("slab-1500-rows", 1500, 64, 40, {}, DA.PANEL, SLAB),
    ("two-pass-d128", 40, 128, 10, {}, DA.SMALL, "dense_hi_select_fuse_kernel"),
)


@functools.lru_cache(maxsize=None)
def dense_data(n, d, k):
    """Integer rows and 257 integer queries inside the 2^24 budget (components of 12-13 bits at the edge columns, which
    fp16 cannot hold): every fp32 dot product is exact in any order -> (X, Q, scores [257, k], ids [257, k])."""
    X, Q = DA.wide_X(n, d), DA.wide_Q(d, P)
    _, es, ei = DA.integer_expect(X, 0, Q, 0, k)
    return FA.frozen(X, Q, es, ei)


def dense_check(nat, idx, Q, es, ei, nq, k, what):
    s, i = idx.search(Q[period(nq)], k)
    assert_tiled(i, ei, (what, "amdr_dense_search ids"))
    assert_tiled(s, es, (what, "amdr_dense_search scores"))
    Qd = tiled_dev(Q, nq)
    os_, oi = Out(nq, (k,), np.float32), Out(nq, (k,), np.int64)
    idx.reserve(nq, k)
    reserved(nat, lambda: idx.search_device(Qd.data_ptr(), nq, k, os_.ptr(), oi.ptr(), stream()), what)
    assert_tiled(oi.host(what), ei, (what, "amdr_dense_search_device ids"))
    assert_tiled(os_.host(what), es, (what, "amdr_dense_search_device scores"))


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("case", DENSE_CASES, ids=[c[0] for c in DENSE_CASES])
def test_dense(nat, monkeypatch, case, nq):
    name, n, d, k, pins, form, topk_kernel = case
    set_pins(monkeypatch, DENSE_PINS, pins)
    X, Q, es, ei = dense_data(n, d, k)
    idx = nat.DenseIndex(X)
    plan = idx.plan_info(nq, k)
    assert DA.form_of(n, d, nq, k, pins) == form and DA.form_from_plan(plan) == form, plan
    assert topk_kernel in plan and f"queries_per_launch={nq}" in plan, plan  # the whole batch is one pass
    if topk_kernel == SLAB:
        assert PAIR not in plan and "merge_parts_kernel" not in plan, plan
    dense_check(nat, idx, Q, es, ei, nq, k, (name, nq))
    idx.close()


@pytest.mark.parametrize("nq", (65541, 131073))
def test_dense_scan_groups_in_grid_y(nat, monkeypatch, nq):
    """dense_scan_topk_kernel puts ceil(queries / queries per block) query groups in the grid's y.  Dimension 4 is outside
    the MFMA forms, 16 385 rows outside the row-waves form: every batch size scans.  k = 256: two queries per block, so
    131 073 queries would be 65 537 groups.  The scan runs in passes of <= 65 535 queries (32 768 groups): one and a rest
    of 6 queries, two and a rest of 3."""
    set_pins(monkeypatch, DENSE_PINS, {})
    n, d, k = 16385, 4, 256
    rng = np.random.default_rng(65)
    X = rng.integers(-50, 51, size=(n, d)).astype(np.float32)
    Q = rng.integers(-50, 51, size=(P, d)).astype(np.float32)
    _, es, ei = DA.integer_expect(X, 0, Q, 0, k)
    idx = nat.DenseIndex(X)
    plan = idx.plan_info(nq, k)
    assert DA.form_of(n, d, nq, k, {}) == DA.SCAN and DA.form_from_plan(plan) == DA.SCAN, plan
    assert "dense_scan_topk_kernel<NQ=2> grid=1x32768" in plan, plan
    dense_check(nat, idx, Q, es, ei, nq, k, ("scan", nq))
    idx.close()


# ---- BM25 ---------------------------------------------------------------------------------------------------------------
ARGMAX, STAGED = "the register arg-max rounds", "the staged selector"
# (documents, k) -> (slabs, ranked by): bm_plan.  2 100 documents are two slabs at k = 10 and ONE slab of the staged
# selector at k = 40 (slabs of <= 4 096 there), so 4 100 documents put the staged selector through the slab lists too.
BM25_PLANS = {(40, 10): (1, ARGMAX), (40, 40): (1, ARGMAX), (2100, 10): (2, ARGMAX), (2100, 40): (1, STAGED),
              (4100, 10): (3, ARGMAX), (4100, 40): (2, STAGED)}


@functools.lru_cache(maxsize=None)
def bm25_corpus(n_docs):
    from oracle import bm25 as OB
    rng = np.random.default_rng(2500 + n_docs)
    words = [f"w{j}" for j in range(60 if n_docs <= 40 else 300)]
    docs = [[words[j] for j in rng.integers(0, len(words), size=int(rng.integers(3, 30)))] for _ in range(n_docs)]
    ob = OB.BM25Okapi(docs)
    csr = OB.to_csr(ob)
    queries = [[words[j] for j in rng.integers(0, len(words), size=int(rng.integers(1, 9)))] for _ in range(P)]
    queries[0] = []                                         # empty: +0.0 everywhere, the lowest ids
    queries[1] = ["zz1", "zz2"]                             # unknown terms only
    queries[2] = ["w3", "w3", "w5", "w3"]                   # repeats count
    queries[3] = [words[j] for j in rng.integers(0, len(words), size=40)]  # longer than 32 tokens
    queries[4] = ["zz1", "w7", "zz2", "w7"]                 # unknown terms between known ones
    tids = [np.asarray([csr["vocab"].get(t, -1) for t in q], dtype=np.int32) for q in queries]
    return ob, csr, queries, tids


@functools.lru_cache(maxsize=None)
def bm25_expected(n_docs, k):
    from oracle import bm25 as OB
    ob, _, queries, _ = bm25_corpus(n_docs)
    es, ei = np.full((P, k), -DBL_MAX), np.full((P, k), -1, dtype=np.int64)
    for q, toks in enumerate(queries):
        hits = OB.search(ob, toks, k)
        ei[q, :len(hits)] = [h[0] for h in hits]
        es[q, :len(hits)] = [h[1] for h in hits]
    assert (ei >= 0).all()  # k <= documents: no padding in these cases
    return FA.frozen(es, ei)


@functools.lru_cache(maxsize=4)
def bm25_batch(n_docs, nq):
    """(q_terms i32, q_ptr i64) of the tiled batch, as amdr_bm25_search takes them."""
    tids = bm25_corpus(n_docs)[3]
    lens = np.asarray([len(t) for t in tids], dtype=np.int64)[period(nq)]
    q_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    reps, rest = divmod(nq, P)
    one = np.concatenate(tids)
    q_terms = np.concatenate([np.tile(one, reps), np.concatenate(tids[:rest]) if rest else np.zeros(0, np.int32)]).astype(np.int32)
    assert q_terms.size == q_ptr[-1]
    return FA.frozen(q_terms, q_ptr)


def bm25_index(nat, n_docs):
    ob, csr, _, _ = bm25_corpus(n_docs)
    return nat.BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"], csr["doc_len"], ob.avgdl, ob.k1, ob.b)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("n_docs", (40, 2100, 4100))
def test_bm25(nat, monkeypatch, n_docs, nq):
    bm = bm25_index(nat, n_docs)
    q_terms, q_ptr = bm25_batch(n_docs, nq)
    qt_d, qp_d = to_dev(q_terms), to_dev(q_ptr)
    lib = nat.load()
    for k in (10, 40):
        slabs, ranker = BM25_PLANS[(n_docs, k)]
        plan = bm.plan_info(nq, k)
        assert f"slabs={slabs} " in plan and ranker in plan, plan
        assert ("(one slab: direct)" if slabs == 1 else "+ merge_parts_kernel") in plan, plan
        es, ei = bm25_expected(n_docs, k)
        for select in ("1", "0"):
            monkeypatch.setenv("AMDR_BM25_SELECT", select)
            what = (n_docs, nq, k, "select=" + select)
            s, i = np.empty((nq, k), dtype=np.float64), np.empty((nq, k), dtype=np.int64)
            nat._check(lib.amdr_bm25_search(bm._h, _p(q_terms, C.c_int32), _p(q_ptr, C.c_int64), C.c_int32(nq), C.c_int32(k),
                                            _p(s, C.c_double), _p(i, C.c_int64)), "amdr_bm25_search")
            assert_tiled(i, ei, (what, "amdr_bm25_search ids"))
            assert_tiled(s, es, (what, "amdr_bm25_search scores"))
            os_, oi = Out(nq, (k,), np.float64), Out(nq, (k,), np.int64)
            bm.reserve(nq, k, int(q_ptr[-1]))
            reserved(nat, lambda: bm.search_device(qt_d.data_ptr(), qp_d.data_ptr(), nq, k, os_.ptr(), oi.ptr(), stream()), what)
            assert_tiled(oi.host(what), ei, (what, "amdr_bm25_search_device ids"))
            assert_tiled(os_.host(what), es, (what, "amdr_bm25_search_device scores"))
    bm.close()


@pytest.mark.parametrize("nq", NQS)
def test_bm25_scores(nat, nq):
    """amdr_bm25_scores: the full [nq, 40] fp64 matrix (21 MB), every row against BM25Okapi.get_scores."""
    ob, _, queries, _ = bm25_corpus(40)
    bm = bm25_index(nat, 40)
    q_terms, q_ptr = bm25_batch(40, nq)
    out = np.full((nq + GUARD, 40), SENT[np.dtype(np.float64)])
    nat._check(nat.load().amdr_bm25_scores(bm._h, _p(q_terms, C.c_int32), _p(q_ptr, C.c_int64), C.c_int32(nq), _p(out, C.c_double)),
               "amdr_bm25_scores")
    assert (out[nq:] == SENT[np.dtype(np.float64)]).all()
    assert_tiled(out[:nq], np.stack([ob.get_scores(q) for q in queries]), (nq, "amdr_bm25_scores"))
    bm.close()


# ---- MaxSim -------------------------------------------------------------------------------------------------------------
MS_DOCS, MS_QLEN = 24, 2
MS_LENS = (1, 40, 2, 17, 16, 15, 31, 32, 33, 3, 39, 8, 24, 5, 12, 20, 28, 36, 7, 9, 11, 13, 30, 4)
# (name, k, pins, form).  The pair forms (one wave per (query, document)) carry the batch in the grid's y, but the route
# gives them a batch only when nq < 8 — or, on the fp32-input form, on a store of more than 8 x 65 535 documents — so they
# need no large case here; their launch goes in pieces all the same (ms_run).
MS_CASES = (("two-pass", 5, MA.P_DEF, MA.TWOPASS), ("ring", 10, MA.P_DEF, MA.RING), ("blocked-f32", 10, MA.P_F32, MA.BLOCKED))


@functools.lru_cache(maxsize=None)
def maxsim_data():
    """24 documents of 1 ... 40 tokens and 257 queries of two tokens, integers in [-15, 15]: exact in the split-fp16 and
    the fp32-input forms (maxsim_adversary certifies both) -> (D, doc_ptr, Q, scores of the split forms, of the fp32 forms)."""
    assert len(MS_LENS) == MS_DOCS and min(MS_LENS) == 1 and max(MS_LENS) == 40
    rng = np.random.default_rng(2400)
    doc_ptr = np.concatenate([[0], np.cumsum(MS_LENS)]).astype(np.int64)
    D = rng.integers(-15, 16, size=(int(doc_ptr[-1]), MA.DIM)).astype(np.float32)
    D[0, 3] = 15.0  # the store's scale
    Q = rng.integers(-15, 16, size=(P, MS_QLEN, MA.DIM)).astype(np.float32)
    Q[:, 0, 5] = np.where(np.arange(P) % 2 == 0, 15.0, -15.0)  # the scale of every query
    return FA.frozen(D, doc_ptr, Q, MA.split_expected(D, doc_ptr, Q), MA.f32_expected(D, doc_ptr, Q))


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("case", MS_CASES, ids=[c[0] for c in MS_CASES])
def test_maxsim(nat, monkeypatch, case, nq):
    name, k, pins, form = case
    set_pins(monkeypatch, MA.PIN_NAMES, pins)
    D, doc_ptr, Q, S_split, S_f32 = maxsim_data()
    assert MA.form_of(MS_DOCS, nq, k, True, pins) == form
    ms = nat.MaxSimIndex(D, doc_ptr)
    assert MA.form_from_plan(ms.plan_info(nq)) == MA.form_of(MS_DOCS, nq, 1, True, pins), ms.plan_info(nq)  # (the plan has no k)
    es, ei = MA.topk_expected(S_f32 if form == MA.BLOCKED else S_split, k)
    what = (name, nq)
    s, i = ms.search(Q[period(nq)], k)
    assert_tiled(i, ei, (what, "amdr_maxsim_search ids"))
    assert_tiled(s, es, (what, "amdr_maxsim_search scores"))
    Qd = tiled_dev(Q, nq)
    os_, oi = Out(nq, (k,), np.float32), Out(nq, (k,), np.int64)
    ms.reserve(nq, k)
    reserved(nat, lambda: ms.search_device(Qd.data_ptr(), nq, MS_QLEN, k, os_.ptr(), oi.ptr(), stream()), what)
    assert_tiled(oi.host(what), ei, (what, "amdr_maxsim_search_device ids"))
    assert_tiled(os_.host(what), es, (what, "amdr_maxsim_search_device scores"))
    ms.close()


@pytest.mark.parametrize("nq", NQS)
def test_maxsim_scores(nat, monkeypatch, nq):
    set_pins(monkeypatch, MA.PIN_NAMES, {})
    D, doc_ptr, Q, S_split, _ = maxsim_data()
    assert MA.form_of(MS_DOCS, nq, 1, False, {}) == MA.RING
    ms = nat.MaxSimIndex(D, doc_ptr)
    assert_tiled(ms.scores(Q[period(nq)]), S_split, (nq, "amdr_maxsim_scores"))
    ms.close()


# ---- fusion, rerank blend, compaction -------------------------------------------------------------------------------------
FUSE_SHAPES = ((5, 5, 5), (10, 10, 10), (22, 22, 21))  # max_out 15, 30, 65: the 16-lane packed, the 32-lane packed, the general form


@functools.lru_cache(maxsize=None)
def fuse_batch(shape):
    """257 queries of fusion_adversary's kinds (disjoint / overlapping ids, ragged lengths, an all -1 middle channel, an
    all -1 query) and the oracle's record of them."""
    rng = np.random.default_rng([65, *shape])
    kinds = [FA.KINDS[q % len(FA.KINDS)] for q in range(P)]
    batch = FA.Batch([FA._query(kd, shape, rng, FA._offset(q)) for q, kd in enumerate(kinds)], shape, 65, kinds)
    exp = FA.expected_arrays(batch.lists, FA.knobs(), FA.MIN_FINAL, sum(shape))
    return batch, FA.frozen(*exp)


def assert_record_tiled(got, exp, what):
    for name, g, e in zip(("ids", "vals", "mask", "count"), got, exp):
        assert_tiled(g, e, (what, name))


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("shape", FUSE_SHAPES, ids=["packed16", "packed32", "general"])
def test_fuse_device(nat, shape, nq):
    batch, exp = fuse_batch(shape)
    mo = sum(shape)
    assert FA.route(mo, 0) == {15: FA.P16, 30: FA.P32, 65: FA.LONG_REG}[mo]
    kn = FA.knobs()
    p = nat.make_fuse_params(method=kn["fusion_method"], rrf_k=kn["rrf_k"], alpha=kn["rrf_alpha"], w_dense=kn["dense_weight"],
                             w_bm25=kn["bm25_weight"], w_colbert=kn["colbert_weight"], min_final_score=FA.MIN_FINAL)
    keep, chans = [], []
    for c, k in enumerate(shape):
        ids = tiled_dev(batch.ids[c], nq)
        sc = tiled_dev(batch.scores[c].astype(np.float64 if c == 1 else np.float32), nq)
        keep += [ids, sc]
        chans.append((ids.data_ptr(), sc.data_ptr(), k, 0))
    outs = [Out(nq, (mo,), np.int64), Out(nq, (mo, FA.NVALS), np.float64), Out(nq, (mo,), np.int32), Out(nq, (), np.int32)]
    reserved(nat, lambda: nat.fuse_device(p, nq, *chans, *(o.ptr() for o in outs), stream=stream()), (shape, nq))
    assert_record_tiled([o.host((shape, nq)) for o in outs], exp, (shape, nq, "amdr_fuse_device"))


@pytest.mark.parametrize("nq", NQS)
def test_rerank_blend_device(nat, nq):
    shape, top_n, beta = (10, 10, 0), 8, 0.35
    mo = sum(shape)
    _, rec = fuse_batch(shape)
    ce = FA.ce_scores(P, top_n)
    exp = FA.expected_rerank(*rec, ce, top_n, beta)
    bufs = [Out(nq, (mo,), np.int64), Out(nq, (mo, FA.NVALS), np.float64), Out(nq, (mo,), np.int32), Out(nq, (mo, 2), np.float64)]
    for b, a in zip(bufs, rec[:3]):
        b.t[:nq] = tiled_dev(a, nq)
    count, ce_d = tiled_dev(rec[3], nq), tiled_dev(ce, nq)
    reserved(nat, lambda: nat.rerank_blend_device(nq, mo, count.data_ptr(), bufs[0].ptr(), bufs[1].ptr(), bufs[2].ptr(),
                                                  ce_d.data_ptr(), top_n, beta, bufs[3].ptr(), stream=stream()), nq)
    for name, b, e in zip(("ids", "vals", "mask", "rerank"), bufs, exp):
        g, e = b.host((nq, name)), np.asarray(e)
        if name == "rerank":  # NaN outside the re-ranked hits, whatever the payload
            assert_tiled(np.isnan(g), np.isnan(e), (nq, "amdr_rerank_blend_device", "rerank NaN"))
            g, e = np.nan_to_num(g), np.nan_to_num(e)
        assert_tiled(g, e, (nq, "amdr_rerank_blend_device", name))


@pytest.mark.parametrize("nq", NQS)
def test_fuse_compact_device(nat, nq):
    from test_hybrid_step import compact
    mo, w = FA.COMPACT_MAX_OUT, 3
    rec = FA.compact_record(P)
    exp = compact(*rec, w)
    ins = [tiled_dev(a, nq) for a in rec]
    outs = [Out(nq, (w,), np.int64), Out(nq, (w,), np.float64), Out(nq, (w,), np.int32), Out(nq, (), np.int32)]
    reserved(nat, lambda: nat.fuse_compact_device(nq, mo, w, *(t.data_ptr() for t in ins), *(o.ptr() for o in outs),
                                                  stream=stream()), nq)
    for name, o, e in zip(("rows", "scores", "mask", "count"), outs, exp):
        assert_tiled(o.host((nq, name)), np.asarray(e), (nq, "amdr_fuse_compact_device", name))


# ---- the step -----------------------------------------------------------------------------------------------------------
STEP_N, STEP_K = 40, 10
STEP_MIN_FINAL = 0.2


@functools.lru_cache(maxsize=None)
def step_expected(with_colbert):
    """The oracle pipeline on the 257 distinct queries: each channel's oracle list, then oracle/fusion.py."""
    _, _, des, dei = dense_data(STEP_N, 64, STEP_K)
    bes, bei = bm25_expected(STEP_N, STEP_K)
    lists = []
    ces = cei = None
    if with_colbert:
        ces, cei = MA.topk_expected(maxsim_data()[3], STEP_K)
    for q in range(P):
        d = [(int(i), float(s)) for s, i in zip(des[q], dei[q]) if i >= 0]
        b = [(int(i), float(s)) for s, i in zip(bes[q], bei[q]) if i >= 0]
        c = [(int(i), float(s)) for s, i in zip(ces[q], cei[q]) if i >= 0] if with_colbert else []
        lists.append((d, b, c))
    mo = STEP_K * (3 if with_colbert else 2)
    return FA.frozen(*FA.expected_arrays(lists, FA.knobs(), STEP_MIN_FINAL, mo))


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("with_colbert", (False, True), ids=["dense+bm25", "dense+bm25+colbert"])
def test_hybrid_step(nat, monkeypatch, with_colbert, nq):
    """HybridEngine.search_batch, the headline path.  dense + BM25: bm25_search_device, then amdr_dense_search_fuse_device
    (the score rows ranked and fused by one kernel); with ColBERT: the three channels, then amdr_fuse_device."""
    import torch
    from legal_rag_amd.retrieval import engine as E
    set_pins(monkeypatch, DENSE_PINS + MA.PIN_NAMES + ("AMDR_BM25_SELECT", "AMDR_ENGINE_OVERLAP"), {})
    X, Q, des, dei = dense_data(STEP_N, 64, STEP_K)
    D, doc_ptr, Qt, S_split, _ = maxsim_data()
    di, bm = nat.DenseIndex(X), bm25_index(nat, STEP_N)
    ms = nat.MaxSimIndex(D, doc_ptr) if with_colbert else None
    eng = E.HybridEngine(di, bm, ms)
    assert E.step_form(True, True, with_colbert, False, nq, STEP_K, True)[0] == (E.CHANNELS_SIDE if with_colbert else E.BM25_THEN_FUSED)
    q_terms, q_ptr = bm25_batch(STEP_N, nq)
    args = dict(q_emb=tiled_dev(Q, nq), q_terms=to_dev(q_terms), q_ptr=to_dev(q_ptr))
    if with_colbert:
        args["q_tok"] = tiled_dev(Qt, nq)
    kn = FA.knobs()
    params = nat.make_fuse_params(method=kn["fusion_method"], rrf_k=kn["rrf_k"], alpha=kn["rrf_alpha"], w_dense=kn["dense_weight"],
                                  w_bm25=kn["bm25_weight"], w_colbert=kn["colbert_weight"], min_final_score=STEP_MIN_FINAL)
    exp = step_expected(with_colbert)
    bes, bei = bm25_expected(STEP_N, STEP_K)
    what = ("dense+bm25+colbert" if with_colbert else "dense+bm25", nq)
    eng.reserve(nq, STEP_K, int(q_ptr[-1]))
    eng.search_batch(params, STEP_K, **args)  # the engine's own torch buffers are made here, outside the counted call
    torch.cuda.synchronize()
    res = []
    reserved(nat, lambda: res.append(eng.search_batch(params, STEP_K, **args)), what)
    res = res[0]
    assert_tiled(res.dense_ids.cpu().numpy(), dei, (what, "dense ids"))
    assert_tiled(res.dense_scores.cpu().numpy(), des, (what, "dense scores"))
    assert_tiled(res.bm25_ids.cpu().numpy(), bei, (what, "bm25 ids"))
    assert_tiled(res.bm25_scores.cpu().numpy(), bes, (what, "bm25 scores"))
    if with_colbert:
        ces, cei = MA.topk_expected(S_split, STEP_K)
        assert_tiled(res.colbert_ids.cpu().numpy(), cei, (what, "colbert ids"))
        assert_tiled(res.colbert_scores.cpu().numpy(), ces, (what, "colbert scores"))
    assert_record_tiled(res.to_host(), exp, (what, "fused"))
    for h in (di, bm, ms):
        if h is not None:
            h.close()


# ---- scoped -------------------------------------------------------------------------------------------------------------
SC_N, SC_K = 80, 5
SC_SIZES = (0, 1, 3, 64, 65)
SC_CYCLE = len(SC_SIZES) + 1  # qscope cycles through the five scopes and one value outside the table


@functools.lru_cache(maxsize=None)
def scoped_data():
    """80 rows in every channel (exact data), a table of 5 scopes per channel's row space, and for each (distinct query,
    qscope value) the unscoped channel's oracle scores restricted to the scope, ranked as test_scope_gpu.ranked does."""
    from oracle import bm25 as OB
    from test_scope_gpu import make_table, ranked
    rng = np.random.default_rng(6500)
    X, Q = DA.wide_X(SC_N, 64), DA.wide_Q(64, P)
    DA.assert_integer_budget(X, Q)
    words = [f"w{j}" for j in range(60)]
    docs = [[words[j] for j in rng.integers(0, 60, size=int(rng.integers(3, 30)))] for _ in range(SC_N)]
    ob = OB.BM25Okapi(docs)
    csr = OB.to_csr(ob)
    queries = bm25_corpus(40)[2]  # the same words: empty, unknown, repeated and long queries included
    tids = [np.asarray([csr["vocab"].get(t, -1) for t in q], dtype=np.int32) for q in queries]
    lens = rng.integers(1, 13, size=SC_N)
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    D = rng.integers(-15, 16, size=(int(doc_ptr[-1]), MA.DIM)).astype(np.float32)
    D[0, 3] = 15.0
    Qt = maxsim_data()[2]
    refs = (DA.exact_scores(X, Q).astype(np.float32), np.stack([ob.get_scores(q) for q in queries]), MA.split_expected(D, doc_ptr, Qt))
    pads = (np.float32(-FLT_MAX), -DBL_MAX, np.float32(-FLT_MAX))
    tables, expected = [], []
    for c in range(3):
        lists = [np.sort(rng.choice(SC_N, size=m, replace=False)) for m in SC_SIZES]
        tables.append(make_table(lists))
        es = np.empty((P * SC_CYCLE, SC_K), dtype=refs[c].dtype)
        ei = np.empty((P * SC_CYCLE, SC_K), dtype=np.int64)
        for q in range(P):
            for s in range(SC_CYCLE):
                r = lists[s] if s < len(lists) else np.zeros(0, np.int64)
                es[q * SC_CYCLE + s], ei[q * SC_CYCLE + s] = ranked(refs[c][q, r], r, SC_K, pads[c])
        expected.append((es, ei))
    return dict(X=X, Q=Q, ob=ob, csr=csr, tids=tids, D=D, doc_ptr=doc_ptr, Qt=Qt, tables=tables, expected=expected)


@functools.lru_cache(maxsize=None)
def scoped_fused_expected(with_colbert):
    sd = scoped_data()
    lists = []
    for j in range(P * SC_CYCLE):
        chans = [[(int(i), float(s)) for s, i in zip(es[j], ei[j]) if i >= 0] for es, ei in sd["expected"]]
        if not with_colbert:
            chans[2] = []
        lists.append(tuple(chans))
    return FA.frozen(*FA.expected_arrays(lists, FA.knobs(), -math.inf, SC_K * (3 if with_colbert else 2)))


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("slab", (None, "2"), ids=["default-slabs", "slab-2"])
def test_scoped(nat, monkeypatch, slab, nq):
    """The three scoped "_device" calls and amdr_hybrid_scope_device.  AMDR_SCOPE_SLAB=2 gives every scope of more than two
    rows several slabs (33 for the longest): each piece of a channel's launch goes through the slab lists and the merge,
    and the step runs as the separate calls."""
    import torch
    from legal_rag_amd.retrieval import engine as E
    set_pins(monkeypatch, MA.PIN_NAMES + ("AMDR_SCOPE_FUSED", "AMDR_BM25_SELECT"), {} if slab is None else {"AMDR_SCOPE_SLAB": slab})
    sd = scoped_data()
    ob, csr = sd["ob"], sd["csr"]
    di = nat.DenseIndex(sd["X"])
    bm = nat.BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"], csr["doc_len"], ob.avgdl, ob.k1, ob.b)
    ms = nat.MaxSimIndex(sd["D"], sd["doc_ptr"])
    eng = E.HybridEngine(di, bm, ms)
    fused, _ = nat.hybrid_scope_plan(nq, SC_K, SC_K, SC_K, max(SC_SIZES), max(SC_SIZES))
    assert fused == (slab is None)
    qscope = (np.arange(nq) % SC_CYCLE).astype(np.int32)  # 5 = outside the table: no rows
    index = period(nq) * SC_CYCLE + qscope
    tabs = [eng.upload_scopes(*sd["tables"][c], qscope, channel=c) for c in range(3)]
    lens = np.asarray([len(t) for t in sd["tids"]], dtype=np.int64)[period(nq)]
    q_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    q_terms = np.concatenate([sd["tids"][q % P] for q in range(nq)] + [np.zeros(1, np.int32)]).astype(np.int32)
    Qd, Qt, qt_d, qp_d = tiled_dev(sd["Q"], nq), tiled_dev(sd["Qt"], nq), to_dev(q_terms), to_dev(q_ptr)
    what = ("slab=" + str(slab), nq)
    eng.reserve(nq, SC_K, int(q_ptr[-1]), rows_max=max(SC_SIZES))
    calls = (("dense", lambda: eng.dense_topk_scoped(Qd, SC_K, tabs[0])),
             ("bm25", lambda: eng.bm25_topk_scoped(qt_d, qp_d, SC_K, tabs[1])),
             ("maxsim", lambda: eng.colbert_topk_scoped(Qt, SC_K, tabs[2])))
    for c, (name, call) in enumerate(calls):
        call()  # (the engine's torch buffers)
        torch.cuda.synchronize()
        got = []
        reserved(nat, lambda: got.append(call()), (what, name))
        s, i = got[0]
        assert_tiled(i.cpu().numpy(), sd["expected"][c][1], (what, name, "ids"), index)
        assert_tiled(s.cpu().numpy(), sd["expected"][c][0], (what, name, "scores"), index)
    kn = FA.knobs()
    params = nat.make_fuse_params(method=kn["fusion_method"], rrf_k=kn["rrf_k"], alpha=kn["rrf_alpha"], w_dense=kn["dense_weight"],
                                  w_bm25=kn["bm25_weight"], w_colbert=kn["colbert_weight"], min_final_score=-math.inf)
    for with_colbert in (False, True):
        args = dict(q_emb=Qd, q_terms=qt_d, q_ptr=qp_d, q_tok=Qt if with_colbert else None,
                    scopes=(tabs[0], tabs[1], tabs[2] if with_colbert else None))
        eng.search_batch(params, SC_K, **args)
        torch.cuda.synchronize()
        got = []
        reserved(nat, lambda: got.append(eng.search_batch(params, SC_K, **args)), (what, "step", with_colbert))
        res = got[0]
        assert_tiled(res.dense_ids.cpu().numpy(), sd["expected"][0][1], (what, "step dense ids"), index)
        assert_tiled(res.bm25_scores.cpu().numpy(), sd["expected"][1][0], (what, "step bm25 scores"), index)
        for name, g, e in zip(("ids", "vals", "mask", "count"), res.to_host(), scoped_fused_expected(with_colbert)):
            assert_tiled(g, e, (what, "amdr_hybrid_scope_device", with_colbert, name), index)
    for h in (di, bm, ms):
        h.close()


# ---- the device tokeniser ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tokenizers():
    from conftest import GOLDEN
    from legal_rag_amd import _native, text
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    chunks = load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")
    bm = BM25Okapi([text.tokenize_en(c.text) for c in chunks])
    vocab = list(bm.vocab().keys()) + ["What", "UCC", " ", "§", "(", ")", "C++", "AT&T", "--", "3.5%", "\r\n", "é", "　", "a", "c#", "0"]
    tok = _native.Tokenizer(vocab)
    return tok, _native.DeviceTokenizer(tok, device=0)


@pytest.mark.parametrize("nq", (65541, 131073))
def test_device_tokenizer(nat, tokenizers, nq):
    """tok_scan_kernel's carry over tiles of 256 block totals: two tiles from 65 537 queries, three at 131 073.  Texts of
    0 ... 12 bytes from the alphabet of test_tokenize_device_gpu's seeded fuzz (Han, emoji, Unicode spaces; a text cut at
    12 bytes may end inside a sequence), byte for byte against the host tokeniser."""
    from test_tokenize_device_gpu import SPACES, host_csr
    tok, dtok = tokenizers
    rng = np.random.default_rng(13)
    alphabet = (list("abcXYZ0159") + list("+#&._%-") * 2 + list(" \t\n\r") + ["\r\n", "§", "é", "(", ")", ",", "C++", "AT&T", "c#",
                "What", "3.5%", "合", "\U0001F600", "一", "鿕", "鿖", "䷿"] + SPACES)
    enc = [a.encode("utf-8") for a in alphabet]
    distinct = [b"".join(enc[j] for j in rng.integers(0, len(enc), size=int(rng.integers(0, 9))))[:12] for _ in range(P)]
    distinct[0] = b""
    assert min(len(t) for t in distinct) == 0 and max(len(t) for t in distinct) == 12
    texts = [distinct[q % P] for q in range(nq)]
    offs = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=offs[1:])
    blob = b"".join(texts)
    ht, hp, hf = host_csr(tok, blob, offs)
    assert hf.any() and not hf.all() and (ht >= 0).any() and (ht < 0).any()
    b_d, o_d = to_dev(np.frombuffer(blob, dtype=np.uint8)), to_dev(offs)
    terms, q_ptr, flags = Out(len(blob), (), np.int32), Out(nq + 1, (), np.int64), Out(nq, (), np.int32)
    dtok.reserve(nq, len(blob))
    reserved(nat, lambda: dtok.encode_device(b_d, o_d, terms.t[:len(blob)], q_ptr.t[:nq + 1], flags.t[:nq]), nq)
    dp, df, dt = q_ptr.host((nq, "q_ptr")), flags.host((nq, "flags")), terms.host((nq, "terms"))
    for r in named_rows(nq):
        assert dp[r] == hp[r] and dp[r + 1] == hp[r + 1] and df[r] == hf[r], f"query {r} of {nq}: q_ptr / flag differ"
        assert np.array_equal(dt[hp[r]:hp[r + 1]], ht[hp[r]:hp[r + 1]]), f"query {r} of {nq}: term ids differ"
    assert np.array_equal(dp, hp), np.flatnonzero(dp != hp)[:5]
    assert np.array_equal(df, hf), np.flatnonzero(df != hf)[:5]
    assert np.array_equal(dt[:int(hp[-1])], ht), np.flatnonzero(dt[:int(hp[-1])] != ht)[:5]


# ---- the rest, at 65 541 ------------------------------------------------------------------------------------------------
BIG = 65541


def merge_parts(rng, parts, k, dtype):
    """[parts, 257, k] descending lists with -1 tails of every length and scores that tie across parts."""
    s = np.sort(rng.integers(-20, 21, size=(parts, P, k)).astype(dtype) / dtype(4.0), axis=2)[:, :, ::-1].copy()
    i = np.stack([np.stack([rng.permutation(1000)[:k] + 1000 * r for _ in range(P)]) for r in range(parts)]).astype(np.int64)
    valid = rng.integers(0, k + 1, size=(parts, P))
    for r in range(parts):
        for q in range(P):  # a channel's own order: score descending, ties -> lower id
            o = np.lexsort((i[r, q], -s[r, q].astype(np.float64)))
            s[r, q], i[r, q] = s[r, q, o], i[r, q, o]
    i[np.arange(k)[None, None, :] >= valid[:, :, None]] = -1
    return s, i


@pytest.mark.parametrize("f64", (False, True), ids=["f32", "f64"])
def test_merge_topk_device(nat, f64):
    import shard_adversary as SA
    from legal_rag_amd.retrieval import sharding
    from oracle import dense as OD
    import torch
    dtype = np.float64 if f64 else np.float32
    k, k_out, nq = 10, 12, BIG
    s, i = merge_parts(np.random.default_rng(66 + f64), 3, k, dtype)
    es, ei = OD.merge_topk(list(s.astype(np.float64)), list(i), k_out)
    want, nan = SA.kernel_view(es, ei, dtype)
    assert not nan.any()
    idx = to_dev(period(nq))
    sd, idv = to_dev(s)[:, idx].contiguous(), to_dev(i)[:, idx].contiguous()
    got = []
    reserved(nat, lambda: got.append(sharding.native_merge(sd, idv, k_out)), ("merge", f64))
    torch.cuda.synchronize()
    assert_tiled(got[0][1].cpu().numpy(), ei, ("amdr_merge_topk_device ids", f64))
    assert_tiled(got[0][0].cpu().numpy(), want, ("amdr_merge_topk_device scores", f64))


def test_shard_pack_and_merge_device(nat):
    """A world of 2, a dense-like fp32 channel and a BM25-like fp64 channel through one pack per rank and one merge."""
    import shard_adversary as SA
    from legal_rag_amd.retrieval import sharding
    from oracle import dense as OD
    import torch
    nq, world, k = BIG, 2, 10
    chans = ((k, np.float32), (k, np.float64))
    offsets = (0, (1 << 33) + 5)
    rng = np.random.default_rng(67)
    lists = [merge_parts(rng, world, kc, dt) for kc, dt in chans]  # lists[c] = (scores [world, 257, k], LOCAL ids)
    idx = to_dev(period(nq))
    S = [to_dev(s)[:, idx].contiguous() for s, _ in lists]
    I = [to_dev(i)[:, idx].contiguous() for _, i in lists]
    row = nat.shard_row_words([kc for kc, _ in chans])
    gathered = Out(world * nq, (row,), np.int64)
    g = gathered.t[:world * nq].view(world, nq, row)
    for r in reversed(range(world)):
        reserved(nat, lambda: nat.shard_pack_device([(S[c][r].data_ptr(), I[c][r].data_ptr(), kc, dt == np.float64)
                                                     for c, (kc, dt) in enumerate(chans)], nq, offsets[r], g[r].data_ptr(),
                                                    stream=stream()), ("pack", r))
    gathered.host("amdr_shard_pack_device")
    for r in range(world):
        ref = sharding.pack_channels([(S[c][r], sharding.to_global(I[c][r], offsets[r])) for c in range(len(chans))])
        bad = (g[r] != ref).any(dim=1).nonzero()
        assert bad.numel() == 0, ("amdr_shard_pack_device", r, "first rows that differ", bad[:8].flatten().tolist())
    outs = [(Out(nq, (kc,), dt), Out(nq, (kc,), np.int64)) for kc, dt in chans]
    reserved(nat, lambda: nat.shard_merge_device(g.data_ptr(), world, nq, [(s.ptr(), i.ptr(), kc, dt == np.float64)
                                                                          for (s, i), (kc, dt) in zip(outs, chans)],
                                                 stream=stream()), "merge")
    for c, (kc, dt) in enumerate(chans):
        s, i = lists[c]
        gi = [np.where(i[r] >= 0, i[r] + np.int64(offsets[r]), i[r]) for r in range(world)]
        es, ei = OD.merge_topk(list(s.astype(np.float64)), gi, kc)
        want, nan = SA.kernel_view(es, ei, dt)
        assert not nan.any()
        assert_tiled(outs[c][1].host(c), ei, ("amdr_shard_merge_device ids", c))
        assert_tiled(outs[c][0].host(c), want, ("amdr_shard_merge_device scores", c))


def test_graph_search_device(nat):
    """The graph channel: 65 541 groups, each with its own query row and seeds; the 257 distinct ones against
    graph_adversary's oracle, every row of the batch against them."""
    import graph_adversary as GA
    import torch
    nq, d, ld, k, limit = BIG, 64, 4, 10, 17
    rng = np.random.default_rng(68)
    t = GA.make_tables(rng, 3000, hubs={5: 300}, row_holes=0.1)
    n_dense = t.n_rows - 7
    X, Q = GA.exact_rows(rng, n_dense, d), GA.exact_queries(rng, P, d)
    g, dense = t.index(nat), nat.DenseIndex(X)
    seeds = rng.integers(0, 60, size=(P, ld)).astype(np.int64)
    seeds[::7, 0] = -1           # dropped: outside [0, n_rows)
    seeds[::11, 1] = t.n_rows
    seed_count = rng.integers(0, ld + 1, size=P).astype(np.int32)
    p = GA.make_params(limit, default_depth=3, rel_max_depth=[3, 2, 3, 4, 1, 3])
    exp = {n: np.empty((P,) if n == "count" else (P, k), dtype=ty) for n, ty in zip(nat.GraphIndex.OUTS, nat.GraphIndex._OUT_T)}
    for q in range(P):
        found = GA.walk_oracle(t, seeds[q, :max(0, int(seed_count[q]))], p, False)
        one = GA.score_oracle(t, X, Q[q], found, p, k, n_dense)
        for n in GA.OUTS:
            exp[n][q] = one[n]
    tabs = [to_dev(p[n]) for n in ("rel_max_depth", "rel_allowed", "rel_weight", "decay")]
    gp = nat.GraphParams(p["limit"], p["default_depth"], p["lang"], 0, p["min_conf"], *(x.data_ptr() for x in tabs))
    Qd, sd, cd = tiled_dev(Q, nq), tiled_dev(seeds, nq), tiled_dev(seed_count, nq)
    outs = {n: Out(nq, () if n == "count" else (k,), ty) for n, ty in zip(nat.GraphIndex.OUTS, nat.GraphIndex._OUT_T)}
    g.reserve(nq, k, limit)
    dense.reserve(nq, k)
    reserved(nat, lambda: g.search_device(dense, Qd.data_ptr(), 0, sd.data_ptr(), cd.data_ptr(), ld, ld, nq, k, gp,
                                          [outs[n].ptr() for n in nat.GraphIndex.OUTS], stream()), "graph")
    assert (exp["count"] > 0).any() and (exp["count"] == 0).any()
    for n in GA.OUTS:
        assert_tiled(outs[n].host(n), exp[n], ("amdr_graph_search_device", n))
    g.close()
    dense.close()

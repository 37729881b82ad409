"""The scoped step as one call (amdr_hybrid_scope_device, csrc/scope.hip scope_hybrid_kernel): all eight outputs — the two
channel lists and the fused record — have the bits of amdr_scope_dense_search_device + amdr_scope_bm25_search_device +
amdr_fuse_device on the same arguments, in the one-launch form and in the form that runs those calls inside; the oracle
directly; statelessness; capture; the public interface under both forms."""
import math

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FLT_MAX = float(np.finfo(np.float32).max)
DBL_MAX = float(np.finfo(np.float64).max)
N = 300
LENS_FIT = [0, 1, 3, 28, 64, 65, 256]   # every scope inside one slab of both channels: the one-launch form
LENS_OVER = LENS_FIT + [257]            # rows_max = 257: two dense slabs, the call runs the separate launches inside
DEPTHS = [(1, 1), (10, 10), (16, 16), (20, 12), (17, 16)]  # the last: 33 candidates, the separate launches inside
FUSIONS = [("weighted_sum", 0.0), ("rrf", 0.0), ("weighted_sum", 0.2)]  # (tests/test_hybrid_small_gpu.py)
OUTS = ("dense_scores", "dense_ids", "bm25_scores", "bm25_ids", "ids", "vals", "mask", "count")


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


@pytest.fixture(autouse=True)
def default_env(monkeypatch):
    monkeypatch.delenv("AMDR_SCOPE_SLAB", raising=False)
    monkeypatch.delenv("AMDR_SCOPE_FUSED", raising=False)
    monkeypatch.delenv("AMDR_SCOPE_OVERLAP", raising=False)


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
    order = np.lexsort((rows, np.where(nan, 0.0, -key), nan))[:k]
    s = np.full(k, pad, dtype=scores.dtype)
    i = np.full(k, -1, dtype=np.int64)
    s[:order.size] = key[order]
    i[:order.size] = np.asarray(rows)[order]
    return s, i


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b))
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    both_nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((a.view(u) == b.view(u)) | both_nan))


def exact_corpus(rng, n, d):
    """Dense components are multiples of 1/8 in [-1, 1] (products multiples of 1/64, sums far inside 24 bits), so the fp64
    oracle and the fp32 GEMV give the same numbers and ties are real; rows 100-104 repeat row 7.  A toy BM25 vocabulary
    of 120 words in documents of 3-29 tokens: most documents score zero for a six-word query."""
    X = (rng.integers(-8, 9, size=(n, d)) / 8.0).astype(np.float32)
    X[100:105] = X[7]
    words = [f"w{j}" for j in range(120)]
    docs = [[words[j] for j in rng.integers(0, len(words), size=int(rng.integers(3, 30)))] for _ in range(n)]
    return X, words, docs


class World:
    """One corpus, its two indexes and the scope tables of both channels on the device."""

    def __init__(self, nat, d):
        from oracle import bm25 as OB
        rng = np.random.default_rng(1000 + d)
        self.nat, self.d = nat, d
        self.X, self.words, self.docs = exact_corpus(rng, N, d)
        self.ob = OB.BM25Okapi(self.docs)
        self.csr = OB.to_csr(self.ob)
        c = self.csr
        self.dense = nat.DenseIndex(self.X)
        self.bm25 = nat.BM25Index(c["term_ptr"], c["post_doc"], c["post_tf"], c["idf"], c["doc_len"], self.ob.avgdl, self.ob.k1,
                                  self.ob.b)
        self.n_terms = len(c["vocab"])
        self.ws = nat.ScopeWorkspace()
        self.ws.reserve(37, 20, 300)  # the separate launches (inside the call, and as the reference) beyond one slab
        # uids: one map for both channels (the union is over uids); d = 768 runs without maps
        self.map = torch.from_numpy(7 * np.arange(N, dtype=np.int64) + 3).to(DEV) if d == 4 else None
        self.tables = {}
        for name, lens in (("fit", LENS_FIT), ("over", LENS_OVER)):
            per_chan = []
            for c in range(2):  # different row lists for the dense and the BM25 table
                lists = [np.sort(rng.choice(N, size=m, replace=False)) for m in lens]
                lists[4] = lists[4].copy()
                lists[4][0], lists[4][-1] = -5, N  # a row of -5 and a row of n in the 64-row scope: skipped, never read
                if c == 0:
                    tied = np.asarray([7, 100, 101, 102, 103, 104])  # the 28-row dense scope holds the tied rows
                    lists[3] = np.sort(np.concatenate([tied, rng.choice(np.setdiff1d(np.arange(N), tied), size=22, replace=False)]))
                ptr, rows = make_table(lists)
                per_chan.append((lists, torch.from_numpy(ptr).to(DEV), torch.from_numpy(rows).to(DEV), len(lens),
                                 int(np.diff(ptr).max())))
            self.tables[name] = per_chan

    def queries(self, nq, seed):
        """(Q [nq, d], token ids per query, qscope of the dense table, qscope of the BM25 table); in a batch of 37: query
        3 has no known token, 4 a duplicated token, 5 no token at all, 6 a NaN query row."""
        rng = np.random.default_rng(seed)
        Q = (rng.integers(-8, 9, size=(nq, self.d)) / 8.0).astype(np.float32)
        toks = [[int(t) for t in rng.integers(0, self.n_terms, size=int(rng.integers(1, 40)))] for _ in range(nq)]
        if nq > 6:
            toks[3] = [-1, self.n_terms, self.n_terms + 5]
            toks[4] = [toks[4][0]] * 3 + toks[4]
            toks[5] = []
            Q[6, 1] = np.nan
        return Q, toks

    def qscopes(self, nq, n_scopes):
        """Different maps for the two tables; values -1 and n_scopes (outside the table) among them."""
        q = np.arange(nq)
        return (((q * 7 + nq) % (n_scopes + 2)) - 1).astype(np.int32), (((q * 11 + 2 * nq + 1) % (n_scopes + 2)) - 1).astype(np.int32)


@pytest.fixture(scope="module", params=[4, 768], ids=["d4", "d768"])
def world(request, nat):
    return World(nat, request.param)


def buffers(nq, kd, kb, kc=0):
    mo = kd + kb + kc
    return {"dense_scores": torch.full((nq, kd), 7.0, dtype=torch.float32, device=DEV),
            "dense_ids": torch.full((nq, kd), 77, dtype=torch.int64, device=DEV),
            "bm25_scores": torch.full((nq, kb), 7.0, dtype=torch.float64, device=DEV),
            "bm25_ids": torch.full((nq, kb), 77, dtype=torch.int64, device=DEV),
            "ids": torch.full((nq, mo), 77, dtype=torch.int64, device=DEV),
            "vals": torch.full((nq, mo, 9), 7.0, dtype=torch.float64, device=DEV),
            "mask": torch.full((nq, mo), 77, dtype=torch.int32, device=DEV),
            "count": torch.full((nq,), 77, dtype=torch.int32, device=DEV)}


def host(o):
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy() for k in OUTS}


def run_step(w, params, Q, qt, qp, td, tb, nq, kd, kb, colbert=None, ws=None):
    """amdr_hybrid_scope_device; td / tb = (scope_ptr, rows, qscope, n_scopes, rows_max) device tensors + sizes."""
    kc = colbert[2] if colbert else 0
    o = buffers(nq, kd, kb, kc)
    m = w.map.data_ptr() if w.map is not None else 0
    (ws or w.ws).hybrid(w.dense, w.bm25, params, Q.data_ptr(), qt.data_ptr(), qp.data_ptr(),
                        (td[0].data_ptr(), td[1].data_ptr(), td[2].data_ptr(), td[3], td[4]),
                        (tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), tb[3], tb[4]), nq, kd, kb, (m, m, m),
                        (colbert[0].data_ptr(), colbert[1].data_ptr(), kc) if colbert else None,
                        (o["dense_scores"].data_ptr(), o["dense_ids"].data_ptr(), o["bm25_scores"].data_ptr(),
                         o["bm25_ids"].data_ptr()),
                        (o["ids"].data_ptr(), o["vals"].data_ptr(), o["mask"].data_ptr(), o["count"].data_ptr()), 0)
    return o


def run_separate(w, params, Q, qt, qp, td, tb, nq, kd, kb, colbert=None):
    """The three existing calls on the same arguments."""
    kc = colbert[2] if colbert else 0
    o = buffers(nq, kd, kb, kc)
    m = w.map.data_ptr() if w.map is not None else 0
    w.ws.dense_search_device(w.dense, Q.data_ptr(), (td[0].data_ptr(), td[1].data_ptr(), td[2].data_ptr(), td[3], td[4]), nq,
                             kd, o["dense_scores"].data_ptr(), o["dense_ids"].data_ptr(), 0)
    w.ws.bm25_search_device(w.bm25, qt.data_ptr(), qp.data_ptr(),
                            (tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), tb[3], tb[4]), nq, kb,
                            o["bm25_scores"].data_ptr(), o["bm25_ids"].data_ptr(), 0)
    w.nat.fuse_device(params, nq, (o["dense_ids"].data_ptr(), o["dense_scores"].data_ptr(), kd, m),
                      (o["bm25_ids"].data_ptr(), o["bm25_scores"].data_ptr(), kb, m),
                      (colbert[0].data_ptr(), colbert[1].data_ptr(), kc, m) if colbert else None,
                      o["ids"].data_ptr(), o["vals"].data_ptr(), o["mask"].data_ptr(), o["count"].data_ptr())
    return o


def device_queries(w, nq, seed):
    Q, toks = w.queries(nq, seed)
    qt_h, qp_h = w.nat.BM25Index.pack_queries(toks)
    qt = torch.from_numpy(np.concatenate([qt_h, np.zeros(1, np.int32)])).to(DEV)
    return Q, toks, torch.from_numpy(Q).to(DEV), qt, torch.from_numpy(qp_h).to(DEV)


def device_tables(w, name, nq):
    (ld, pd, rd, nsd, rmd), (lb, pb, rb, nsb, rmb) = w.tables[name]
    qsd, qsb = w.qscopes(nq, nsd)
    return (ld, lb, qsd, qsb, (pd, rd, torch.from_numpy(qsd).to(DEV), nsd, rmd), (pb, rb, torch.from_numpy(qsb).to(DEV), nsb, rmb))


@pytest.mark.parametrize("table", ["fit", "over"])
@pytest.mark.parametrize("nq", [1, 2, 5, 37])
def test_all_eight_outputs_have_the_bits_of_the_three_calls(world, table, nq):
    w = world
    Q, toks, Qd, qt, qp = device_queries(w, nq, 50 + nq)
    ld, lb, qsd, qsb, td, tb = device_tables(w, table, nq)
    for kd, kb in DEPTHS:
        fused, _ = w.nat.hybrid_scope_plan(nq, kd, kb, 0, td[4], tb[4])
        assert fused == (table == "fit" and kd + kb <= 32)  # which form the call below takes
        for method, mf in FUSIONS:
            params = w.nat.make_fuse_params(method=method, min_final_score=mf)
            a = host(run_step(w, params, Qd, qt, qp, td, tb, nq, kd, kb))
            b = host(run_separate(w, params, Qd, qt, qp, td, tb, nq, kd, kb))
            for name in OUTS:
                assert same_bits(a[name], b[name]), (table, nq, kd, kb, method, mf, name)
        # the contracts of the scoped channels, on the step's own lists
        for q in range(nq):
            for lists, qs, n_sc, ids, sc, k, pad in ((ld, qsd, td[3], a["dense_ids"], a["dense_scores"], kd, -FLT_MAX),
                                                   (lb, qsb, tb[3], a["bm25_ids"], a["bm25_scores"], kb, -DBL_MAX)):
                rows = lists[qs[q]] if 0 <= qs[q] < n_sc else np.zeros(0, np.int64)
                rows = rows[(rows >= 0) & (rows < N)]  # a row outside [0, n) is skipped
                m = min(k, rows.size)
                assert np.all(ids[q, m:] == -1) and np.all(sc[q, m:] == pad), (q, k)
                assert set(ids[q, :m].tolist()) <= set(rows.tolist()) and len(set(ids[q, :m].tolist())) == m
            if (not 0 <= qsd[q] < td[3] or ld[qsd[q]].size == 0) and (not 0 <= qsb[q] < tb[3] or lb[qsb[q]].size == 0):
                assert a["count"][q] == 0 and np.all(a["ids"][q] == -1)  # a fusion of nothing
        if nq == 37:
            for q in (3, 5):  # no known token / no token: the first kb scope documents at +0.0
                if 0 <= qsb[q] < tb[3]:
                    rows = lb[qsb[q]]
                    rows = rows[(rows >= 0) & (rows < N)][:kb]
                    assert a["bm25_ids"][q, :rows.size].tolist() == rows.tolist()
                    assert np.all(a["bm25_scores"][q, :rows.size] == 0.0) and not np.any(np.signbit(a["bm25_scores"][q, :rows.size]))
            if 0 <= qsd[6] < td[3] and ld[qsd[6]].size:  # the NaN query row: every score NaN, ids ascending (ties)
                m = min(kd, int(((ld[qsd[6]] >= 0) & (ld[qsd[6]] < N)).sum()))
                assert np.all(np.isnan(a["dense_scores"][6, :m])) and np.all(np.diff(a["dense_ids"][6, :m]) > 0)


def test_overlapped_and_sequential_phase_orders_give_the_same_bits(world, monkeypatch):
    """BM25 scopes of <= 64 documents (0, 1, 3, 28, 64 here) run on wave 0 beside the dense rows of waves 1-3, longer ones
    (65, 256) after the dense piece on all four waves; AMDR_SCOPE_OVERLAP=0 pins the second order for every scope."""
    w = world
    nq = 37
    Q, toks, Qd, qt, qp = device_queries(w, nq, 71)
    ld, lb, qsd, qsb, td, tb = device_tables(w, "fit", nq)
    assert {int(lb[s].size) for s in qsb if 0 <= s < tb[3]} >= {0, 1, 3, 28, 64, 65, 256}
    for kd, kb in ((10, 10), (20, 12), (1, 1)):
        params = w.nat.make_fuse_params()
        a = host(run_step(w, params, Qd, qt, qp, td, tb, nq, kd, kb))
        monkeypatch.setenv("AMDR_SCOPE_OVERLAP", "0")
        s = host(run_step(w, params, Qd, qt, qp, td, tb, nq, kd, kb))
        monkeypatch.delenv("AMDR_SCOPE_OVERLAP")
        b = host(run_separate(w, params, Qd, qt, qp, td, tb, nq, kd, kb))
        for name in OUTS:
            assert same_bits(a[name], b[name]) and same_bits(s[name], b[name]), (kd, kb, name)


def test_ties_take_the_lower_id_in_the_step(world):
    """Rows 100-104 repeat row 7 and all six sit in the 28-row dense scope: a query equal to that row ranks them first, in
    id order."""
    w = world
    nq, kd, kb = 2, 22, 10
    Q, toks, Qd, qt, qp = device_queries(w, nq, 9)
    Q[:] = w.X[7]
    Qd = torch.from_numpy(Q).to(DEV)
    (ld, pd, rd, nsd, rmd), (lb, pb, rb, nsb, rmb) = w.tables["fit"]
    qs = torch.full((nq,), 3, dtype=torch.int32, device=DEV)
    a = host(run_step(w, w.nat.make_fuse_params(), Qd, qt, qp, (pd, rd, qs, nsd, rmd), (pb, rb, qs, nsb, rmb), nq, kd, kb))
    ids = a["dense_ids"][0].tolist()
    at = ids.index(7)  # the six tied rows: next to each other, the lower id first
    assert ids[at:at + 6] == [7, 100, 101, 102, 103, 104]
    assert len(set(a["dense_scores"][0, at:at + 6].tolist())) == 1


def test_step_behind_a_colbert_list_equals_the_four_launches(world, nat):
    w = world
    nq, k = 5, 10
    rng = np.random.default_rng(77)
    lens = rng.integers(1, 40, size=N)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    D = (rng.integers(-8, 9, size=(int(ptr[-1]), 128)) / 8.0).astype(np.float32)
    mi = nat.MaxSimIndex(D, ptr)
    Qt = torch.from_numpy((rng.integers(-8, 9, size=(nq, 32, 128)) / 8.0).astype(np.float32)).to(DEV)
    Q, toks, Qd, qt, qp = device_queries(w, nq, 31)
    ld, lb, qsd, qsb, td, tb = device_tables(w, "fit", nq)
    cs = torch.empty((nq, k), dtype=torch.float32, device=DEV)
    ci = torch.empty((nq, k), dtype=torch.int64, device=DEV)
    w.ws.maxsim_search_device(mi, Qt.data_ptr(), 32, (tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), tb[3], tb[4]), nq, k,
                              cs.data_ptr(), ci.data_ptr(), 0)
    assert nat.hybrid_scope_plan(nq, k, k, k, td[4], tb[4])[0]
    for method, mf in FUSIONS + [("rrf_norm_blend", -math.inf), ("wrrf", 0.0)]:
        params = nat.make_fuse_params(method=method, min_final_score=mf)
        a = host(run_step(w, params, Qd, qt, qp, td, tb, nq, k, k, colbert=(ci, cs, k)))
        b = host(run_separate(w, params, Qd, qt, qp, td, tb, nq, k, k, colbert=(ci, cs, k)))
        for name in OUTS:
            assert same_bits(a[name], b[name]), (method, mf, name)
        assert a["ids"].shape == (nq, 3 * k) and (a["mask"] & 4).any()  # the third channel took part


def test_step_against_the_oracle_directly(world):
    from oracle import dense as OD
    from oracle import fusion as OF
    w = world
    nq, k = 8, 10
    Q, toks, Qd, qt, qp = device_queries(w, nq, 5)
    Q[6] = np.nan_to_num(Q[6])  # (no NaN row here: the oracle's order of NaNs is not the channel's)
    Qd = torch.from_numpy(Q).to(DEV)
    ld, lb, qsd, qsb, td, tb = device_tables(w, "fit", nq)
    params = w.nat.make_fuse_params(method="rrf_norm_blend", rrf_k=60, alpha=0.5, w_dense=0.6, w_bm25=0.4, w_colbert=0.35,
                                    min_final_score=-math.inf)
    a = host(run_step(w, params, Qd, qt, qp, td, tb, nq, k, k))
    inv = {v: t for t, v in w.csr["vocab"].items()}
    dref = OD.flatip_scores(w.X, Q).astype(np.float64)
    uid = (lambda r: 7 * int(r) + 3) if w.map is not None else int
    FV = w.nat.FV
    checked = 0
    for q in range(nq):
        rd = ld[qsd[q]] if 0 <= qsd[q] < td[3] else np.zeros(0, np.int64)
        rb = lb[qsb[q]] if 0 <= qsb[q] < tb[3] else np.zeros(0, np.int64)
        rd, rb = rd[(rd >= 0) & (rd < N)], rb[(rb >= 0) & (rb < N)]
        es, ei = ranked(dref[q, rd], rd, k, -DBL_MAX)
        assert np.array_equal(a["dense_ids"][q], ei)
        assert np.array_equal(a["dense_scores"][q, :min(k, rd.size)].astype(np.float64), es[:min(k, rd.size)])  # exact
        bsc = w.ob.get_scores([inv[t] for t in toks[q] if t in inv])
        bs, bi = ranked(bsc[rb], rb, k, -DBL_MAX)
        assert np.array_equal(a["bm25_ids"][q], bi) and same_bits(a["bm25_scores"][q], bs)
        exp = OF.fuse([(uid(i), float(s)) for s, i in zip(es, ei) if i >= 0], [(uid(i), float(s)) for s, i in zip(bs, bi) if i >= 0],
                      [], {"dense_weight": 0.6, "bm25_weight": 0.4, "colbert_weight": 0.35, "rrf_alpha": 0.5, "rrf_k": 60,
                           "fusion_method": "rrf_norm_blend"})
        assert a["count"][q] == len(exp)
        assert a["ids"][q, :len(exp)].tolist() == [h["id"] for h in exp] and np.all(a["ids"][q, len(exp):] == -1)
        for r, h in enumerate(exp):
            sb = h["breakdown"]
            want = {"score": h["score"], "rrf_norm": sb["rrf_norm"], "weighted_sum": sb["weighted_sum"],
                    "dense_norm": sb["dense_norm"], "bm25_norm": sb["bm25_norm"], "colbert_norm": sb["colbert_norm"],
                    "contrib_dense": sb["channel_contrib"]["dense"], "contrib_bm25": sb["channel_contrib"]["bm25"],
                    "contrib_colbert": sb["channel_contrib"]["colbert"]}
            for name, v in want.items():
                assert same_bits(a["vals"][q, r, FV[name]:FV[name] + 1], np.asarray([v], dtype=np.float64)), (q, r, name)
            checked += 1
    assert checked > 40


def test_twenty_launches_on_one_handle_pair_are_identical_and_need_no_workspace(world, nat):
    w = world
    nq, k = 5, 10
    Q, toks, Qd, qt, qp = device_queries(w, nq, 13)
    ld, lb, qsd, qsb, td, tb = device_tables(w, "fit", nq)
    params = nat.make_fuse_params(min_final_score=0.1)
    ws = nat.ScopeWorkspace()  # never reserved: the one-launch form takes nothing from it
    first = host(run_step(w, params, Qd, qt, qp, td, tb, nq, k, k, ws=ws))
    assert (first["ids"] >= 0).any()
    g0 = nat.workspace_growths()
    for _ in range(20):
        again = host(run_step(w, params, Qd, qt, qp, td, tb, nq, k, k, ws=ws))
        for name in OUTS:
            assert same_bits(again[name], first[name]), name
    assert nat.workspace_growths() == g0
    # ... while the form that runs the separate calls inside needs the reserve, as those calls do
    ld, lb, qsd, qsb, td, tb = device_tables(w, "over", nq)
    with pytest.raises(nat.NativeError, match="reserve"):
        run_step(w, params, Qd, qt, qp, td, tb, nq, k, k, ws=ws)
    ws.close()


def test_captured_step_replays_with_the_tables_rewritten_in_place(nat):
    from legal_rag_amd.retrieval.engine import HybridEngine
    from oracle import bm25 as OB
    rng = np.random.default_rng(21)
    n, nq, k = 300, 5, 10
    X, words, docs = exact_corpus(rng, n, 64)
    ob = OB.BM25Okapi(docs)
    c = OB.to_csr(ob)
    eng = HybridEngine(nat.DenseIndex(X), nat.BM25Index(c["term_ptr"], c["post_doc"], c["post_tf"], c["idf"], c["doc_len"],
                                                        ob.avgdl, ob.k1, ob.b), None)
    params = nat.make_fuse_params(min_final_score=0.0)
    Q = torch.from_numpy((rng.integers(-8, 9, size=(nq, 64)) / 8.0).astype(np.float32)).to(DEV)
    q_terms, q_ptr = nat.BM25Index.pack_queries([[int(t) for t in rng.integers(0, len(words), size=5)] for _ in range(nq)])
    q_terms_d, q_ptr_d = torch.from_numpy(q_terms).to(DEV), torch.from_numpy(q_ptr).to(DEV)
    rows_max = 150  # one slab of both channels: the captured step is the one launch
    assert nat.hybrid_scope_plan(nq, k, k, 0, rows_max, rows_max)[0]
    tabs = []
    for _ in range(2):  # the dense and the BM25 table: their own tensors
        tabs.append((torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(3 * rows_max, dtype=torch.int64, device=DEV),
                     torch.zeros(nq, dtype=torch.int32, device=DEV), 3, rows_max))

    def write(seed):
        for j, (sp, rw, qs, _, _) in enumerate(tabs):
            r = np.random.default_rng(seed * 10 + j)
            lists = [np.sort(r.choice(n, size=int(m), replace=False)) for m in r.integers(1, rows_max, size=3)]
            p, rr = make_table(lists)
            sp.copy_(torch.from_numpy(p))
            rw[:rr.size].copy_(torch.from_numpy(rr))
            qs.copy_(torch.from_numpy(r.integers(0, 4, size=nq).astype(np.int32)))  # (3: outside -> padding)

    def snapshot(res):
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (res.ids, res.vals, res.mask, res.count, res.dense_ids, res.dense_scores,
                                                 res.bm25_ids, res.bm25_scores)]
    kw = dict(q_emb=Q, q_terms=q_terms_d, q_ptr=q_ptr_d, scopes=(tabs[0], tabs[1], None))
    write(1)
    graph, gres = eng.capture(params, k, **kw)
    g0 = nat.workspace_growths()
    for seed in (2, 3):
        write(seed)
        graph.replay()
        got = snapshot(gres)
        exp = snapshot(eng.search_batch(params, k, **kw))  # the eager step on the new tables
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
    data = tmp_path_factory.mktemp("scope_step_data")
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


def test_public_searches_give_the_same_dumps_under_both_forms(ucc_index, nat, monkeypatch):
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from legal_rag_amd.retrieval.scope import Scope
    cfg, chunks = ucc_index
    sizes = {}
    for c in chunks:
        if c.section:
            sizes[c.section] = sizes.get(c.section, 0) + 1
    sec28 = min(sizes, key=lambda s: (abs(sizes[s] - 28), s))
    s1, s2 = Scope(section=chunks[10].section), Scope(section=chunks[150].section)
    scopes = [None, s1, None, Scope(section="no such section"), s2, s1]
    qs = [QUESTIONS[j % len(QUESTIONS)] for j in range(len(scopes))]

    def run():
        r = HybridRetriever(cfg)
        one = [[dump(h) for h in r.search(q, top_k=10, scope=Scope(section=sec28))] for q in QUESTIONS]
        mixed = [[dump(h) for h in hits] for hits in r.search_batch(qs, top_k=10, scopes=scopes)]
        return one, mixed
    ws = nat.ScopeWorkspace()
    assert "scope_hybrid_kernel" in ws.plan_info(1, 10, sizes[sec28])
    fused = run()
    monkeypatch.setenv("AMDR_SCOPE_FUSED", "0")
    assert "scope_hybrid_kernel" not in ws.plan_info(1, 10, sizes[sec28])
    assert "separate launches" in ws.plan_info(1, 10, sizes[sec28])
    separate = run()
    assert fused == separate
    assert all(fused[0][:2]) and fused[1][1] and fused[1][4] and fused[1][3] == []
    ws.close()

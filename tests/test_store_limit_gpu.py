"""Resident stores past byte 2^32, element 2^31 and element 2^32 in every row-indexed call (tests/store_limit_cases.py).

A 5 596 619 x 768 closed-form matrix wrapped by DenseIndex(device_ptr=...), an OWNED 2 800 416 x 768 index for the
updates (they refuse wrapped memory) and a ColBERT store of 2^24 + 3 001 tokens.  Every id and every score bit is compared
with a reference that never calls the library: torch fp64 GEMMs in chunks on the device (exact on these integers), numpy
fp64 on rows made by the formula for the row-addressed calls.  Every case asserts the form that ran, and that what it
compares holds rows on both sides of every mark, so a routing change cannot empty it.

The fixtures build each store once (module scope) and may skip only below a free-HBM need computed from their shapes."""
import time

import numpy as np
import pytest
import torch

import dense_adversary as DA
import maxsim_adversary as MS
import mmr_adversary as MA
import store_limit_cases as SL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GIB = float(1 << 30)
N, D = SL.N_DENSE, SL.D_DENSE
MARK_ROWS = SL.DENSE_MARKS.rows(N)
FILL_TEMPS = 4 * (1 << 18) * D * 8  # the int64 / fp64 temporaries of one 2^18-row chunk of the fill and the reference


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    return _native


def _require_hbm(what, need):
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"{what}: needs {need / GIB:.1f} GiB of free HBM, {free / GIB:.1f} GiB are free")


def _clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def _pin(mp, names, pins):
    for name in names:
        mp.delenv(name, raising=False)
    for name, v in pins.items():
        mp.setenv(name, v)


def _assert_bits(s, i, es, ei, what):
    assert np.array_equal(i, ei), (what, "ids", np.argwhere(i != ei)[:4].tolist(), i[i != ei][:4], ei[i != ei][:4])
    assert DA.bits_equal(s, es), (what, "score bits", np.argwhere(s.view(np.uint32) != es.view(np.uint32))[:4].tolist())


# ---- 1. dense search on the wrapped store -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense(nat):
    """(index over the wrapped matrix, Q on the device, reference scores / ids [161, 128])."""
    # the matrix, its fp16 image (Hi with build_image), one score matrix of kScoreBytesMax, the chunk temporaries
    _require_hbm("dense store-limit cases", N * D * 4 + N * D * 2 + (4 << 30) + FILL_TEMPS)
    t0 = _clock()
    X = torch.empty((N, D), dtype=torch.float32, device=DEV)
    SL.fill_dense_torch(torch, X)
    t1 = _clock()
    Q = torch.from_numpy(SL.dense_queries().copy()).to(DEV)
    ref_s, ref_i = SL.chunked_topk_torch(torch, lambda lo, hi: X[lo:hi], N, Q, 128)
    t2 = _clock()
    idx = nat.DenseIndex(device_ptr=X.data_ptr(), n=N, dim=D, device=0, keepalive=X)
    t3 = _clock()
    print(f"OBS store limit fixture dense: fill {t1 - t0:.1f} s, reference {t2 - t1:.1f} s, create {t3 - t2:.1f} s")
    # the reference itself: every planted row of a query heads its list, in id order, all at 3 sum|q|
    plants = SL.dense_plants()
    for q in SL.PLANT_QUERIES:
        mine = sorted(r for r, qq in plants.items() if qq == q)
        assert ref_i[q, :len(mine)].tolist() == mine and set(ref_s[q, :len(mine)].tolist()) == {3.0 * np.abs(SL.dense_queries()[q]).sum()}
    ref_s.setflags(write=False), ref_i.setflags(write=False)
    yield idx, Q, ref_s, ref_i
    idx.close()
    del X, idx
    torch.cuda.empty_cache()


def _sides(ids, marks=MARK_ROWS):
    """{mark: (a row before the row that holds it is listed, a row behind it is)}"""
    return {m: (bool((ids < r).any()), bool((ids > r).any())) for m, r in marks.items()}


def _device_search(idx, q, nq, k):
    s = torch.full((nq, k), 123.0, dtype=torch.float32, device=DEV)
    i = torch.full((nq, k), 77, dtype=torch.int64, device=DEV)
    idx.search_device(q.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def _search_case(nat, mp, dense, form, nq, k, image=False):
    idx, Q, ref_s, ref_i = dense
    pins = DA.pins_of(form, nq)
    _pin(mp, DA.PIN_NAMES, pins)
    try:
        assert DA.form_of(N, D, nq, k, pins) == form, (form, nq, k)
        plan = idx.plan_info(nq, k)
        assert DA.form_from_plan(plan) == form, (form, nq, k, plan)
        if form == DA.HI:
            assert ("dense_hi_image_tilemax_kernel" in plan) == image, plan
        es, ei = ref_s[:nq, :k], ref_i[:nq, :k]
        # what is compared: query 0's list holds rows before and behind every mark (its planted rows tie across them)
        assert all(a and b for a, b in _sides(ei[0]).values()), _sides(ei[0])
        q = Q[:nq].contiguous()
        s, i = _device_search(idx, q, nq, k)
        _assert_bits(s, i, es, ei, (form, nq, k, "eager"))
        idx.reserve(nq, k)
        before = nat.workspace_growths()
        s, i = _device_search(idx, q, nq, k)
        assert nat.workspace_growths() == before, (form, nq, k, "the call grew a workspace inside its reserve")
        _assert_bits(s, i, es, ei, (form, nq, k, "inside reserve"))
        return plan
    finally:
        _pin(mp, DA.PIN_NAMES, {})


@pytest.mark.parametrize("k", [10, 128])
@pytest.mark.parametrize("form,nq", [(DA.SCAN, 1), (DA.SCAN, 4), (DA.TILES, 33), (DA.PANEL, 96), (DA.TWOLEVEL, 33),
                                     (DA.TWOLEVEL, 97)])
def test_dense_search_forms(nat, monkeypatch, dense, form, nq, k):
    _search_case(nat, monkeypatch, dense, form, nq, k)


@pytest.mark.parametrize("k", [10, 128])
@pytest.mark.parametrize("nq", [160, 161])
def test_dense_search_largest_score_matrix_and_second_pass(nat, monkeypatch, dense, nq, k):
    """160 queries: one pass with the largest score matrix kScoreBytesMax admits on this store (3.58 GB: its row products
    pass byte 2^32 themselves); 161: that pass and a second one."""
    plan = _search_case(nat, monkeypatch, dense, DA.TILES, nq, k)
    assert "queries_per_launch=160" in plan, plan
    assert 160 * N * 4 <= 4 << 30 < 192 * N * 4 and 160 * N * 4 > 1 << 31


# the fp16 first pass admits k + max(k, 96) + 1 <= 256 candidates: k = 127 is its deepest list (at 128 the route gives
# the exact two-level form, which test_dense_search_forms covers)
@pytest.mark.parametrize("nq,image", [(64, False), (65, True)])
def test_dense_search_fp16_first_pass(nat, monkeypatch, dense, nq, image):
    idx, _, _, ref_i = dense
    if image:
        idx.build_image()
        present, nbytes, rows, _ = idx.image_info()
        assert present and rows == N and nbytes >= N * D * 2 > 1 << 32
    try:
        for k in (10, 127):
            assert DA.form_of(N, D, nq, 128, DA.pins_of(DA.HI, nq)) == DA.TWOLEVEL
            c0 = idx.hi_counters()
            _search_case(nat, monkeypatch, dense, DA.HI, nq, k, image)
            c1 = idx.hi_counters()
            took, unresolved = c1[0] - c0[0], c1[1] - c0[1]
            print(f"OBS store limit Hi nq={nq} k={k} image={image}: fp16 pass took {took} queries, {unresolved} unresolved, "
                  f"level {c1[2]}, in use {c1[3]}, passes {c1[4] - c0[4]}, with the exact chain {c1[5] - c0[5]}")
            assert took == 2 * nq, (took, nq)  # the eager call and the one inside the reserve
            # queries whose list lacks a row behind some mark; the pass resolved more queries than those (per call), so it
            # resolved at least one whose top k holds a row past each mark
            lacking = sum(1 for b in range(nq) if not all(behind for _, behind in _sides(ref_i[b, :k]).values()))
            assert took - unresolved > 2 * lacking, (took, unresolved, lacking)
    finally:
        if image:
            idx.drop_image()


# ---- 2. the row-addressed calls --------------------------------------------------------------------------------------------
WINDOW = SL.mark_window_rows(N, SL.DENSE_MARKS)


def test_read_rows_bytes(dense):
    idx = dense[0]
    for m, row in list(MARK_ROWS.items()) + [("first", 2), ("last", N - 3)]:
        got = idx.read_rows(row - 2, 5)
        want = SL.dense_rows_np(np.arange(row - 2, row + 3)).astype(np.float32)
        assert got.tobytes() == want.tobytes(), m


def test_score_rows(dense):
    idx = dense[0]
    Q = SL.dense_queries()[:9]
    assert all((WINDOW < r).any() and (WINDOW == r).any() and (WINDOW > r).any() for r in MARK_ROWS.values())
    rows = np.tile(np.concatenate([WINDOW, [-1, N]]), (9, 1))
    rows[1::2, :WINDOW.size] = WINDOW[::-1]  # every second query in descending order
    X = SL.dense_rows_np(WINDOW)
    S = Q.astype(np.float64) @ X.T
    got = idx.score_rows(Q, rows)
    want = S.copy()
    want[1::2] = S[1::2, ::-1]
    assert DA.bits_equal(got[:, :WINDOW.size], want.astype(np.float32))
    assert np.all(got[:, WINDOW.size:] == -DA.FLT_MAX)


def _scope_rows():
    parts = [[0, N - 1]] + [np.arange(r - 40, r + 41) for r in MARK_ROWS.values()]
    return np.unique(np.concatenate(parts).astype(np.int64))


@pytest.mark.parametrize("slab", [None, "64"], ids=["default-slabs", "slab-64"])
def test_scoped_dense_search(nat, monkeypatch, dense, slab):
    idx = dense[0]
    _pin(monkeypatch, ("AMDR_SCOPE_SLAB",), {"AMDR_SCOPE_SLAB": slab} if slab else {})
    rows = _scope_rows()
    scopes = [rows, rows[::2], rows[rows > MARK_ROWS["elem2^31"]]]
    for sc in scopes:
        assert all(a and b for a, b in _sides(sc, {m: r for m, r in MARK_ROWS.items() if r >= sc.min()}).values())
    sp = np.concatenate([[0], np.cumsum([len(r) for r in scopes])]).astype(np.int64)
    rw = np.concatenate(scopes)
    nq = 9
    Q = SL.dense_queries()[:nq]
    S = Q.astype(np.float64) @ SL.dense_rows_np(rows).T
    col = {int(r): j for j, r in enumerate(rows)}
    qs = (np.arange(nq) % len(scopes)).astype(np.int32)
    ws = nat.ScopeWorkspace()
    try:
        for k in (10, 100):
            es, ei = np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
            for b in range(nq):
                sc = scopes[qs[b]]
                s1, i1 = DA.oracle_topk(S[b:b + 1, [col[int(r)] for r in sc]], k)
                es[b], ei[b] = s1[0], np.where(i1[0] >= 0, sc[np.maximum(i1[0], 0)], -1)
            s, i = ws.dense_search(idx, Q, sp, rw, qs, k)
            _assert_bits(s, i, es, ei, ("scoped dense", slab, k))
    finally:
        ws.close()
        _pin(monkeypatch, ("AMDR_SCOPE_SLAB",), {})


@pytest.mark.parametrize("slab", [None, "64"], ids=["default-slabs", "slab-64"])
def test_mmr_row_gather(monkeypatch, dense, slab):
    idx = dense[0]
    _pin(monkeypatch, ("AMDR_SCOPE_SLAB",), {"AMDR_SCOPE_SLAB": slab} if slab else {})
    try:
        rng = np.random.default_rng(5)
        uniq = _scope_rows()
        local = SL.dense_rows_np(uniq).astype(np.float32)
        nq, pool, k_sel = 5, 64, 12
        pos = np.stack([rng.permutation(uniq.size)[:pool] for _ in range(nq)])
        pos[0, :WINDOW.size] = np.searchsorted(uniq, WINDOW)  # the rows at, before and behind every mark, in one pool
        rows = uniq[pos]
        assert all(a and b for a, b in _sides(rows[0]).values())
        rel = -np.sort(-rng.uniform(0.1, 1.0, size=(nq, pool)), axis=1)
        count = np.full(nq, pool, np.int32)
        for lam in (0.5, MA.LAM_ODD):
            want = MA.mmr_oracle(local, pos, rel, count, pool, k_sel, lam)
            got = idx.mmr(rows, rel, count, pool, k_sel, lam)
            MA.assert_exact(got, want, ("mmr past the marks", slab, lam))
    finally:
        _pin(monkeypatch, ("AMDR_SCOPE_SLAB",), {})


# ---- 3. updates of an owned index -----------------------------------------------------------------------------------------
NO = SL.N_OWNED
OWN_MARKS = SL.DENSE_MARKS.rows(NO)


@pytest.fixture(scope="module")
def owned(nat):
    """(owned index of f with its planted rows, the model of where each row comes from)."""
    # the matrix, then an update's staged copy: add grows to twice the rows beside the old matrix
    _require_hbm("dense update store-limit cases", NO * D * 4 * 3 + FILL_TEMPS)
    t0 = _clock()
    plants = SL.dense_plants(NO)
    host = np.empty((NO, D), np.float32)
    step = 1 << 18
    for lo in range(0, NO, step):
        hi = min(NO, lo + step)
        blk = torch.empty((hi - lo, D), dtype=torch.float32, device=DEV)
        SL.fill_dense_torch(torch, blk, row0=lo, plants=plants)
        host[lo:hi] = blk.cpu().numpy()
    del blk
    t1 = _clock()
    idx = nat.DenseIndex(host)
    del host
    model = SL.RowSource(NO)
    rows = sorted(plants)
    model.replace(rows, extra=[SL.plant_row(plants[r], r) for r in rows])
    print(f"OBS store limit fixture owned: fill on the device and copy to the host {t1 - t0:.1f} s, create {_clock() - t1:.1f} s")
    yield idx, model
    idx.close()
    torch.cuda.empty_cache()


def _check_rows(idx, model, positions, what):
    """score_rows of the probe queries on ~10 000 rows against numpy on the rows the model says are there."""
    assert idx.ntotal == model.n, (what, idx.ntotal, model.n)
    ids = SL.sample_ids(model.n, [p for p in positions if 0 <= p < model.n])
    P = SL.probe_queries()
    want = (P.astype(np.float64) @ model.rows(ids).T).astype(np.float32)
    got = idx.score_rows(P, np.tile(ids, (P.shape[0], 1)))
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert DA.bits_equal(got, want), (what, len(bad), "first wrong (probe, row id):", [(int(a), int(ids[b])) for a, b in bad[:6]])
    return ids


def test_dense_updates_across_the_marks(nat, monkeypatch, owned):
    idx, model = owned
    m_byte, m_int = OWN_MARKS["byte2^32"], OWN_MARKS["elem2^31"]
    ids = _check_rows(idx, model, [m_byte, m_int], "as created")
    assert ids.size > 10_000 and all(r in ids for r in (m_byte - 1, m_byte, m_byte + 1, m_int - 1, m_int, m_int + 1, NO - 1))

    # replace: the rows at the marks and their neighbours, row 5 and the last row; the mark rows become planted rows
    rep = np.array(sorted({5, NO - 1} | {r + o for r in (m_byte, m_int) for o in (-1, 0, 1)}), np.int64)
    extra = [SL.plant_row(2, int(r) + 10_000_000) if r in (m_byte, m_int) else
             SL.plant_row(0, int(r) + 10_000_000) if r not in (5, NO - 1) else None for r in rep]  # (the neighbours: query 0's)
    model.replace(rep, src=rep + 10_000_000, extra=extra)
    idx.replace(rep, model.rows(rep).astype(np.float32))
    _check_rows(idx, model, [m_byte, m_int], "after replace")

    # remove: a spread from row 1 000 on (well before the first mark: every later row shifts across it) with the rows
    # that hold the marks; the total falls below the 2^31-element mark
    rem = np.unique(np.concatenate([np.arange(1000, NO, 461), [m_byte, m_int]]).astype(np.int64))
    old = model.remove(rem)
    idx.remove(rem)

    def new_of(r):  # where old row r (or its successor) sits now
        return int(np.searchsorted(old, r))
    assert model.n * D < 1 << 31 < NO * D and model.n * D * 4 > 1 << 32
    moved_across = int(np.count_nonzero((old >= m_byte + 1) & (np.arange(model.n) < m_byte)))
    assert moved_across > 1000  # rows that sat behind the byte mark and now sit before it
    _check_rows(idx, model, [m_byte, m_int, new_of(m_byte), new_of(m_int), new_of(m_byte) - 3000], "after remove")

    # add: the total crosses the 2^31-element mark from below
    n0 = model.n
    add = 20_000_000 + np.arange(5000, dtype=np.int64)
    model.add(add)
    assert n0 * D < 1 << 31 < model.n * D and n0 <= m_int < model.n - 1
    model.replace([m_int, m_int + 1], extra=[SL.plant_row(0, 30_000_000), SL.plant_row(0, 30_000_001)])  # planted among the new rows
    idx.add(model.rows(np.arange(n0, model.n)).astype(np.float32))
    _check_rows(idx, model, [m_byte, m_int, n0, new_of(m_byte)], "after add")

    # one planted search on the updated index: a reference over all its rows, made from the model on the device
    src = torch.from_numpy(model.src).to(DEV)
    ex_ids = np.nonzero(model.src < 0)[0]
    ex = torch.from_numpy(model.rows(ex_ids).astype(np.float32)).to(DEV)
    ex_ids_d = torch.from_numpy(ex_ids).to(DEV)

    def rows_of(lo, hi):
        X = SL.f_torch(torch, src[lo:hi].clamp(min=0)).float()
        hit = (ex_ids_d >= lo) & (ex_ids_d < hi)
        X[ex_ids_d[hit] - lo] = ex[hit]
        return X
    nq, k = 33, 10
    Q = SL.dense_queries()[:nq]
    es, ei = SL.chunked_topk_torch(torch, rows_of, model.n, torch.from_numpy(Q.copy()).to(DEV), k)
    # query 0's planted rows: the replaced neighbours of both marks, moved by the remove, and two of the added rows
    mine = [new_of(m_byte - 1), new_of(m_byte + 1), new_of(m_int - 1), new_of(m_int + 1), m_int, m_int + 1]
    assert ei[0, :6].tolist() == mine and len(set(es[0, :6].tolist())) == 1
    assert mine[1] < m_byte < mine[2] and mine[3] < m_int < mine[5]  # ties across both marks, the lower id first
    for form, n_q in ((DA.SCAN, 4), (DA.TILES, 33)):
        pins = DA.pins_of(form, n_q)
        _pin(monkeypatch, DA.PIN_NAMES, pins)
        try:
            assert DA.form_from_plan(idx.plan_info(n_q, k)) == form
            s, i = idx.search(Q[:n_q], k)
        finally:
            _pin(monkeypatch, DA.PIN_NAMES, {})
        _assert_bits(s, i, es[:n_q], ei[:n_q], ("search after the updates", form))


# ---- 4. the ColBERT store ---------------------------------------------------------------------------------------------------
T = SL.T_MS
MS_STORE_BYTES = T * SL.DIM_MS * (4 + 4 + 2)  # D, img (hi and lo), img_hi


@pytest.fixture(scope="module")
def colbert(nat):
    """(index, DocSource model, Q [8, 32, 128], reference scores fp64 [8, n_docs] as numpy)."""
    # the store with its two images, an update's staged store (add: twice the capacity) beside it
    _require_hbm("ColBERT store-limit cases", 3 * MS_STORE_BYTES + FILL_TEMPS)
    SL.ms_range_certificate()
    t0 = _clock()
    ptr = SL.ms_doc_ptr()
    model = SL.DocSource(ptr)
    Dd = torch.empty((T, SL.DIM_MS), dtype=torch.float32, device=DEV)
    step = 1 << 20
    for lo in range(0, T, step):
        hi = min(T, lo + step)
        Dd[lo:hi] = SL.g_torch(torch, torch.arange(lo, hi, dtype=torch.int64, device=DEV)).float()
    t1 = _clock()
    Q = SL.ms_queries()
    seg = torch.from_numpy(model.all_tokens()[1]).to(DEV)
    ref = SL.ms_scores_torch(torch, lambda lo, hi: Dd[lo:hi], seg, model.n, torch.from_numpy(Q.copy()).to(DEV)).cpu().numpy()
    t2 = _clock()
    host = np.empty((T, SL.DIM_MS), np.float32)
    for lo in range(0, T, step):
        host[lo:lo + step] = Dd[lo:lo + step].cpu().numpy()
    del Dd, seg
    torch.cuda.empty_cache()
    t3 = _clock()
    idx = nat.MaxSimIndex(host, ptr)
    del host
    print(f"OBS store limit fixture colbert: fill {t1 - t0:.1f} s, reference {t2 - t1:.1f} s, copy to the host {t3 - t2:.1f} s, "
          f"create {_clock() - t3:.1f} s; {model.n} documents")
    info = idx.info()
    assert info[0] == model.n and info[1] == T and info[4] == 1
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and np.abs(ref).max() < MS.LIMIT
    yield idx, model, Q, ref
    idx.close()
    torch.cuda.empty_cache()


def _ms_reference(model, Q):
    """The fp64 scores of every document of the store the model describes, from g on the device."""
    tok, seg = model.all_tokens()
    tok_d, seg_d = torch.from_numpy(tok).to(DEV), torch.from_numpy(seg).to(DEV)
    out = SL.ms_scores_torch(torch, lambda lo, hi: SL.g_torch(torch, tok_d[lo:hi]), seg_d, model.n, torch.from_numpy(Q.copy()).to(DEV))
    return out.cpu().numpy()


def _straddlers(model):
    ptr = model.ptr()
    return ptr, {s: SL.ms_doc_of(ptr, s) for s in (1 << 23, 1 << 24) if s < ptr[-1]}


MS_PINS = (MS.P_DEF, MS.P_F32, MS.P_ONE)


@pytest.mark.parametrize("nq", [1, 7, 8])
def test_maxsim_scores_and_search(monkeypatch, colbert, nq):
    """nq 1 and 7: the pair forms; 8: the forms of a batch (ring, two-pass, blocked) — every form of
    maxsim_adversary.FORMS but the scoped one, which has its own test."""
    idx, model, Q, ref = colbert
    ptr, st = _straddlers(model)
    for s, d in st.items():
        assert ptr[d] < s < ptr[d + 1] and 0 < d < model.n - 1  # a document straddles the mark; documents on both sides
    n, k = model.n, 10
    q = Q[:nq]
    want = ref[:nq].astype(np.float32)
    seen = set()
    for pins in MS_PINS:
        _pin(monkeypatch, MS.PIN_NAMES, pins)
        try:
            form = MS.form_of(n, nq, 1, False, pins)
            assert MS.form_from_plan(idx.plan_info(nq)) == MS.form_of(n, nq, 1, True, pins), (pins, idx.plan_info(nq))
            got = idx.scores(q)
            bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
            assert MS.same_scores(got, want), (form, pins, len(bad), "first wrong (query, document):", bad[:6].tolist())
            seen.add(form)
            form = MS.form_of(n, nq, k, True, pins)
            es, ei = MS.topk_expected(want, k)
            s, i = idx.search(q, k)
            assert np.array_equal(i, ei) and MS.same_scores(s, es), (form, pins, i.tolist(), ei.tolist())
            seen.add(form)
        finally:
            _pin(monkeypatch, MS.PIN_NAMES, {})
    assert seen == ({MS.PAIRHALF, MS.PAIRF32} if nq < MS.K_MSQ else {MS.RING, MS.TWOPASS, MS.BLOCKED}), seen


@pytest.mark.parametrize("slab", [None, "4"], ids=["default-slabs", "slab-4"])
def test_scoped_maxsim_on_the_straddlers(nat, monkeypatch, colbert, slab):
    idx, model, Q, ref = colbert
    _, st = _straddlers(model)
    scope = np.unique(np.concatenate([[0, model.n - 1]] + [np.arange(d - 3, d + 4) for d in st.values()]).astype(np.int64))
    assert len(st) == 2 and all(d in scope and d - 1 in scope and d + 1 in scope for d in st.values())
    _pin(monkeypatch, MS.PIN_NAMES, {"AMDR_SCOPE_SLAB": slab} if slab else {})
    ws = nat.ScopeWorkspace()
    try:
        for nq in (1, 7):
            for k in (10, scope.size):
                es, ei = MS.topk_expected(ref[:nq].astype(np.float32), k, rows=[scope] * nq)
                s, i = ws.maxsim_search(idx, Q[:nq], [0, scope.size], scope, np.zeros(nq, np.int32), k)
                assert np.array_equal(i, ei) and MS.same_scores(s, es), (slab, nq, k, i.tolist(), ei.tolist())
    finally:
        ws.close()
        _pin(monkeypatch, MS.PIN_NAMES, {})


def _check_store(idx, model, Q, what):
    """scores() of 7 queries on every document (the ~2 000 sampled ones included) against the reference on g of the
    documents' source tokens."""
    info = idx.info()
    assert info[0] == model.n and info[1] == int(model.length.sum()), (what, info[:2], model.n)
    want = _ms_reference(model, Q[:7]).astype(np.float32)
    got = idx.scores(Q[:7])
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert MS.same_scores(got, want), (what, len(bad), "first wrong (query, document):", bad[:6].tolist())
    # a sample of ~2 000 documents once more, by numpy on the host, for a few of them
    few = np.unique(np.concatenate([[0, model.n - 1], list(_straddlers(model)[1].values())]).astype(np.int64))
    host = SL.ms_scores_np([model.tokens(int(d)) for d in few], Q[:7]).astype(np.float32)
    assert MS.same_scores(got[:, few], host), (what, "numpy on the host")
    return want


def test_maxsim_updates_across_the_marks(colbert):
    idx, model, Q, _ = colbert
    fresh = 1 << 25  # source tokens of new documents: g beyond the store
    # replace: the document straddling token 2^23 by a longer one, the one straddling 2^24 by a shorter one
    _, st = _straddlers(model)
    d23, d24 = st[1 << 23], st[1 << 24]
    new_len = np.array([model.length[d23] + 41, max(1, model.length[d24] // 2)], np.int64)
    new_start = np.array([fresh, fresh + 1000], np.int64)
    model.replace([d23, d24], new_start, new_len)
    toks = np.concatenate([model.tokens(d23), model.tokens(d24)])
    idx.replace([d23, d24], SL.g_np(toks).astype(np.float32), np.array([0, new_len[0], new_len.sum()], np.int64))
    assert model.length.sum() > 1 << 24
    _check_store(idx, model, Q, "after replace")
    # remove: one document before token 2^23, the documents that straddle the marks now, and a spread that takes the
    # total below token 2^24
    ptr, st = _straddlers(model)
    rem = np.unique(np.concatenate([[1000], list(st.values()), np.arange(2000, model.n, 2500)]).astype(np.int64))
    assert ptr[1001] < 1 << 23
    model.remove(rem)
    idx.remove(rem)
    assert (1 << 23) < model.length.sum() < 1 << 24
    _check_store(idx, model, Q, "after remove")
    # add: across token 2^24
    n0 = int(model.length.sum())
    lens = np.full(80, 100, np.int64)
    lens[::7] = 1
    lens[3::11] = 220
    start = fresh + 5000 + np.concatenate([[0], np.cumsum(lens)[:-1]])
    model.add(start, lens)
    toks = np.concatenate([model.tokens(d) for d in range(model.n - 80, model.n)])
    idx.add(SL.g_np(toks).astype(np.float32), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    assert n0 < 1 << 24 < int(model.length.sum())
    want = _check_store(idx, model, Q, "after add")
    es, ei = MS.topk_expected(want, 10)
    s, i = idx.search(Q[:7], 10)
    assert np.array_equal(i, ei) and MS.same_scores(s, es)

"""The closed-form stores of tests/store_limit_cases.py, checked on the host: the two write-ups of f and g agree, the
integer budgets hold, the chunked references equal dense numpy ones on a store with scaled-down marks, and the
certificates of the full-size case — evaluated by formula only, no store is built."""
import numpy as np
import pytest

import dense_adversary as DA
import maxsim_adversary as MS
import torch

import store_limit_cases as SL

# a store small enough to hold, with the three marks inside rows 85, 170 and 341 (the planted rows reach 33 rows either
# side of a mark, so a row-768 store cannot scale its marks below 2^16 elements)
SMALL = SL.Marks(SL.D_DENSE, byte_mark=1 << 18, int_mark=1 << 17, uint_mark=1 << 18)
N_SMALL = 341 + 43


def _mark_rows(n, marks):
    return SL.mark_window_rows(n, marks)


def test_numpy_and_torch_forms_agree():
    rng = np.random.default_rng(1)
    rows = np.unique(np.concatenate([rng.integers(0, SL.N_DENSE, size=300), _mark_rows(SL.N_DENSE, SL.DENSE_MARKS),
                                     [SL.N_DENSE + 10_000_000]]))
    a = SL.f_np(rows)
    b = SL.f_torch(torch, torch.from_numpy(rows)).numpy()
    assert a.dtype == np.int64 and np.array_equal(a, b)
    assert a.min() == -SL.VAL_DENSE and a.max() == SL.VAL_DENSE
    assert np.abs(np.bincount((a + 3).ravel(), minlength=7) / a.size - 1 / 7).max() < 0.01  # hash-like: every value as often
    toks = np.unique(np.concatenate([rng.integers(0, SL.T_MS, size=300), _mark_rows(SL.T_MS, SL.MS_MARKS), [1 << 25]]))
    a = SL.g_np(toks)
    assert np.array_equal(a, SL.g_torch(torch, torch.from_numpy(toks)).numpy())
    assert a.min() == -SL.VAL_MS and a.max() == SL.VAL_MS
    # a contiguous chunk, as the device fill makes it, against single rows
    lo = SL.DENSE_MARKS.row("elem2^31") - 3
    chunk = SL.f_torch(torch, torch.arange(lo, lo + 7, dtype=torch.int64)).numpy()
    assert np.array_equal(chunk, np.concatenate([SL.f_np([r]) for r in range(lo, lo + 7)]))
    # the flat view the certificates use
    e = lo * SL.D_DENSE + np.arange(7 * SL.D_DENSE)
    assert np.array_equal(SL.dense_flat_np(e, plants={}), chunk.ravel())


def test_no_short_period():
    """Rows 2^30 / 768, 2^31 / 768 and 2^32 / 768 elements apart are not equal (a periodic store would hide a wrap)."""
    rows = np.arange(0, 4000, 37)
    for shift in (1, 1_398_101, 1_398_102, 2_796_202, 2_796_203, 5_592_405, 5_592_406):
        assert not np.any(np.all(SL.f_np(rows) == SL.f_np(rows + shift), axis=1))
    for shift in (1, 1 << 23, 1 << 24, 1 << 25):
        assert not np.any(np.all(SL.g_np(rows) == SL.g_np(rows + shift), axis=1))


def test_integer_budget():
    Q = SL.dense_queries()
    rows = np.concatenate([np.array(sorted(SL.dense_plants())), np.arange(0, SL.N_DENSE, 99_991)])
    budget = DA.assert_integer_budget(SL.dense_rows_np(rows), Q)
    assert budget <= 6912
    # whatever the rows: |x| <= 3, |q| <= 3, 768 columns
    assert SL.VAL_DENSE * SL.D_DENSE * SL.VAL_DENSE == 6912 < DA.LIMIT
    assert DA.stats_finite(SL.dense_rows_np(rows))
    # every planted row is the unique best possible row of its query: 3 sum|q|
    for r, q in list(SL.dense_plants().items())[::7]:
        assert float(SL.dense_rows_np([r])[0] @ Q[q].astype(np.float64)) == 3.0 * np.abs(Q[q]).sum()
    assert SL.ms_range_certificate() == 32 * 128 * 49


def test_chunked_dense_reference_equals_dense_numpy_at_scaled_marks():
    plants = SL.dense_plants(N_SMALL, SMALL)
    X = SL.dense_rows_np(np.arange(N_SMALL), plants)
    Q = SL.dense_queries()[:35].copy()
    Xt = torch.empty((N_SMALL, SL.D_DENSE), dtype=torch.float32)
    SL.fill_dense_torch(torch, Xt, chunk=100, plants=plants)
    assert np.array_equal(Xt.numpy().astype(np.float64), X)
    for k in (10, 128):
        es, ei = DA.oracle_topk(DA.exact_scores(X, Q), k)
        for chunk in (64, 97, N_SMALL):
            s, i = SL.chunked_topk_torch(torch, lambda lo, hi: Xt[lo:hi], N_SMALL, torch.from_numpy(Q), k, chunk=chunk)
            assert np.array_equal(i, ei) and DA.bits_equal(s, es), (k, chunk)
    # the planted rows of query 0 tie, on both sides of every mark, and come in id order
    es, ei = DA.oracle_topk(DA.exact_scores(X, Q), 10)
    mine = sorted(r for r, q in plants.items() if q == 0)
    assert ei[0].tolist() == mine and len(set(es[0].tolist())) == 1
    # ... and a kernel with any of the address faults returns something else on this store
    flat = X.ravel()
    for model in SL.FAULT_MODELS:
        Xw = X.copy()
        for r in range(N_SMALL):
            e = SL.wrapped_elements(model, r, SMALL)
            Xw[r] = np.where(e == SL.OUTSIDE, 0.0, flat[np.maximum(e, 0)])
        ws, wi = DA.oracle_topk(DA.exact_scores(Xw, Q), 10)
        assert not np.array_equal(wi[:4], ei[:4]), model


def test_chunked_maxsim_reference_equals_dense_numpy_at_scaled_marks():
    T = 4096 + 301
    ptr = SL.ms_doc_ptr(T, (2048, 4096), 40, 5)
    src = SL.DocSource(ptr)
    Q = SL.ms_queries()[:3, :17].copy()
    tok, seg = src.all_tokens()
    assert np.array_equal(tok, np.arange(T))
    D = SL.g_torch(torch, torch.from_numpy(tok))
    got = SL.ms_scores_torch(torch, lambda lo, hi: D[lo:hi], torch.from_numpy(seg), src.n, torch.from_numpy(Q), chunk=777)
    want = SL.ms_scores_np([src.tokens(d) for d in range(src.n)], Q)
    assert np.array_equal(got.numpy(), want)
    assert MS.same_scores(want.astype(np.float32), MS.f32_expected(SL.g_np(tok).astype(np.float32), ptr, Q))
    assert MS.same_scores(want.astype(np.float32), MS.split_expected(SL.g_np(tok).astype(np.float32), ptr, Q))


def test_full_size_certificate_both_sides_of_every_mark():
    plants = SL.dense_plants()
    sides = SL.sides_certificate(plants, SL.DENSE_MARKS, SL.N_DENSE)
    assert set(sides) == {"byte2^32", "elem2^31", "elem2^32"}
    for m, qs in sides.items():
        assert 0 in qs and 1 in qs and len(qs) == len(SL.PLANT_QUERIES), (m, qs)  # every batch size has such a query
    rows = sorted(r for r, q in plants.items() if q == 0)
    assert len(rows) == 10 and rows[-1] == SL.N_DENSE - 1  # query 0 at k = 10: exactly its planted rows, all tied
    own = SL.dense_plants(SL.N_OWNED)
    assert set(SL.sides_certificate(own, SL.DENSE_MARKS, SL.N_OWNED)) == {"byte2^32", "elem2^31"}
    # the ColBERT store: a document straddles each mark token
    ptr = SL.ms_doc_ptr()
    assert ptr[-1] == SL.T_MS and int(np.diff(ptr).max()) <= SL.MS_MAXLEN and int(np.diff(ptr).min()) == 1
    for s in (1 << 23, 1 << 24):
        d = SL.ms_doc_of(ptr, s)
        assert ptr[d] < s < ptr[d + 1]
    # D: 512 B rows; img (hi and lo halves, 2 x 2 B x 128) the same row bytes; img_hi 256 B rows
    assert SL.T_MS * 512 > 1 << 32 and SL.T_MS * 128 > 1 << 31 and SL.T_MS * 256 > 1 << 32


@pytest.mark.parametrize("model", SL.FAULT_MODELS)
def test_full_size_certificate_wrong_addresses(model):
    """No address fault of the four models can pass: what it reads in place of each planted or checked row differs from
    the row in at least one 16-byte unit (or lies before the store)."""
    n, marks = SL.N_DENSE, SL.DENSE_MARKS
    rows = sorted(set(SL.dense_plants()) | set(SL.mark_window_rows(n, marks).tolist()) |
                  set(SL.sample_ids(n, marks.rows(n).values(), step=99_991, half=8).tolist()))
    moved, outside, least = SL.wrong_address_certificate(model, rows, marks, SL.dense_flat_np)
    first = SL.rows_past(marks, n)[model]
    assert first is not None and moved and min(moved) == first and set(moved) == {r for r in rows if r >= first}
    print(f"OBS store limit: {model}: {len(moved)} rows moved, {len(outside)} before the store, >= {least} of 192 units differ")
    assert least >= 1, (model, least)  # (in fact a third of a row or more: 73 units where a planted row lands on another)
    if model != SL.FAULT_MODELS[1]:
        assert not outside
    # the owned index of the update tests reaches the first two faults
    own_rows = sorted(set(SL.mark_window_rows(SL.N_OWNED, marks).tolist()))
    first = SL.rows_past(marks, SL.N_OWNED)[model]
    moved, _, _ = SL.wrong_address_certificate(model, own_rows, marks, lambda e: SL.dense_flat_np(e, SL.N_OWNED, {}))
    assert (first is None and not moved) or (moved and min(moved) == first)
    # the ColBERT token rows: fp32 rows of 128 and the 2-byte rows of the images
    for ms_marks in (SL.MS_MARKS, SL.Marks(SL.DIM_MS, elem=2), SL.Marks(2 * SL.DIM_MS, elem=2)):
        toks = sorted(set(SL.mark_window_rows(SL.T_MS, SL.MS_MARKS).tolist()) | {SL.T_MS - 1, (1 << 24) + 1500})
        flat = SL.ms_flat_np if ms_marks.width == SL.DIM_MS else (lambda e: SL.ms_flat_np(e // 2))  # (hi, lo pairs: by token)
        moved, _, _ = SL.wrong_address_certificate(model, toks, ms_marks, flat, unit=16 // ms_marks.elem)
        first = SL.rows_past(ms_marks, SL.T_MS)[model]
        assert (first is None and not moved) or (moved and min(moved) == first), (model, ms_marks.elem)


def test_update_models_follow_the_rules():
    src = SL.RowSource(40)
    old = src.remove([0, 3, 4, 39])
    assert old.tolist() == [r for r in range(40) if r not in (0, 3, 4, 39)] and np.array_equal(src.src, old)
    src.replace([1, 2], src=[100, 0], extra=[None, np.ones(SL.D_DENSE)])
    src.add([500, 501])
    X = src.rows(np.arange(src.n))
    assert np.array_equal(X[0], SL.f_np([1])[0]) and np.array_equal(X[1], SL.f_np([100])[0]) and np.all(X[2] == 1)
    assert np.array_equal(X[-1], SL.f_np([501])[0]) and src.n == 38
    ids = SL.sample_ids(SL.N_OWNED, [SL.DENSE_MARKS.row("byte2^32")])
    assert 10_000 < ids.size < 12_000 and ids[0] == 0 and ids[-1] == SL.N_OWNED - 1
    docs = SL.DocSource(np.array([0, 3, 5, 9]))
    docs.replace([1], 100, 7)
    docs.remove([0])
    docs.add([50], [2])
    tok, seg = docs.all_tokens()
    assert tok.tolist() == list(range(100, 107)) + [5, 6, 7, 8, 50, 51] and seg.tolist() == [0] * 7 + [1] * 4 + [2] * 2

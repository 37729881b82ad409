"""amdr_maxsim_add: after any sequence of adds a MaxSim handle is what amdr_maxsim_create makes of the concatenated
store — the same scale and images, hence the same ids and score BITS from every entry point and on every route
(csrc/maxsim_store.hip).  `grown` is created from the first part and added to, `fresh` from the concatenation."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LENS = (1, 31, 32, 33, 63, 64, 65, 220)  # the 32- and 64-token tile edges of img / img_hi
PINS = (None, "AMDR_MAXSIM_F16X3", "AMDR_MAXSIM_TWOPASS")
SEARCHES = ((1, 1), (7, 10), (8, 10), (9, 10), (24, 1))  # (nq, k)


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


def unit_rows(rng, n, d=128):
    X = rng.standard_normal((n, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X


def part(rng, n_docs):
    """(token rows, doc_ptr from 0): lengths from LENS, the last document 33 tokens (its last tile reads the padding)."""
    lens = rng.choice(LENS, size=n_docs)
    lens[-1] = 33
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return unit_rows(rng, int(ptr[-1])), ptr


def concat(parts):
    ptr = [np.zeros(1, np.int64)]
    for _, p in parts:
        ptr.append(p[1:] + ptr[-1][-1])
    return np.concatenate([d for d, _ in parts]), np.concatenate(ptr)


def fresh(nat, parts):
    return nat.MaxSimIndex(*concat(parts))


def grown(nat, parts):
    idx = nat.MaxSimIndex(*parts[0])
    for d, p in parts[1:]:
        idx.add(d, p)
    return idx


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def results(idx, Q):
    """Every host entry point's output: scores for 1 and 9 queries, the searches of SEARCHES."""
    out = [idx.scores(Q[:nq]) for nq in (1, 9)]
    for nq, k in SEARCHES:
        out.extend(idx.search(Q[:nq], k))
    return out


def assert_same(nat, monkeypatch, g, f, Q, seam=None):
    """The equality check: info()[0, 1, 3, 4] and the bits of (d_scale, d_norm_max), then scores and searches unpinned, under AMDR_MAXSIM_F16X3=0 and under
    AMDR_MAXSIM_TWOPASS=0, then (stores with images) one scoped search whose scope holds rows of both sides of `seam`."""
    gi, fi = g.info(), f.info()
    assert [gi[j] for j in (0, 1, 3, 4)] == [fi[j] for j in (0, 1, 3, 4)], (gi, fi)
    assert g.n_docs == f.n_docs == gi[0]
    assert bits(g.stats()).tolist() == bits(f.stats()).tolist(), (g.stats(), f.stats())  # d_scale, d_norm_max
    for pin in PINS:
        if pin:
            monkeypatch.setenv(pin, "0")
        a, b = results(g, Q), results(f, Q)
        if pin:
            monkeypatch.delenv(pin)
        for j, (x, y) in enumerate(zip(a, b)):
            if x.dtype == np.int64:
                assert np.array_equal(x, y), (pin, j)
            else:
                assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), (pin, j)
    if seam is not None and gi[4]:
        n = gi[0]
        rows = np.asarray(sorted({0, seam - 2, seam - 1, seam, min(seam + 1, n - 1), n - 1}), dtype=np.int64)
        ws = nat.ScopeWorkspace()
        (gs, gid), (fs, fid) = (ws.maxsim_search(h, Q[:3], [0, rows.size], rows, [0, 0, 0], 4) for h in (g, f))
        ws.close()
        assert np.array_equal(gid, fid) and np.array_equal(bits(gs), bits(fs))
        assert set(gid[0].tolist()) <= set(rows.tolist()) and gid[0].min() >= 0


@pytest.fixture(scope="module")
def queries():
    return unit_rows(np.random.default_rng(11), 24 * 32).reshape(24, 32, 128)


@pytest.fixture(scope="module")
def case1():
    """30 documents, + 12 in one add, + 1 five times."""
    rng = np.random.default_rng(2027)
    return [part(rng, 30), part(rng, 12)] + [part(rng, 1) for _ in range(5)]


def test_plain_adds_convert_only_the_new_rows(nat, monkeypatch, queries, case1):
    g = nat.MaxSimIndex(*case1[0])
    t0 = int(case1[0][1][-1])
    assert g.info() == (30, t0, t0, g.info()[3], 1, 1)
    g.add(*case1[1])
    cap = g.info()[2]
    assert cap >= 2 * t0 > t0 and g.info()[5] == 1  # the capacity doubled; no whole-store conversion
    f = fresh(nat, case1[:2])
    assert_same(nat, monkeypatch, g, f, queries, seam=30)
    f.close()
    for p in case1[2:]:
        g.add(*p)
        assert g.info()[2] == cap and g.info()[5] == 1  # these fit
    f = fresh(nat, case1)
    assert g.info()[:2] == (47, int(concat(case1)[1][-1]))
    assert_same(nat, monkeypatch, g, f, queries, seam=42)
    g.add(np.zeros((0, 128), np.float32), np.zeros(1, np.int64))  # n_add == 0: a no-op
    assert_same(nat, monkeypatch, g, f, queries)
    g.close()
    f.close()


def test_an_add_grows_the_document_table_alone(nat, monkeypatch, queries):
    """Many one-token documents behind a few long ones: doc_ptr has no room for them while D and the images have (the
    first add doubled 880 token rows to 1 760 and 4 documents to 8).  Then an add that fits both."""
    rng = np.random.default_rng(2028)

    def docs(lens):
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        return unit_rows(rng, int(ptr[-1])), ptr

    parts = [docs([220] * 4), docs([220, 220]), docs([1] * 40), docs([1])]
    g = nat.MaxSimIndex(*parts[0])
    g.add(*parts[1])
    assert g.info()[:3] == (6, 1320, 1760) and g.info()[5] == 1
    g.add(*parts[2])  # 46 documents > 8, 1 360 token rows <= 1 760
    assert g.info()[:3] == (46, 1360, 1760) and g.info()[5] == 1
    f = fresh(nat, parts[:3])
    assert_same(nat, monkeypatch, g, f, queries, seam=6)
    f.close()
    g.add(*parts[3])  # 47 documents <= 2 x 46
    assert g.info()[:3] == (47, 1361, 1760) and g.info()[5] == 1
    f = fresh(nat, parts)
    assert_same(nat, monkeypatch, g, f, queries, seam=46)
    d, p = g.read()
    assert np.array_equal(bits(d), bits(concat(parts)[0])) and np.array_equal(p, concat(parts)[1])
    g.close()
    f.close()


def test_the_first_pass_bound_follows_the_largest_token_norm(nat, monkeypatch, queries):
    """d_norm_max = max(old, new rows) at an unchanged scale, wherever the longest token sits: in an added row (the bound
    rises with the add), then in none of a further add's (it stays)."""
    rng = np.random.default_rng(12)
    base, longer, plain = part(rng, 30), part(rng, 3), part(rng, 3)
    longer[0][9] *= np.float32(1.2)  # the longest token of the store, its components still inside the store's exponent
    assert float(np.abs(base[0]).max()) >= 0.25 and max(float(np.abs(p[0]).max()) for p in (base, longer, plain)) < 0.5
    g = nat.MaxSimIndex(*base)
    scale, n0 = g.stats()
    assert scale == 2.0 and 1.999 < n0 < 2.001  # unit rows x 2^1
    g.add(*longer)
    n1 = g.stats()[1]
    assert g.stats()[0] == scale and g.info()[5] == 1 and 2.399 < n1 < 2.401
    f = fresh(nat, [base, longer])
    assert_same(nat, monkeypatch, g, f, queries, seam=30)
    f.close()
    g.add(*plain)
    assert g.stats() == (scale, n1) and g.info()[5] == 1
    f = fresh(nat, [base, longer, plain])
    assert_same(nat, monkeypatch, g, f, queries, seam=33)
    g.close()
    f.close()


def test_an_add_that_crosses_the_two_pass_threshold(nat, monkeypatch, queries):
    """39 documents at k = 10, 8 queries: one pass (4 k > n_docs); one more document: two passes."""
    rng = np.random.default_rng(39)
    parts = [part(rng, 39), part(rng, 1)]
    rows = lambda n: (8 * n * 4 + 255) // 256 * 256  # noqa: E731
    assert nat.maxsim_workspace_plan(39, True, 8, 10, 8, 10)[1] == rows(39)    # the one-pass score rows alone
    assert nat.maxsim_workspace_plan(40, True, 8, 10, 8, 10)[1] > 3 * rows(40)  # the two-pass layout
    g, f = nat.MaxSimIndex(*parts[0]), fresh(nat, parts[:1])
    assert "maxsim_hi2_ring_kernel" in g.plan_info(8) and g.info()[0] == 39
    assert_same(nat, monkeypatch, g, f, queries)
    f.close()
    g.add(*parts[1])
    f = fresh(nat, parts)
    assert g.info()[0] == 40
    assert_same(nat, monkeypatch, g, f, queries, seam=39)
    g.close()
    f.close()


def test_an_add_that_raises_the_scale_converts_the_store_again(nat, monkeypatch, queries):
    rng = np.random.default_rng(5)
    base, big, plain = part(rng, 30), part(rng, 3), part(rng, 4)
    absmax = float(np.abs(base[0]).max())
    assert 2 * absmax < 0.95  # the new component is more than twice the store's largest: the exponent rises
    v = unit_rows(rng, 1)[0]
    v[7] = 0.0
    v *= np.float32(np.sqrt(1 - 0.95 ** 2)) / np.linalg.norm(v)
    v[7] = 0.95
    big[0][5] = v
    g = nat.MaxSimIndex(*base)
    e0 = g.info()[3]
    g.add(*big)
    assert g.info()[3] != e0 and g.info()[3] == 0 and g.info()[5] == 2  # 0.95 = 0.95 * 2^0: d_scale = 2^0
    f = fresh(nat, [base, big])
    assert f.info()[5] == 1
    assert_same(nat, monkeypatch, g, f, queries, seam=30)
    f.close()
    g.add(*plain)
    assert g.info()[5] == 2
    f = fresh(nat, [base, big, plain])
    assert_same(nat, monkeypatch, g, f, queries, seam=33)
    g.close()
    f.close()


def test_a_non_finite_add_drops_the_images(nat, monkeypatch, queries):
    rng = np.random.default_rng(6)
    base, bad, more = part(rng, 30), part(rng, 3), part(rng, 4)
    bad[0][5, 17] = np.nan
    g = nat.MaxSimIndex(*base)
    assert g.info()[4] == 1
    g.add(*bad)
    assert g.info()[4] == 0
    f = fresh(nat, [base, bad])
    assert f.info()[4] == 0 and "fp32-input" in g.plan_info(8)
    assert_same(nat, monkeypatch, g, f, queries)
    f.close()
    g.add(*more)
    assert g.info()[4] == 0
    f = fresh(nat, [base, bad, more])
    assert_same(nat, monkeypatch, g, f, queries)
    g.close()
    f.close()


def test_bad_arguments_leave_the_handle_as_it_was(nat, queries):
    rng = np.random.default_rng(7)
    base, add = part(rng, 30), part(rng, 2)
    g = nat.MaxSimIndex(*base)
    before = (g.info(), g.search(queries[:9], 10))
    lib = nat.load()
    D = np.ascontiguousarray(add[0])
    fp, lp = C.POINTER(C.c_float), C.POINTER(C.c_int64)

    def raw(h, d, ptr, n):
        ptr = None if ptr is None else np.ascontiguousarray(ptr, dtype=np.int64)
        nat._check(lib.amdr_maxsim_add(h, None if d is None else d.ctypes.data_as(fp),
                                       None if ptr is None else ptr.ctypes.data_as(lp), C.c_int64(n)), "amdr_maxsim_add")

    ok = add[1]
    empty = np.array([0, 33, 33], np.int64)
    for args in ((None, D, ok, 2), (g._h, D, ok, -1), (g._h, None, ok, 2), (g._h, D, None, 2),
                 (g._h, D, ok + 1, 2), (g._h, D, empty, 2), (g._h, D, ok[::-1].copy(), 2), (g._h, D, ok, (1 << 32) - 30)):
        with pytest.raises(nat.NativeError, match="status -1"):
            raw(*args)
        after = (g.info(), g.search(queries[:9], 10))
        assert after[0] == before[0] and np.array_equal(after[1][1], before[1][1])
        assert np.array_equal(bits(after[1][0]), bits(before[1][0]))
    with pytest.raises(ValueError):
        g.add(D[:, :64], ok)
    with pytest.raises(ValueError):
        g.add(D[:-1], ok)
    raw(g._h, None, None, 0)  # n_add == 0: a no-op whatever the pointers
    assert g.info() == before[0]
    g.close()


def test_grown_store_against_the_fp64_oracle(nat, queries, case1):
    """Ranks are pinned by the equality with `fresh` above; here the scores themselves: every reported score within
    1e-4 (the project's bar) of the oracle's score of the reported id."""
    from oracle import maxsim as OM
    D, ptr = concat(case1)
    ref = OM.maxsim_scores(queries[:9], D, ptr)
    g = grown(nat, case1)
    s, i = g.search(queries[:9], 10)
    full = g.scores(queries[:9])
    g.close()
    assert i.min() >= 0 and i.max() < 47 and all(len(set(r.tolist())) == 10 for r in i)
    err = np.abs(s - np.take_along_axis(ref, i, axis=1)).max()
    print(f"max |score - oracle| over the reported ids: {err:.3e}; over all documents: {np.abs(full - ref).max():.3e}")
    assert err <= 1e-4
    assert np.abs(full - ref).max() <= 1e-4


def test_device_calls_after_an_add(nat, queries):
    """A "_device" call after an add without a new reserve grows its workspace (visible in amdr_workspace_growths) and
    returns what a fresh handle returns; after a new reserve a call allocates nothing."""
    rng = np.random.default_rng(8)
    parts = [part(rng, 40), part(rng, 30)]
    nq, k = 8, 10
    g = nat.MaxSimIndex(*parts[0])
    stream = torch.cuda.Stream(device=DEV)
    Qd = torch.from_numpy(queries[:nq]).to(DEV)
    s = torch.empty((nq, k), dtype=torch.float32, device=DEV)
    i = torch.empty((nq, k), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()

    def call():
        g.search_device(Qd.data_ptr(), nq, 32, k, s.data_ptr(), i.data_ptr(), int(stream.cuda_stream))
        stream.synchronize()  # (also what orders this work before the add below)
        return s.cpu().numpy(), i.cpu().numpy()

    g.reserve(nq, k)
    g0 = nat.workspace_growths()
    s0, i0 = call()
    assert nat.workspace_growths() == g0
    f = fresh(nat, parts[:1])
    es, ei = f.search(queries[:nq], k)
    f.close()
    assert np.array_equal(i0, ei) and np.array_equal(bits(s0), bits(es))
    g.add(*parts[1])
    s1, i1 = call()  # not re-reserved: the call sizes its workspace for 70 documents
    assert nat.workspace_growths() > g0
    f = fresh(nat, parts)
    es, ei = f.search(queries[:nq], k)
    f.close()
    assert np.array_equal(i1, ei) and np.array_equal(bits(s1), bits(es))
    g.reserve(nq, k)
    g1 = nat.workspace_growths()
    s2, i2 = call()
    assert nat.workspace_growths() == g1
    assert np.array_equal(i2, ei) and np.array_equal(bits(s2), bits(es))
    g.close()

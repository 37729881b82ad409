"""amdr_maxsim_remove: after a remove a MaxSim handle is what amdr_maxsim_create makes of the surviving store — D and
doc_ptr the same bytes, the scale, the first-pass bound and the images made again from the new D, hence the same ids and
score BITS from every entry point and on every route (csrc/maxsim_store.hip, csrc/rows_compact.hip).  `removed` is created from
the whole store and removed from, `fresh` from the survivors filtered on the host.  The helpers are those of
tests/test_maxsim_add_gpu.py, restated."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENS = (1, 31, 32, 33, 63, 64, 65, 220)  # the 32- and 64-token tile edges of img / img_hi
PINS = (None, "AMDR_MAXSIM_F16X3", "AMDR_MAXSIM_TWOPASS")
SEARCHES = ((1, 1), (7, 10), (8, 10), (9, 10), (24, 1))  # (nq, k)
N_DOCS = 40
PATTERNS = {
    "first": [0],
    "last": [N_DOCS - 1],  # the new last document's last tile reads the zero padding behind the new end
    "one adjacent run": list(range(13, 18)),
    "alternating": list(range(1, N_DOCS, 2)),
    "all but one": [i for i in range(N_DOCS) if i != 20],
    "a single id": [20],
}


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


def survivors(store, ids):
    """The plain filter on the host: the store without documents `ids`."""
    D, ptr = store
    keep = [j for j in range(ptr.shape[0] - 1) if j not in set(int(i) for i in ids)]
    lens = [int(ptr[j + 1] - ptr[j]) for j in keep]
    rows = np.concatenate([np.arange(ptr[j], ptr[j + 1]) for j in keep])
    return np.ascontiguousarray(D[rows]), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def results(idx, Q):
    """Every host entry point's output: scores for 1 and 9 queries, the searches of SEARCHES."""
    out = [idx.scores(Q[:nq]) for nq in (1, 9)]
    for nq, k in SEARCHES:
        out.extend(idx.search(Q[:nq], k))
    return out


def assert_same(nat, monkeypatch, g, f, Q, seam=None):
    """The equality check: info()[0, 1, 3, 4], the bits of (d_scale, d_norm_max) and of the resident D and doc_ptr, then
    scores and searches unpinned, under AMDR_MAXSIM_F16X3=0 and under AMDR_MAXSIM_TWOPASS=0, then (stores with images) one
    scoped search whose scope holds documents of both sides of `seam`."""
    gi, fi = g.info(), f.info()
    assert [gi[j] for j in (0, 1, 3, 4)] == [fi[j] for j in (0, 1, 3, 4)], (gi, fi)
    assert g.n_docs == f.n_docs == gi[0]
    assert bits(g.stats()).tolist() == bits(f.stats()).tolist(), (g.stats(), f.stats())  # d_scale, d_norm_max
    (gd, gp), (fd, fp) = g.read(), f.read()
    assert gd.shape == fd.shape and np.array_equal(bits(gd), bits(fd))
    assert np.array_equal(gp, fp)
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
    if seam is not None and gi[4] and gi[0] >= 3:
        n = gi[0]
        seam = min(max(seam, 2), n - 1)
        rows = np.asarray(sorted({0, seam - 2, seam - 1, seam, min(seam + 1, n - 1), n - 1}), dtype=np.int64)
        ws = nat.ScopeWorkspace()
        (gs, gid), (fs, fid) = (ws.maxsim_search(h, Q[:3], [0, rows.size], rows, [0, 0, 0], min(4, rows.size)) for h in (g, f))
        ws.close()
        assert np.array_equal(gid, fid) and np.array_equal(bits(gs), bits(fs))
        assert set(gid[0].tolist()) <= set(rows.tolist()) and gid[0].min() >= 0


@pytest.fixture(scope="module")
def queries():
    return unit_rows(np.random.default_rng(11), 24 * 32).reshape(24, 32, 128)


@pytest.fixture(scope="module")
def base():
    store = part(np.random.default_rng(2031), N_DOCS)
    store[0].setflags(write=False)
    store[1].setflags(write=False)
    return store


def removed_and_fresh(nat, store, ids):
    g = nat.MaxSimIndex(*store)
    g.remove(ids)
    return g, nat.MaxSimIndex(*survivors(store, ids))


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_removal_patterns(nat, monkeypatch, queries, base, pattern):
    ids = PATTERNS[pattern]
    g = nat.MaxSimIndex(*base)
    assert g.remove_kernel_ms() == -1.0 and g.info()[5] == 1
    g.remove(ids)
    f = nat.MaxSimIndex(*survivors(base, ids))
    info = g.info()
    assert info[0] == N_DOCS - len(ids) and info[2] == info[1] == f.info()[1]  # capacity = the survivors
    assert info[5] == 2 and g.remove_kernel_ms() >= 0.0  # one more whole-store conversion
    assert_same(nat, monkeypatch, g, f, queries, seam=ids[0])  # the scope straddles the first gap
    g.close()
    f.close()


def unit_store_with(rng, doc, row):
    """40 documents of unit rows, one token of document `doc` replaced by `row`; returns (store, that document)."""
    D, ptr = part(rng, N_DOCS)
    D[int(ptr[doc]) + (int(ptr[doc + 1] - ptr[doc]) // 2)] = row
    return (D, ptr)


def test_the_scale_falls_with_the_largest_component(nat, monkeypatch, queries):
    rng = np.random.default_rng(41)
    row = np.zeros(128, np.float32)
    row[7] = 3.0
    store = unit_store_with(rng, 17, row)
    g = nat.MaxSimIndex(*store)
    assert g.info()[3] == -2  # 3.0 = 0.75 * 2^2: d_scale = 2^-2
    g.remove([17])
    f = nat.MaxSimIndex(*survivors(store, [17]))
    assert g.info()[3] == f.info()[3] == 1  # unit rows, largest component in [0.25, 0.5): d_scale = 2^1
    assert_same(nat, monkeypatch, g, f, queries, seam=17)
    g.close()
    f.close()


def test_the_first_pass_bound_falls_with_the_largest_token_norm(nat, monkeypatch, queries):
    rng = np.random.default_rng(42)
    D, ptr = part(rng, N_DOCS)
    t = int(ptr[9]) + 3 if ptr[10] - ptr[9] > 3 else int(ptr[9])
    D[t] *= np.float32(1.2)  # the longest token of the store, its components still inside the store's exponent
    assert 0.25 <= float(np.abs(D).max()) < 0.5
    g = nat.MaxSimIndex(D, ptr)
    scale, n0 = g.stats()
    assert scale == 2.0 and 2.399 < n0 < 2.401
    g.remove([9])
    f = nat.MaxSimIndex(*survivors((D, ptr), [9]))
    assert g.stats()[0] == 2.0 and 1.999 < g.stats()[1] < 2.001
    assert bits(g.stats()).tolist() == bits(f.stats()).tolist()
    assert_same(nat, monkeypatch, g, f, queries, seam=9)
    g.close()
    f.close()


def test_removing_the_only_nan_brings_the_images(nat, monkeypatch, queries):
    rng = np.random.default_rng(43)
    D, ptr = part(rng, N_DOCS)
    D[int(ptr[5]), 17] = np.nan
    g = nat.MaxSimIndex(D, ptr)
    assert g.info()[4] == 0 and g.info()[5] == 0 and "fp32-input" in g.plan_info(8)
    g.remove([30])  # the NaN stays: still no images, no conversion
    f = nat.MaxSimIndex(*survivors((D, ptr), [30]))
    assert g.info()[4] == 0 and g.info()[5] == 0
    assert_same(nat, monkeypatch, g, f, queries)
    f.close()
    g.remove([5])
    f = nat.MaxSimIndex(*survivors((D, ptr), [5, 30]))
    assert g.info()[4] == 1 and f.info()[4] == 1 and g.info()[5] == 1
    assert_same(nat, monkeypatch, g, f, queries, seam=5)
    g.close()
    f.close()


def test_add_remove_add_against_fresh(nat, monkeypatch, queries, base):
    rng = np.random.default_rng(44)
    a, b = part(rng, 7), part(rng, 3)
    g = nat.MaxSimIndex(*base)
    g.add(*a)
    whole = concat([base, a])
    ids = [0, 38, 39, 40, 46]  # across the seam of the add, its last document too
    g.remove(ids)
    left = survivors(whole, ids)
    f = nat.MaxSimIndex(*left)
    assert_same(nat, monkeypatch, g, f, queries, seam=37)
    f.close()
    g.add(*b)
    f = nat.MaxSimIndex(*concat([left, b]))
    assert g.info()[0] == N_DOCS + 7 - 5 + 3
    assert_same(nat, monkeypatch, g, f, queries, seam=42)
    g.close()
    f.close()


def test_bad_arguments_leave_the_handle_as_it_was(nat, queries, base):
    g = nat.MaxSimIndex(*base)
    before = (g.info(), g.stats(), g.search(queries[:9], 10))
    lib = nat.load()
    lp = C.POINTER(C.c_int64)

    def raw(h, ids, n):
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
        nat._check(lib.amdr_maxsim_remove(h, None if ids is None else ids.ctypes.data_as(lp), C.c_int64(n)),
                   "amdr_maxsim_remove")

    ok = [1, 3]
    for args in ((None, ok, 2), (g._h, ok, -1), (g._h, None, 2), (g._h, [1, N_DOCS], 2), (g._h, [-1, 3], 2),
                 (g._h, [3, 1], 2), (g._h, [3, 3], 2), (g._h, list(range(N_DOCS)), N_DOCS)):
        with pytest.raises(nat.NativeError, match="status -1"):
            raw(*args)
        after = (g.info(), g.stats(), g.search(queries[:9], 10))
        assert after[0] == before[0] and after[1] == before[1] and np.array_equal(after[2][1], before[2][1])
        assert np.array_equal(bits(after[2][0]), bits(before[2][0]))
    raw(g._h, None, 0)  # n_remove == 0: a no-op that reads nothing
    assert g.info() == before[0] and g.remove_kernel_ms() == -1.0
    g.close()

"""amdr_dense_remove: after a remove a dense handle is what amdr_dense_create makes of the surviving rows — the same
matrix bytes, the fp16 statistics taken again from zero, a present image made again — hence the same ids and score BITS
from every entry point (csrc/dense.hip, csrc/rows_compact.hip).  `removed` is created from the whole matrix and removed
from, `fresh` from the survivors filtered on the host."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEARCHES = ((1, 1), (4, 10), (9, 10), (33, 32))  # (nq, k)
# (n, d): 16-byte rows (2 048 of them a slab), 512-byte rows, 4 096-byte rows (8 a slab), and fewer rows than one slab
SHAPES = ((300, 4), (300, 128), (300, 1024), (37, 128))


def patterns(n):
    return {
        "first": [0],
        "last": [n - 1],
        "one adjacent run": list(range(n // 3, n // 3 + 5)),
        "alternating": list(range(1, n, 2)),
        "all but one": [i for i in range(n) if i != n // 2],
        "a single id": [n // 2],
    }


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


def unit_rows(rng, n, d):
    X = rng.standard_normal((n, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X


def survivors(X, ids):
    keep = np.ones(X.shape[0], dtype=bool)
    keep[np.asarray(ids, dtype=np.int64)] = False
    return np.ascontiguousarray(X[keep])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(g, f, Q, X_left):
    """ntotal, the resident bytes, every search of SEARCHES (ids and score bits) and score_rows bits."""
    n = X_left.shape[0]
    assert g.ntotal == f.ntotal == n
    if n:
        assert np.array_equal(bits(g.read_rows(0, n)), bits(X_left))
        assert np.array_equal(bits(f.read_rows(0, n)), bits(X_left))
    for nq, k in SEARCHES:
        (gs, gi), (fs, fi) = g.search(Q[:nq], k), f.search(Q[:nq], k)
        assert np.array_equal(gi, fi), (nq, k)
        assert np.array_equal(bits(gs), bits(fs)), (nq, k)
    if n == 0:
        return
    rows = np.tile(np.asarray([0, n - 1, n // 2, n, -1, max(n - 2, 0)], dtype=np.int64), (5, 1))
    assert np.array_equal(bits(g.score_rows(Q[:5], rows)), bits(f.score_rows(Q[:5], rows)))


@pytest.mark.parametrize("n, d", SHAPES)
def test_removal_patterns(nat, n, d):
    rng = np.random.default_rng(1000 * n + d)
    X, Q = unit_rows(rng, n, d), unit_rows(rng, 33, d)
    for what, ids in patterns(n).items():
        g = nat.DenseIndex(X)
        assert g.remove_kernel_ms() == -1.0
        g.remove(ids)
        assert g.remove_kernel_ms() >= 0.0, what
        left = survivors(X, ids)
        f = nat.DenseIndex(left)
        assert_same(g, f, Q, left)
        g.close()
        f.close()


def test_the_statistics_are_taken_again_and_the_image_follows(nat):
    """One row holds a component 8x the others': while it is resident the image's scale is set by it; removing it must
    bring the scale a fresh handle's image has, over all the surviving rows."""
    rng = np.random.default_rng(51)
    n, d = 300, 128
    X, Q = unit_rows(rng, n, d), unit_rows(rng, 33, d)
    top = int(np.abs(X).max(axis=1).argmax())  # the row of the largest component; 8x a copy of it into another row
    big = 50 if top != 50 else 51
    X[big] = np.float32(8.0) * X[top]
    g = nat.DenseIndex(X)
    g.build_image()
    e_before = g.image_info()[3]
    g.remove([big])
    left = survivors(X, [big])
    f = nat.DenseIndex(left)
    f.build_image()
    present, _, covered, e = g.image_info()
    assert present and covered == n - 1
    assert e == f.image_info()[3] and e == e_before - 3, (e_before, e, f.image_info())
    assert_same(g, f, Q, left)
    g.close()
    f.close()


def test_the_two_pass_short_corpus_form_reads_the_new_statistics(nat):
    rng = np.random.default_rng(52)
    n, d, nq, k = 200, 128, 4096, 10
    X, Q = unit_rows(rng, n, d), unit_rows(rng, nq, d)
    X[50] *= np.float32(8.0)
    g = nat.DenseIndex(X)
    assert "dsh_scores_kernel" in g.plan_info(nq, k)
    s0, i0 = g.search(Q, k)  # makes the short-corpus fp16 image of the old matrix
    f0 = nat.DenseIndex(X)
    fs, fi = f0.search(Q, k)
    f0.close()
    assert np.array_equal(i0, fi) and np.array_equal(bits(s0), bits(fs))
    g.remove([50])
    f = nat.DenseIndex(survivors(X, [50]))
    assert "dsh_scores_kernel" in g.plan_info(nq, k)
    (gs, gi), (fs, fi) = g.search(Q, k), f.search(Q, k)
    assert np.array_equal(gi, fi) and np.array_equal(bits(gs), bits(fs))
    g.close()
    f.close()


def test_remove_add_remove_against_fresh(nat):
    rng = np.random.default_rng(53)
    n, d = 300, 128
    X, more, Q = unit_rows(rng, n, d), unit_rows(rng, 40, d), unit_rows(rng, 33, d)
    g = nat.DenseIndex(X)
    g.remove([0, 7, 8, 299])
    rows = survivors(X, [0, 7, 8, 299])
    g.add(more)  # grows from a capacity equal to the survivors
    rows = np.concatenate([rows, more])
    ids = [5, 295, 296, 335]  # old rows, the seam of the add, the last row
    g.remove(ids)
    rows = survivors(rows, ids)
    f = nat.DenseIndex(rows)
    assert_same(g, f, Q, rows)
    g.close()
    f.close()


@pytest.mark.parametrize("with_image", (False, True))
def test_adds_that_grow_the_matrix_on_their_own(nat, with_image):
    """A created matrix has no spare rows: one row forces a growth (33 -> 66), 40 more force the next (74 > 66 -> 132), one
    more fits.  After each add the resident bytes and the searches are those of a fresh handle of the concatenation, and
    a resident fp16 image covers every row."""
    rng = np.random.default_rng(56)
    n, d, nq, k = 33, 128, 3, 5
    rows, Q = unit_rows(rng, n, d), unit_rows(rng, nq, d)
    g = nat.DenseIndex(rows)
    if with_image:
        g.build_image()
    for n_add in (1, 40, 1):
        more = unit_rows(rng, n_add, d)
        g.add(more)
        rows = np.concatenate([rows, more])
        ntotal = rows.shape[0]
        assert g.ntotal == ntotal and np.array_equal(bits(g.read_rows(0, ntotal)), bits(rows))
        f = nat.DenseIndex(rows)
        (gs, gi), (fs, fi) = g.search(Q, k), f.search(Q, k)
        assert np.array_equal(gi, fi) and np.array_equal(bits(gs), bits(fs)), n_add
        f.close()
        if with_image:
            assert g.image_info()[0] and g.image_info()[2] == ntotal, n_add
    g.close()


def test_removing_everything_leaves_the_empty_index(nat):
    rng = np.random.default_rng(54)
    n, d = 300, 128
    X, Q = unit_rows(rng, n, d), unit_rows(rng, 33, d)
    g = nat.DenseIndex(X)
    g.build_image()
    g.remove(np.arange(n))
    assert g.ntotal == 0 and g.image_info() == (False, 0, 0, 0)
    f = nat.DenseIndex(dim=d)
    assert_same(g, f, Q, X[:0])
    s, i = g.search(Q[:4], 10)
    assert (i == -1).all() and (s == np.float32(-3.4028234663852886e38)).all()
    f.close()
    g.add(X[:64])
    f = nat.DenseIndex(X[:64])
    assert_same(g, f, Q, X[:64])
    g.close()
    f.close()


def test_bad_arguments_leave_the_handle_as_it_was(nat):
    rng = np.random.default_rng(55)
    n, d = 300, 128
    X = unit_rows(rng, n, d)
    g = nat.DenseIndex(X)
    lib = nat.load()
    lp = C.POINTER(C.c_int64)

    def raw(h, ids, cnt):
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
        nat._check(lib.amdr_dense_remove(h, None if ids is None else ids.ctypes.data_as(lp), C.c_int64(cnt)),
                   "amdr_dense_remove")

    Xd = torch.from_numpy(X).to(DEV)
    torch.cuda.synchronize()
    wrapped = nat.DenseIndex(device_ptr=Xd.data_ptr(), n=n, dim=d, keepalive=Xd)
    ok = [1, 3]
    for h, ids, cnt in ((None, ok, 2), (g, ok, -1), (g, None, 2), (g, [1, n], 2), (g, [-1, 3], 2), (g, [3, 1], 2),
                        (g, [3, 3], 2), (wrapped, ok, 2)):
        with pytest.raises(nat.NativeError, match="status -1"):
            raw(None if h is None else h._h, ids, cnt)
        for idx in (g, wrapped):
            assert idx.ntotal == n and np.array_equal(bits(idx.read_rows(0, n)), bits(X))
    raw(g._h, None, 0)  # n_remove == 0: a no-op that reads nothing
    assert g.ntotal == n and g.remove_kernel_ms() == -1.0
    g.close()
    wrapped.close()

"""amdr_dense_replace: after a replace a dense handle is what amdr_dense_create makes of the edited matrix — the same
matrix bytes, the fp16 statistics taken again from zero, a present image kept current — hence the same ids and score BITS
from every entry point (csrc/dense.hip, csrc/rows_compact.hip).  `g` is created from the whole matrix and replaced in,
`f` from the matrix edited on the host."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_dense_remove_gpu import SEARCHES, assert_same, bits, nat, unit_rows  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NS = (31, 32, 33, 65, 1025)
DS = (4, 128, 768)


def patterns(n):
    """Rows 0 and n - 1, both sides of every 32-row tile edge, one adjacent run, every row."""
    edges = sorted({r for e in range(32, n, 32) for r in (e - 1, e)} | ({31} if n > 31 else set()))
    return {
        "first": [0],
        "last": [n - 1],
        "first and last": [0, n - 1],
        "tile edges": [r for r in edges if r < n],
        "one adjacent run": list(range(n // 3, n // 3 + 5)),
        "every row": list(range(n)),
    }


def edited(X, ids, R):
    out = X.copy()
    out[np.asarray(ids, dtype=np.int64)] = R
    return out


def device_search(idx, Q, k):
    nq = Q.shape[0]
    q = torch.from_numpy(Q).to(DEV)
    s = torch.empty((nq, k), dtype=torch.float32, device=DEV)
    i = torch.empty((nq, k), dtype=torch.int64, device=DEV)
    idx.reserve(nq, k)
    idx.search_device(q.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def assert_same_device(g, f, Q):
    for nq, k in SEARCHES:
        k = min(k, max(g.ntotal, 1))
        (gs, gi), (fs, fi) = device_search(g, Q[:nq], k), device_search(f, Q[:nq], k)
        assert np.array_equal(gi, fi) and np.array_equal(bits(gs), bits(fs)), ("search_device", nq, k)


# with and without a resident fp16 image; the fp16 first pass (and so the image) exists at multiples of 128 only
CASES = [(n, d, image) for n in NS for d in DS for image in (False, True) if not image or d % 128 == 0]


@pytest.mark.parametrize("n, d, image", CASES, ids=[f"{n}x{d}{'-fp16-image' if i else ''}" for n, d, i in CASES])
def test_replace_patterns(nat, n, d, image):
    assert not image or nat.dense_hi_supported(d)
    rng = np.random.default_rng(1000 * n + d)
    X, Q = unit_rows(rng, n, d), unit_rows(rng, 33, d)
    for what, ids in patterns(n).items():
        if not ids:  # (31 rows have no tile edge)
            continue
        R = unit_rows(rng, len(ids), d)
        g = nat.DenseIndex(X)
        if image:
            g.build_image()
        assert g.replace_kernel_ms() == -1.0
        g.replace(ids, R)
        assert g.replace_kernel_ms() >= 0.0, what
        want = edited(X, ids, R)
        f = nat.DenseIndex(want)
        if image:
            f.build_image()
            assert g.image_info() == f.image_info(), what
        assert_same(g, f, Q, want)
        assert_same_device(g, f, Q)
        g.close()
        f.close()


def test_the_two_pass_short_corpus_form_reads_the_new_statistics(nat):
    """4 096 queries on <= 1 024 rows: the two-pass form, whose short-corpus fp16 image is of the old matrix."""
    rng = np.random.default_rng(52)
    n, d, nq, k = 200, 128, 4096, 10
    X, Q = unit_rows(rng, n, d), unit_rows(rng, nq, d)
    X[50] *= np.float32(8.0)
    g = nat.DenseIndex(X)
    assert "dsh_scores_kernel" in g.plan_info(nq, k)
    g.search(Q, k)  # makes the short-corpus fp16 image of the old matrix
    R = unit_rows(rng, 3, d)
    g.replace([31, 50, 199], R)
    f = nat.DenseIndex(edited(X, [31, 50, 199], R))
    assert "dsh_scores_kernel" in g.plan_info(nq, k)
    (gs, gi), (fs, fi) = g.search(Q, k), f.search(Q, k)
    assert np.array_equal(gi, fi) and np.array_equal(bits(gs), bits(fs))
    g.close()
    f.close()


def test_the_scale_falls_with_the_largest_component_and_the_image_follows(nat):
    """One row holds a component 8x the others': while it is resident the image's scale is set by it; replacing it with
    a unit row must bring the scale a fresh handle's image has — all of the image is converted again, not only the
    tiles from the replaced row on."""
    rng = np.random.default_rng(51)
    n, d = 300, 128
    X, Q = unit_rows(rng, n, d), unit_rows(rng, 33, d)
    top = int(np.abs(X).max(axis=1).argmax())
    big = 250 if top != 250 else 251  # in the image's last tiles: rows before it are converted again for the new scale
    X[big] = np.float32(8.0) * X[top]
    g = nat.DenseIndex(X)
    g.build_image()
    e_before = g.image_info()[3]
    R = unit_rows(rng, 1, d) * np.float32(0.5)
    g.replace([big], R)
    want = edited(X, [big], R)
    f = nat.DenseIndex(want)
    f.build_image()
    present, _, covered, e = g.image_info()
    assert present and covered == n
    assert e == f.image_info()[3] and e == e_before - 3, (e_before, e, f.image_info())
    assert g.image_info() == f.image_info()
    assert_same(g, f, Q, want)
    assert_same_device(g, f, Q)
    g.close()
    f.close()


def test_a_nan_row_an_infinite_row_and_back(nat):
    """A NaN component leaves the statistics finite (the maxima drop it, as under create and add), so the handle keeps
    its image, as a fresh handle of that matrix builds one; an infinity does not: the image is dropped, and once the row
    is replaced back the owner of the handle builds it again."""
    rng = np.random.default_rng(56)
    n, d = 300, 128
    X, Q = unit_rows(rng, n, d), unit_rows(rng, 33, d)
    g = nat.DenseIndex(X)
    g.build_image()
    bad = X[[40]].copy()
    bad[0, 5] = np.nan
    g.replace([40], bad)
    want = edited(X, [40], bad)
    f = nat.DenseIndex(want)
    f.build_image()
    assert g.image_info() == f.image_info() and g.image_info()[0]
    assert_same(g, f, Q, want)
    f.close()
    bad[0, 5] = np.inf
    g.replace([40], bad)
    assert g.image_info() == (False, 0, 0, 0)  # statistics that are not finite: no first pass is left to read it
    want = edited(X, [40], bad)
    assert np.array_equal(bits(g.read_rows(0, n)), bits(want))
    f = nat.DenseIndex(want)
    with pytest.raises(nat.NativeError):
        f.build_image()
    assert_same(g, f, Q, want)
    f.close()
    g.replace([40], X[[40]])
    assert g.image_info() == (False, 0, 0, 0)  # dropped, not made from nothing
    f = nat.DenseIndex(X)
    assert_same(g, f, Q, X)
    g.build_image()
    f.build_image()
    assert g.image_info() == f.image_info() and g.image_info()[0]
    assert_same(g, f, Q, X)
    assert_same_device(g, f, Q)
    g.close()
    f.close()


def test_replace_after_add_and_remove_and_twice(nat):
    rng = np.random.default_rng(53)
    n, d = 300, 128
    X, more, Q = unit_rows(rng, n, d), unit_rows(rng, 40, d), unit_rows(rng, 33, d)
    g = nat.DenseIndex(X)
    g.build_image()
    g.add(more)
    rows = np.concatenate([X, more])
    R = unit_rows(rng, 4, d)
    g.replace([0, 299, 300, 339], R)  # old rows, the seam of the add, the last row
    rows = edited(rows, [0, 299, 300, 339], R)
    g.remove([5, 300])
    rows = np.delete(rows, [5, 300], axis=0)
    R2 = unit_rows(rng, 2, d)
    g.replace([4, 337], R2)
    g.replace([4], R[:1])  # two replaces in a row, of one row
    rows = edited(edited(rows, [4, 337], R2), [4], R[:1])
    f = nat.DenseIndex(rows)
    f.build_image()
    assert g.image_info() == f.image_info()
    assert_same(g, f, Q, rows)
    g.close()
    f.close()


def test_bad_arguments_leave_the_rows_as_they_were(nat):
    rng = np.random.default_rng(55)
    n, d = 300, 128
    X = unit_rows(rng, n, d)
    R = unit_rows(rng, 2, d)
    g = nat.DenseIndex(X)
    lib = nat.load()

    def raw(h, ids, rows, cnt):
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
        nat._check(lib.amdr_dense_replace(h, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int64)),
                                          None if rows is None else rows.ctypes.data_as(C.POINTER(C.c_float)),
                                          C.c_int64(cnt)), "amdr_dense_replace")

    Xd = torch.from_numpy(X).to(DEV)
    torch.cuda.synchronize()
    wrapped = nat.DenseIndex(device_ptr=Xd.data_ptr(), n=n, dim=d, keepalive=Xd)
    ok = [1, 3]
    many = np.ascontiguousarray(np.tile(R, (151, 1))[:n + 1])
    for h, ids, rows, cnt in ((None, ok, R, 2), (g, ok, R, -1), (g, None, R, 2), (g, ok, None, 2), (g, [1, n], R, 2),
                              (g, [-1, 3], R, 2), (g, [3, 1], R, 2), (g, [3, 3], R, 2), (g, list(range(n + 1)), many, n + 1),
                              (wrapped, ok, R, 2)):
        with pytest.raises(nat.NativeError, match="status -1"):
            raw(None if h is None else h._h, ids, rows, cnt)
        for idx in (g, wrapped):
            assert idx.ntotal == n and np.array_equal(bits(idx.read_rows(0, n)), bits(X))
    raw(g._h, None, None, 0)  # n_rep == 0: a no-op that reads nothing
    assert g.ntotal == n and g.replace_kernel_ms() == -1.0
    with pytest.raises(ValueError):
        g.replace([1], R)  # the wrapper: one row for every id
    g.close()
    wrapped.close()

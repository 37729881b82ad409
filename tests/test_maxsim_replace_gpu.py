"""amdr_maxsim_replace: after a replace a MaxSim handle is what amdr_maxsim_create makes of the edited store — D and
doc_ptr the same bytes, the scale, the first-pass bound and the images made again from the new D, hence the same ids and
score BITS from every entry point and on every route (csrc/maxsim_store.hip, csrc/rows_compact.hip).  `g` is created from the
whole store and replaced in, `f` from the store edited on the host.  The helpers are those of
tests/test_maxsim_remove_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from test_maxsim_remove_gpu import N_DOCS, assert_same, bits, concat, nat, part, queries, survivors, unit_rows  # noqa: F401

pytestmark = pytest.mark.gpu

EDGE = (1, 2, 31, 32, 33)


def edge_store(rng, n_docs=N_DOCS):
    """Documents of 1, 2, 31, 32, 33 tokens in turn (document j: EDGE[j % 5]), the last one 33."""
    lens = np.asarray([EDGE[j % 5] for j in range(n_docs)])
    lens[-1] = 33
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return unit_rows(rng, int(ptr[-1])), ptr


def new_part(rng, lens):
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return unit_rows(rng, int(ptr[-1])), ptr


def edited(store, ids, new):
    """The plain edit on the host: documents `ids` of the store exchanged for the documents of `new`."""
    D, ptr = store
    nd, nptr = new
    docs = [D[ptr[j]:ptr[j + 1]] for j in range(ptr.shape[0] - 1)]
    for i, j in enumerate(ids):
        docs[int(j)] = nd[nptr[i]:nptr[i + 1]]
    return np.ascontiguousarray(np.concatenate(docs)), np.concatenate([[0], np.cumsum([d.shape[0] for d in docs])]).astype(np.int64)


PATTERNS = {
    "first": [0],
    "last": [N_DOCS - 1],
    "one adjacent run": list(range(13, 18)),
    "alternating": list(range(1, N_DOCS, 2)),
    "all but one": [i for i in range(N_DOCS) if i != 20],
    "every document": list(range(N_DOCS)),
    "a single id": [20],
}


# the new length of old document j: grow to the next edge length, shrink to the previous one, keep
HOW = {"grow": lambda n: EDGE[min(EDGE.index(n) + 1, 4)], "shrink": lambda n: EDGE[max(EDGE.index(n) - 1, 0)],
       "keep": lambda n: n, "long": lambda n: 220}


@pytest.mark.parametrize("how", list(HOW))
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_replace_patterns(nat, monkeypatch, queries, pattern, how):
    rng = np.random.default_rng(2032)
    store = edge_store(rng)
    ids = PATTERNS[pattern]
    old_lens = np.diff(store[1])
    new = new_part(rng, [HOW[how](int(old_lens[j])) for j in ids])
    g = nat.MaxSimIndex(*store)
    assert g.replace_kernel_ms() == -1.0 and g.info()[5] == 1
    g.replace(ids, *new)
    want = edited(store, ids, new)
    f = nat.MaxSimIndex(*want)
    info = g.info()
    assert info[0] == N_DOCS and info[2] == info[1] == f.info()[1] == want[0].shape[0]  # capacity = the store
    assert info[5] == 2 and g.replace_kernel_ms() >= 0.0  # one more whole-store conversion
    assert_same(nat, monkeypatch, g, f, queries, seam=ids[0])
    g.close()
    f.close()


def test_the_scale_falls_with_the_largest_component(nat, monkeypatch, queries):
    rng = np.random.default_rng(41)
    D, ptr = part(rng, N_DOCS)
    D[int(ptr[17]) + (int(ptr[18] - ptr[17]) // 2), :] = 0.0
    D[int(ptr[17]) + (int(ptr[18] - ptr[17]) // 2), 7] = 3.0
    g = nat.MaxSimIndex(D, ptr)
    assert g.info()[3] == -2  # 3.0 = 0.75 * 2^2: d_scale = 2^-2
    new = new_part(rng, [5])
    g.replace([17], *new)
    f = nat.MaxSimIndex(*edited((D, ptr), [17], new))
    assert g.info()[3] == f.info()[3] == 1  # unit rows, largest component in [0.25, 0.5): d_scale = 2^1
    assert_same(nat, monkeypatch, g, f, queries, seam=17)
    # and rises again with a replacement that brings such a component
    big = new_part(rng, [3])
    big[0][1, 9] = 3.0
    g.replace([N_DOCS - 1], *big)
    f.close()
    f = nat.MaxSimIndex(*edited(edited((D, ptr), [17], new), [N_DOCS - 1], big))
    assert g.info()[3] == f.info()[3] == -2
    assert_same(nat, monkeypatch, g, f, queries, seam=N_DOCS - 1)
    g.close()
    f.close()


def test_replacing_the_only_nan_brings_the_images(nat, monkeypatch, queries):
    rng = np.random.default_rng(43)
    D, ptr = part(rng, N_DOCS)
    D[int(ptr[5]), 17] = np.nan
    g = nat.MaxSimIndex(D, ptr)
    assert g.info()[4] == 0 and g.info()[5] == 0 and "fp32-input" in g.plan_info(8)
    a, b = new_part(rng, [33]), new_part(rng, [2])
    g.replace([30], *a)  # the NaN stays: still no images, no conversion
    store = edited((D, ptr), [30], a)
    f = nat.MaxSimIndex(*store)
    assert g.info()[4] == 0 and g.info()[5] == 0
    assert_same(nat, monkeypatch, g, f, queries)
    f.close()
    g.replace([5], *b)
    store = edited(store, [5], b)
    f = nat.MaxSimIndex(*store)
    assert g.info()[4] == 1 and f.info()[4] == 1 and g.info()[5] == 1
    assert_same(nat, monkeypatch, g, f, queries, seam=5)
    f.close()
    # and a replacement that brings an infinity takes them away again
    c = new_part(rng, [4])
    c[0][2, 3] = np.inf
    g.replace([0], *c)
    f = nat.MaxSimIndex(*edited(store, [0], c))
    assert g.info()[4] == 0 and f.info()[4] == 0
    assert_same(nat, monkeypatch, g, f, queries)
    g.close()
    f.close()


def test_replace_after_add_and_after_remove(nat, monkeypatch, queries):
    rng = np.random.default_rng(44)
    base, a = part(rng, N_DOCS), part(rng, 7)
    g = nat.MaxSimIndex(*base)
    g.add(*a)
    whole = concat([base, a])
    ids = [0, 39, 40, 46]  # across the seam of the add, its last document too
    new = new_part(rng, [64, 1, 33, 2])
    g.replace(ids, *new)
    whole = edited(whole, ids, new)
    f = nat.MaxSimIndex(*whole)
    assert_same(nat, monkeypatch, g, f, queries, seam=40)
    f.close()
    g.remove([0, 40])
    left = survivors(whole, [0, 40])
    new2 = new_part(rng, [31, 220])
    g.replace([0, 44], *new2)  # the new first and the new last document
    left = edited(left, [0, 44], new2)
    f = nat.MaxSimIndex(*left)
    assert g.info()[0] == N_DOCS + 7 - 2
    assert_same(nat, monkeypatch, g, f, queries, seam=1)
    g.close()
    f.close()


def test_bad_arguments_leave_the_store_as_it_was(nat, queries):
    base = part(np.random.default_rng(45), N_DOCS)
    g = nat.MaxSimIndex(*base)
    before = (g.info(), g.stats(), g.search(queries[:9], 10))
    lib = nat.load()
    new = new_part(np.random.default_rng(46), [3, 4])

    def raw(h, ids, D, ptr, n):
        arr = lambda x, t: None if x is None else np.ascontiguousarray(x, dtype=t)  # noqa: E731
        ids, D, ptr = arr(ids, np.int64), arr(D, np.float32), arr(ptr, np.int64)
        p = lambda x, t: None if x is None else x.ctypes.data_as(C.POINTER(t))  # noqa: E731
        nat._check(lib.amdr_maxsim_replace(h, p(ids, C.c_int64), p(D, C.c_float), p(ptr, C.c_int64), C.c_int64(n)),
                   "amdr_maxsim_replace")

    ok = [1, 3]
    every = list(range(N_DOCS + 1))
    for args in ((None, ok, *new, 2), (g._h, ok, *new, -1), (g._h, None, *new, 2), (g._h, ok, None, new[1], 2),
                 (g._h, ok, new[0], None, 2), (g._h, [1, N_DOCS], *new, 2), (g._h, [-1, 3], *new, 2), (g._h, [3, 1], *new, 2),
                 (g._h, [3, 3], *new, 2), (g._h, every, new[0], np.arange(N_DOCS + 2), N_DOCS + 1),
                 (g._h, ok, new[0], [1, 3, 7], 2), (g._h, ok, new[0], [0, 0, 7], 2), (g._h, ok, new[0], [0, 7, 7], 2)):
        with pytest.raises(nat.NativeError, match="status -1"):
            raw(*args)
        after = (g.info(), g.stats(), g.search(queries[:9], 10))
        assert after[0] == before[0] and after[1] == before[1] and np.array_equal(after[2][1], before[2][1])
        assert np.array_equal(bits(after[2][0]), bits(before[2][0]))
        gd, gp = g.read()
        assert np.array_equal(bits(gd), bits(base[0])) and np.array_equal(gp, base[1])
    raw(g._h, None, None, None, 0)  # n_rep == 0: a no-op that reads nothing
    assert g.info() == before[0] and g.replace_kernel_ms() == -1.0
    with pytest.raises(ValueError):
        g.replace([1], new[0], new[1])  # the wrapper: one document for every id
    g.close()

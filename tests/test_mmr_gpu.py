"""amdr_mmr / amdr_mmr_device (csrc/mmr.hip) against the fp64 restatement of the definition (tests/mmr_adversary.py).

Integer matrices: positions, counts and the bits of out_mmr / out_maxsim, whole rows including the fill past out_count.
Real-valued matrices: certified seeds only, equal positions, values inside the rounding bound of an fp32 Gram.  Every case
runs through BOTH call forms, which must agree with each other bit for bit; the device outputs carry guard rows behind
them, which must come back untouched."""
import math

import numpy as np
import pytest

import mmr_adversary as M

pytestmark = pytest.mark.gpu

GUARD = 64
SENT_I, SENT_V = -777, -123.25


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


_INDEX = {}


def index_of(nat, X):
    """One resident index per matrix object (the builders cache and freeze their matrices)."""
    if id(X) not in _INDEX:
        _INDEX[id(X)] = (X, nat.DenseIndex(X, device=0))
    return _INDEX[id(X)][1]


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(dev())


class Guarded:
    """A device output of `rows` rows with GUARD sentinel rows behind it."""

    def __init__(self, rows, width, dtype, fill):
        import torch
        self.rows, self.width, self.fill = rows, max(width, 1), fill
        self.t = torch.full(((rows + GUARD) * self.width,), fill, dtype=dtype, device=dev())

    def host(self, shape, what):
        a = self.t.cpu().numpy()
        assert (a[self.rows * self.width:] == self.fill).all(), (what, "wrote past the end of an output")
        return a[:self.rows * self.width].reshape(shape).copy()


def run_device(idx, rows, rel, count, pool, k_sel, lam, what, rel_dev=None):
    import torch
    nq = len(count)
    rows_t, cnt_t = to_dev(rows), to_dev(np.asarray(count, dtype=np.int32))
    rel_t = rel_dev if rel_dev is not None else to_dev(rel)
    op, oc = Guarded(nq, k_sel, torch.int32, SENT_I), Guarded(nq, 1, torch.int32, SENT_I)
    ov, os_ = Guarded(nq, k_sel, torch.float64, SENT_V), Guarded(nq, k_sel, torch.float64, SENT_V)
    idx.mmr_device(rows_t, rel_t, cnt_t, nq, pool, k_sel, lam, op.t, ov.t, os_.t, oc.t, ld_rows=rows.shape[1],
                   stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return op.host((nq, k_sel), what), ov.host((nq, k_sel), what), os_.host((nq, k_sel), what), oc.host((nq,), what)


def run_both(nat, case, what=None):
    """-> the host form's record, after checking that the device form's equals it bit for bit."""
    what = what or case.name
    idx = index_of(nat, case.X)
    host = idx.mmr(case.rows, case.rel, case.count, case.pool, case.k_sel, case.lam)
    devr = run_device(idx, case.rows, case.rel, case.count, case.pool, case.k_sel, case.lam, what)
    M.assert_exact(devr, host, (what, "amdr_mmr_device against amdr_mmr"))
    return host


# ---- a. pools x widths x k_sel x matrices, integer data ---------------------------------------------------------------------
@pytest.mark.parametrize("n", (7, 5000))
@pytest.mark.parametrize("d", M.DIMS)
def test_integer_grid(nat, d, n):
    """Every pool of the tile and wave edges, k_sel = 1 / half / pool, ragged, full and short counts (0 and above the pool
    included), rows in random, descending and repeated order with a -1, an n, the zero row and a row twice planted, every
    rel kind and lambda: the oracle's answer bit for bit."""
    for case in M.grid_cases(d, n):
        M.assert_exact(run_both(nat, case), case.exp, case.name)


# ---- b. real-valued rows: certified seeds ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", M.REAL_LAMS)
@pytest.mark.parametrize("d", M.REAL_DIMS)
def test_real_certified(nat, d, lam):
    for case in M.real_cases(d, lam):
        got = run_both(nat, case)
        print(case.name, "max |maxsim - oracle|", np.abs(got[2] - case.exp[2]).max(), "E", M.cos_bound(d))
        M.assert_close(got, case.exp, lam, d, case.name)


# ---- c. the grid edge: more queries than a grid's y holds ----------------------------------------------------------------------
@pytest.mark.parametrize("nq", (1, 3, 70000))
def test_batch_sizes(nat, nq):
    base = M.int_case(7, 4, 997, 3, 2, 0.5, seed=3, rel_kind="edges", ld_extra=1)
    rows, rel, count, exp = M.tiled(base, nq)
    idx = index_of(nat, base.X)
    host = idx.mmr(rows, rel, count, 3, 2, 0.5)
    M.assert_exact(host, exp, ("amdr_mmr", nq))
    M.assert_exact(run_device(idx, rows, rel, count, 3, 2, 0.5, nq), host, ("amdr_mmr_device", nq))


# ---- d. value edges of rel, and the two pinned consequences ----------------------------------------------------------------
def test_rel_edges_every_lambda(nat):
    """Exact ties, +-0.0, +-inf and NaN among the relevances, at every lambda (0 * inf = NaN at lambda 0 included)."""
    for t, lam in enumerate(M.LAMS):
        for pool in (3, 33, 64):
            case = M.int_case(50, 132, 4, pool, pool, lam, seed=40 + t, rel_kind="edges", count_kind="full")
            M.assert_exact(run_both(nat, case), case.exp, case.name)
    X = M.int_matrix(7, 4)
    rel = np.array([[0.0, -0.0, 0.0, -0.0], [math.nan, -math.inf, math.nan, -math.inf], [1.0, 1.0, 1.0, 1.0]])
    rows = np.array([[6, 6, 6, 6], [4, 5, 6, 0], [3, 3, -1, 7]], dtype=np.int64)  # one vector; mixed; no vector at all
    case = M.Case(X, rows, rel, [4, 4, 4], 4, 4, 0.5, "ties, signed zeros, NaN behind -inf")
    got = run_both(nat, case)
    M.assert_exact(got, case.exp, case.name)
    assert got[0][0].tolist() == [0, 1, 2, 3] and got[0][2].tolist() == [0, 1, 2, 3]
    assert got[0][1].tolist() == [1, 3, 0, 2], "NaN ranks behind -inf and NaNs keep their order"


def test_lambda_one_is_the_plain_ranking(nat):
    case = M.int_case(5000, 768, 5, 64, 64, 1.0, rel_kind="desc", count_kind="full", seed=7)
    got = run_both(nat, case)
    M.assert_exact(got, case.exp, case.name)
    assert (got[0] == np.arange(64)).all()


def test_same_row_twice_has_cosine_one(nat):
    X = M.int_matrix(7, 124)
    case = M.Case(X, np.array([[4, 5, 4]]), np.array([[3.0, 2.0, 2.5]]), [3], 3, 3, 0.25, "row 4 twice")
    got = run_both(nat, case)
    M.assert_exact(got, case.exp, case.name)
    assert got[2][0][got[0][0].tolist().index(2)] == 1.0


# ---- e. a strided view into a packed fused result ----------------------------------------------------------------------------
def test_rel_view_into_packed_block(nat):
    """rel = the AMDR_FV_SCORE column of a [nq, max_out, 9] block (rel_stride 9, rel_ld max_out * 9), read in place by both
    forms; the other eight values of every hit are garbage."""
    case = M.int_case(5000, 128, 5, 31, 10, M.LAM_ODD, seed=9, rel_kind="random", ld_extra=4)
    nq, max_out = case.nq, case.rows.shape[1]
    rng = np.random.default_rng(5)
    vals = rng.standard_normal((nq, max_out, 9)) * 1e3
    vals[:, :, 0] = case.rel
    idx = index_of(nat, case.X)
    host = idx.mmr(case.rows, vals[:, :, 0], case.count, case.pool, case.k_sel, case.lam)
    M.assert_exact(host, case.exp, ("amdr_mmr, strided rel", case.name))
    vt = to_dev(vals)
    view = vt[:, :, 0]
    assert view.stride() == (max_out * 9, 9)
    devr = run_device(idx, case.rows, None, case.count, case.pool, case.k_sel, case.lam, case.name, rel_dev=view)
    M.assert_exact(devr, host, ("amdr_mmr_device, strided rel", case.name))


# ---- f. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors(nat):
    import torch
    X = M.int_matrix(7, 4)
    idx = index_of(nat, X)
    rows, rel, count = np.zeros((2, 8), dtype=np.int64), np.zeros((2, 8)), np.array([3, 3], dtype=np.int32)

    def host(pool=4, k=2, lam=0.5, rows=rows):
        return idx.mmr(rows, rel, count, pool, k, lam)

    for kw, msg in ((dict(pool=0), r"pool must be in \[1, 64\]"), (dict(pool=65), r"pool must be in \[1, 64\]"),
                    (dict(k=0), r"k_sel must be in \[1, pool\]"), (dict(k=5), r"k_sel must be in \[1, pool\]"),
                    (dict(lam=-0.01), r"lambda must be in \[0, 1\]"), (dict(lam=1.01), r"lambda must be in \[0, 1\]"),
                    (dict(lam=math.nan), r"lambda must be in \[0, 1\]"),
                    (dict(pool=8, rows=rows[:, :7].copy()), r"ld_rows must be >= pool")):
        with pytest.raises(nat.NativeError, match=msg):
            host(**kw)
    lib = nat.load()
    t = torch.zeros(64, dtype=torch.float64, device=dev())
    p = t.data_ptr()

    def raw(**kw):
        a = dict(rows=p, ld=8, rel=p, rs=1, rl=8, count=p, nq=2, pool=4, k=2, lam=0.5, op=p, om=p, os=p, oc=p)
        a.update(kw)
        return lib.amdr_mmr_device(idx._h, a["rows"], a["ld"], a["rel"], a["rs"], a["rl"], a["count"], a["nq"], a["pool"],
                                   a["k"], a["lam"], a["op"], a["om"], a["os"], a["oc"], None)

    for kw, msg in ((dict(nq=-1), "nq must be >= 0"), (dict(ld=3), "ld_rows must be >= pool"), (dict(rs=0), "bad rel strides"),
                    (dict(pool=65), "pool must be in"), (dict(k=5), "k_sel must be in"), (dict(lam=2.0), "lambda must be in"),
                    *((({name: None}), "null buffer") for name in ("rows", "rel", "count", "op", "om", "os", "oc"))):
        assert raw(**kw) == -1, kw
        assert msg in lib.amdr_last_error().decode(), (kw, lib.amdr_last_error())
    assert lib.amdr_mmr_device(None, p, 8, p, 1, 8, p, 2, 4, 2, 0.5, p, p, p, p, None) == -1
    assert "null handle" in lib.amdr_last_error().decode()
    assert lib.amdr_mmr(idx._h, None, 8, None, 1, 8, None, 2, 4, 2, 0.5, None, None, None, None) == -1
    assert "null buffer" in lib.amdr_last_error().decode()
    # nq == 0: a successful no-op in both forms, null buffers included
    assert raw(nq=0, rows=None, rel=None, count=None, op=None, om=None, os=None, oc=None) == 0
    pos, val, sim, cnt = idx.mmr(np.zeros((0, 4), dtype=np.int64), np.zeros((0, 4)), np.zeros(0, dtype=np.int32), 4, 2, 0.5)
    assert pos.shape == (0, 2) and cnt.shape == (0,)
    torch.cuda.synchronize()

"""Facet counts on the GPU (amdr_facet_counts: csrc/facet.hip, csrc/facet_rule.hpp): the "_device" call and the host twin
equal the plain evaluator of tests/facet_cases.py exactly, at the smallest shapes where the kernels can go wrong — scopes of
0, 1, T - 1, T, T + 1 and 3 T + 7 rows (T = AMDR_FACET_TILE_ROWS), fields of 1, B - 1, B, B + 1 and 3 B + 5 values (B =
AMDR_FACET_LDS_BINS: the step from the LDS histogram to global adds), one bin that takes every add, every row its own code,
no row with a value, codes outside [0, n_codes), ties across the cut, top 1 and 64, a padded list, three fields of different
widths in one call, 70 000 one-row constraints — then rows outside [0, n_rows) in the "_device" form, each argument error
(after which the outputs are untouched), and the call captured in a graph and replayed over a rewritten table."""
import ctypes as C

import numpy as np
import pytest
import torch

import facet_cases as FC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = -77
NAMES = ("total", "missing", "distinct", "code", "count")


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    assert (_native.FACET_TILE_ROWS, _native.FACET_LDS_BINS) == (FC.T, FC.B)
    return _native


@pytest.fixture(scope="module")
def ws(nat):
    return nat.ScopeWorkspace(device=0)


@pytest.fixture(scope="module")
def families():
    """name -> (case, what the evaluator gives): computed once, shared and left unchanged."""
    return {name: (c, FC.evaluate(**c)) for name, c in FC.families().items()}


def dev_arr(a, dtype):
    t = torch.zeros(max(int(np.size(a)), 1), dtype=dtype, device=DEV)
    if np.size(a):
        t[:np.size(a)].copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()))
    return t


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


class DeviceCall:
    """The operands of one amdr_facet_counts_device call on the device and its outputs, filled with SENTINEL."""

    def __init__(self, nat, case, rows_max=None, rows_cap=None):
        self.nat = nat
        sp, rows = case["scope_ptr"], case["rows"]
        self.n_cons, self.n_codes, self.top = int(sp.size) - 1, list(case["n_codes"]), int(case["top"])
        self.n_fields, self.n_rows = case["codes"].shape
        self.rows_max = int(np.diff(sp).max()) if rows_max is None and self.n_cons else int(rows_max or 0)
        self.sp = dev_arr(sp, torch.int64)
        self.rows = dev_arr(np.concatenate([rows, np.zeros(max(int(rows_cap or 0) - rows.size, 0), np.int64)]), torch.int64)
        self.codes = dev_arr(case["codes"], torch.int32)
        cf = self.n_cons * self.n_fields
        shapes = ((self.n_cons,), (self.n_cons, self.n_fields), (self.n_cons, self.n_fields), (self.n_cons, self.n_fields, self.top),
                  (self.n_cons, self.n_fields, self.top))
        dtypes = (torch.int64, torch.int64, torch.int32, torch.int32, torch.int64)
        self.shapes = shapes
        self.outs = [torch.full((max(int(np.prod(s)), 1),), SENTINEL, dtype=d, device=DEV) for s, d in zip(shapes, dtypes)]
        assert cf >= 0
        self.work_bytes = nat.facet_plan(self.n_cons, self.n_codes)
        self.work = torch.full((self.work_bytes + 8,), 0x5a, dtype=torch.uint8, device=DEV)  # (dirty: the call zeroes it)

    def __call__(self):
        self.nat.facet_counts_device(self.sp.data_ptr(), self.rows.data_ptr(), self.n_cons, self.rows_max, self.codes.data_ptr(),
                                     self.n_rows, self.n_codes, self.top, *(o.data_ptr() for o in self.outs),
                                     self.work.data_ptr(), self.work_bytes, stream_ptr())

    def fetch(self):
        torch.cuda.synchronize()
        return tuple(o.cpu().numpy()[:int(np.prod(s))].reshape(s).copy() for o, s in zip(self.outs, self.shapes))


def assert_equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w):
            at = tuple(int(x) for x in np.argwhere(g != w)[0])
            raise AssertionError(f"{what}: {name} differs first at {at}: got {g[at]}, want {w[at]}")


@pytest.mark.parametrize("name", sorted(FC.families()))
def test_the_device_call_and_the_host_twin_equal_the_evaluator(nat, ws, families, name):
    case, want = families[name]
    call = DeviceCall(nat, case)
    call()
    assert_equal(call.fetch(), want, f"{name} (device)")
    got = ws.facet_counts(case["scope_ptr"], case["rows"], case["codes"], case["n_codes"], case["top"])
    assert_equal(got, want, f"{name} (host twin)")
    # a looser bound changes nothing; the tile count follows it
    loose = DeviceCall(nat, case, rows_max=FC.N_ROWS + 5 * FC.T)
    loose()
    assert_equal(loose.fetch(), want, f"{name} (device, loose rows_max)")


def test_70_000_one_row_constraints_in_one_call(nat, ws):
    case = FC.many_case()
    want = FC.evaluate(**case)
    assert (want[0] == 1).all() and case["scope_ptr"].size - 1 > 65_535
    call = DeviceCall(nat, case)
    call()
    assert_equal(call.fetch(), want, "70 000 constraints (device)")
    assert_equal(ws.facet_counts(case["scope_ptr"], case["rows"], case["codes"], case["n_codes"], case["top"]), want,
                 "70 000 constraints (host twin)")


def test_no_constraint_enqueues_nothing_and_empty_scopes_are_all_padding(nat, ws):
    codes = np.zeros((2, 5), dtype=np.int32)
    none = {"scope_ptr": np.zeros(1, np.int64), "rows": np.zeros(0, np.int64), "codes": codes, "n_codes": [3, 4], "top": 4}
    call = DeviceCall(nat, none)
    call()
    torch.cuda.synchronize()
    assert all((o == SENTINEL).all() for o in call.outs) and (call.work == 0x5a).all()
    got = ws.facet_counts(none["scope_ptr"], none["rows"], codes, [3, 4], 4)
    assert [g.shape for g in got] == [(0,), (0, 2), (0, 2), (0, 2, 4), (0, 2, 4)]
    empty = {"scope_ptr": np.zeros(4, np.int64), "rows": np.zeros(0, np.int64), "codes": codes, "n_codes": [3, FC.B + 1], "top": 4}
    want = FC.evaluate(**empty)
    assert not want[0].any() and not want[2].any() and (want[3] == -1).all() and not want[4].any()
    call = DeviceCall(nat, empty)
    call()
    assert_equal(call.fetch(), want, "empty scopes (device)")
    assert_equal(ws.facet_counts(empty["scope_ptr"], empty["rows"], codes, empty["n_codes"], 4), want, "empty scopes (host twin)")
    # no row in the list at all: every scope is empty whatever it says
    bare = dict(empty, codes=np.zeros((2, 0), dtype=np.int32))
    assert_equal(ws.facet_counts(bare["scope_ptr"], bare["rows"], bare["codes"], bare["n_codes"], 4), want, "no rows (host twin)")


def test_the_device_form_never_counts_a_row_outside_the_list(nat, ws):
    """Rows outside [0, n_rows) — negative, n_rows itself, far past it — are not dereferenced and counted nowhere, total
    included; a rows_max below a scope's length reads only that many of its rows.  The host twin refuses both tables."""
    case = FC.case(("random", "stray"), (11, FC.B + 3), 6, 301, lengths=(0, 5, FC.T + 9, 700), n_rows=3000)
    rows = case["rows"].copy()
    rng = np.random.default_rng(302)
    hit = rng.random(rows.size) < 0.3
    rows[hit] = rng.choice(np.array([-1, -2 ** 40, 3000, 3001, 2 ** 31, 2 ** 62], dtype=np.int64), size=int(hit.sum()))
    stray = dict(case, rows=rows)
    want = FC.evaluate(**stray)
    assert 0 < want[0][2] < FC.T + 9
    call = DeviceCall(nat, stray)
    call()
    assert_equal(call.fetch(), want, "stray rows (device)")
    with pytest.raises(nat.NativeError, match="strictly ascending"):
        ws.facet_counts(stray["scope_ptr"], rows, stray["codes"], stray["n_codes"], 6)
    # rows_max = 600: the scopes of T + 9 and 700 rows are read up to their 600th row
    cut = DeviceCall(nat, case, rows_max=600)
    cut()
    sp = case["scope_ptr"]
    parts = [case["rows"][sp[p]:sp[p + 1]][:600] for p in range(4)]
    short = dict(case, scope_ptr=np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64), rows=np.concatenate(parts))
    assert_equal(cut.fetch(), FC.evaluate(**short), "rows_max below the scopes (device)")
    with pytest.raises(nat.NativeError, match="rows_max"):
        ws.facet_counts(case["scope_ptr"], case["rows"], case["codes"], case["n_codes"], 6, rows_max=600)


def test_argument_errors_enqueue_nothing_and_leave_the_outputs_untouched(nat, ws):
    case = FC.families()["three-fields"]
    call = DeviceCall(nat, case)
    lib = nat.load()
    nc = np.asarray(call.n_codes, dtype=np.int64)

    def raw(**over):
        a = dict(scope_ptr=call.sp.data_ptr(), rows=call.rows.data_ptr(), n_cons=call.n_cons, rows_max=call.rows_max,
                 codes=call.codes.data_ptr(), n_rows=call.n_rows, n_fields=call.n_fields, n_codes=nc, top=call.top,
                 total=call.outs[0].data_ptr(), missing=call.outs[1].data_ptr(), distinct=call.outs[2].data_ptr(),
                 code=call.outs[3].data_ptr(), count=call.outs[4].data_ptr(), work=call.work.data_ptr(), work_bytes=call.work_bytes)
        a.update(over)
        vp = lambda x: C.c_void_p(int(x) if x else 0)  # noqa: E731
        ncp = None if a["n_codes"] is None else a["n_codes"].ctypes.data_as(C.c_void_p)
        return lib.amdr_facet_counts_device(vp(a["scope_ptr"]), vp(a["rows"]), C.c_int64(a["n_cons"]), C.c_int64(a["rows_max"]),
                                            vp(a["codes"]), C.c_int64(a["n_rows"]), C.c_int32(a["n_fields"]), ncp, C.c_int32(a["top"]),
                                            vp(a["total"]), vp(a["missing"]), vp(a["distinct"]), vp(a["code"]), vp(a["count"]),
                                            vp(a["work"]), C.c_int64(a["work_bytes"]), vp(stream_ptr()))
    bad = [dict(scope_ptr=0), dict(rows=0), dict(codes=0), dict(n_codes=None), dict(total=0), dict(missing=0), dict(distinct=0),
           dict(code=0), dict(count=0), dict(work=0),
           dict(n_cons=-1), dict(rows_max=-1), dict(n_rows=-1), dict(n_rows=2 ** 31), dict(work_bytes=-1),
           dict(top=0), dict(top=65), dict(top=-3), dict(n_fields=0), dict(n_fields=9), dict(n_fields=-1),
           dict(n_codes=np.array([3, -1, 5], dtype=np.int64)), dict(n_codes=np.array([3, 2 ** 31, 5], dtype=np.int64)),
           dict(work_bytes=call.work_bytes - 1), dict(work_bytes=0),
           dict(n_cons=2 ** 24), dict(n_cons=(2 ** 24 - 1) // 3 + 1)]
    for over in bad:
        assert raw(**over) == -1, over  # AMDR_EINVAL
        assert lib.amdr_last_error(), over
    torch.cuda.synchronize()
    assert all((o == SENTINEL).all() for o in call.outs) and (call.work == 0x5a).all()
    assert raw() == 0  # the same arguments, unchanged, are a valid call
    assert_equal(call.fetch(), FC.evaluate(**case), "after the refusals")
    # the host twin: the same sizes, and the table's contents
    for top in (0, 65):
        with pytest.raises(nat.NativeError):
            ws.facet_counts(case["scope_ptr"], case["rows"], case["codes"], case["n_codes"], top)
    with pytest.raises(nat.NativeError):
        ws.facet_counts(case["scope_ptr"], case["rows"], case["codes"], [3, -1, 5], 4)
    codes = np.zeros((1, 6), dtype=np.int32)
    for sp, rows, msg in (([1, 2], [0, 1], "scope_ptr"), ([0, 2, 1], [0, 1], "scope_ptr"), ([0, 2], [1, 1], "ascending"),
                          ([0, 2], [4, 1], "ascending"), ([0, 2], [-1, 4], "ascending"), ([0, 2], [1, 6], "ascending")):
        with pytest.raises(nat.NativeError, match=msg):
            ws.facet_counts(np.asarray(sp, np.int64), np.asarray(rows, np.int64), codes, [2], 3, rows_max=2)


def test_a_captured_call_replays_over_a_rewritten_table(nat):
    """One linear graph: the call's three launches.  Between the replays the scope table is rewritten in place; both results
    must be exact, which they are only if the call zeroes its counters itself, on every replay."""
    rng = np.random.default_rng(401)
    n_rows, n_cons = 2 * FC.T + 100, 5
    cap = n_cons * (FC.T + 50)
    codes = np.stack([FC.column("skewed", 9, n_rows, rng), FC.column("random", FC.B + 5, n_rows, rng)])

    def variant(seed):
        r = np.random.default_rng(seed)
        lens = r.integers(0, FC.T + 50, size=n_cons)
        lens[int(r.integers(0, n_cons))] = FC.T + 50  # one scope of two tiles
        sp, rows = FC.table(lens, n_rows, r)
        return {"scope_ptr": sp, "rows": rows, "codes": codes, "n_codes": [9, FC.B + 5], "top": 5}
    first = variant(1)
    call = DeviceCall(nat, first, rows_max=FC.T + 50, rows_cap=cap)

    def write(case):
        call.sp.copy_(torch.from_numpy(case["scope_ptr"]))
        call.rows[:case["rows"].size].copy_(torch.from_numpy(case["rows"]))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):  # an eager run first, outside the capture
        call()
    side.synchronize()
    assert_equal(call.fetch(), FC.evaluate(**first), "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    g0 = nat.workspace_growths()
    for seed in (2, 3):
        case = variant(seed)
        write(case)
        graph.replay()
        got = call.fetch()
        assert nat.workspace_growths() == g0
        want = FC.evaluate(**case)
        assert want[0].sum() > FC.T and not np.array_equal(want[0], FC.evaluate(**first)[0])
        assert_equal(got, want, f"replay {seed}")

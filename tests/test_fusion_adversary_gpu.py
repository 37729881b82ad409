"""Fusion (all four forms launch_fuse chooses from), rerank blend and compaction — csrc/fuse.hip, csrc/fuse_core.hpp —
against oracle/fusion.py in BATCHES whose queries differ inside one wave (tests/fusion_adversary.py).  Every comparison is
== on ids, masks and counts and on the bit patterns of all nine values, whole rows including the padding past the union;
order inside exact ties is first appearance on both sides, so nothing is set aside.  Both call forms: _native.fuse (host
pointers, every channel float64) and _native.fuse_device on torch tensors (dense / ColBERT float32, BM25 float64, row2uid
maps).  The device outputs carry guard rows behind them, which must come back untouched."""
import ctypes as C
import math

import numpy as np
import pytest

import fusion_adversary as FA

pytestmark = pytest.mark.gpu

GUARD = 64  # rows behind every device output
SENT_I, SENT_V = -777, -123.25


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


def params(nat, kn, min_final=-math.inf):
    return nat.make_fuse_params(method=kn["fusion_method"], rrf_k=kn["rrf_k"], alpha=kn["rrf_alpha"], w_dense=kn["dense_weight"],
                                w_bm25=kn["bm25_weight"], w_colbert=kn["colbert_weight"], min_final_score=min_final)


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, copy=True)).to(dev())


class Guarded:
    """A device output of `rows` rows with GUARD sentinel rows behind it."""

    def __init__(self, rows, width, dtype, fill):
        import torch
        self.rows, self.width, self.fill = rows, width, fill
        self.t = torch.full(((rows + GUARD) * width,), fill, dtype=dtype, device=dev())

    def ptr(self):
        return self.t.data_ptr()

    def host(self, shape, what):
        a = self.t.cpu().numpy()
        assert (a[self.rows * self.width:] == self.fill).all(), (what, "wrote past the end of an output")
        return a[:self.rows * self.width].reshape(shape).copy()


def fuse_host(nat, batch, p):
    return nat.fuse(p, batch.nq, *batch.host_args())


def fuse_dev(nat, batch, p, maps=(None, None, None), what=None):
    import torch
    nq, mo = batch.nq, batch.max_out
    keep, chans = [], []
    for c, k in enumerate(batch.shape):
        if k == 0:
            chans.append(None)
            continue
        ids = to_dev(batch.ids[c])
        sc = to_dev(batch.scores[c], np.float64 if c == 1 else np.float32)
        m = to_dev(maps[c]) if maps[c] is not None else None
        keep += [ids, sc, m]
        chans.append((ids.data_ptr(), sc.data_ptr(), k, m.data_ptr() if m is not None else 0))
    oi, ov = Guarded(nq * mo, 1, torch.int64, SENT_I), Guarded(nq * mo, FA.NVALS, torch.float64, SENT_V)
    om, oc = Guarded(nq * mo, 1, torch.int32, SENT_I), Guarded(nq, 1, torch.int32, SENT_I)
    nat.fuse_device(p, nq, *chans, oi.ptr(), ov.ptr(), om.ptr(), oc.ptr())
    torch.cuda.synchronize()
    return (oi.host((nq, mo), what), ov.host((nq, mo, FA.NVALS), what), om.host((nq, mo), what), oc.host((nq,), what))


def check_both(nat, batch, kn, min_final, exp, what):
    p = params(nat, kn, min_final)
    FA.assert_record(fuse_host(nat, batch, p), exp, (what, "amdr_fuse"))
    FA.assert_record(fuse_dev(nat, batch, p, what=what), exp, (what, "amdr_fuse_device"))


# ---- a. routes x batch sizes x methods ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FA.SHAPES, ids=["-".join(map(str, s)) for s in FA.SHAPES])
def test_routes_batches_methods(nat, shape):
    """Every form of launch_fuse, nq of every remainder of 4 and 2, all four methods; queries of different kinds side by
    side in a wave (disjoint / heavily overlapping ids, ragged lengths, an all -1 middle channel, an all -1 query)."""
    full = FA.mixed_batch(shape)
    for method in FA.METHODS:
        kn = FA.knobs(method)
        exp = FA.expected_mixed(shape, method)
        for nq in FA.NQS:
            check_both(nat, full.head(nq), kn, FA.MIN_FINAL, FA.head(exp, nq), (shape, method, nq))


# ---- b. row2uid maps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FA.ROUTE_SHAPES, ids=str)
def test_row2uid_maps(nat, shape):
    """A different map per channel, and every way of leaving channels without one: the oracle on the mapped lists."""
    batch, maps = FA.map_batch(shape)
    for use in ((1, 1, 1), (1, 0, 1), (0, 1, 0), (1, 0, 0), (0, 0, 1)):
        mp = tuple(m if u else None for m, u in zip(maps, use))
        lists = FA.mapped_lists(batch.lists, mp)
        for method in FA.METHODS:
            kn = FA.knobs(method)
            exp = FA.expected_arrays(lists, kn, FA.MIN_FINAL, batch.max_out)
            got = fuse_dev(nat, batch, params(nat, kn, FA.MIN_FINAL), mp, what=(shape, use, method))
            FA.assert_record(got, exp, (shape, use, method))


# ---- c. knob and value edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FA.ROUTE_SHAPES, ids=str)
def test_knob_edges(nat, shape):
    batch = FA.mixed_batch(shape).head(5)
    for name, kn in FA.KNOB_EDGES:
        exp = FA.expected_arrays(batch.lists, kn, FA.MIN_FINAL, batch.max_out)
        check_both(nat, batch, kn, FA.MIN_FINAL, exp, (shape, name))


@pytest.mark.parametrize("shape", FA.ROUTE_SHAPES, ids=str)
def test_min_final_edges(nat, shape):
    """min_final exactly at a candidate's score (>= keeps it), one double above, +inf, -inf."""
    batch = FA.mixed_batch(shape).head(5)
    for method in FA.METHODS:
        kn = FA.knobs(method)
        if method == "rrf_norm_blend":
            edges = FA.min_final_edges(batch.lists, kn)
        else:  # (rrf totals tie: the edge is taken at whatever score the middle hit of query 0 has)
            hits = FA.F.fuse(*batch.lists[0], kn)
            s = hits[len(hits) // 2]["score"]
            edges = (s, math.nextafter(s, math.inf), math.inf, -math.inf)
        counts = []
        for mf in edges:
            exp = FA.expected_arrays(batch.lists, kn, mf, batch.max_out)
            counts.append(exp[3])
            check_both(nat, batch, kn, mf, exp, (shape, method, mf))
        assert counts[0][0] > counts[1][0] and (counts[2] == 0).all() and counts[3].tolist() == batch.unions()


@pytest.mark.parametrize("shape", FA.ROUTE_SHAPES, ids=str)
def test_value_edges(nat, shape):
    """Channel spans 2^-40 / 2^-39 around _minmax's 1e-12, one-entry channels, negative scores, flat channels."""
    batch = FA.value_edge_batch(shape)
    for method in FA.METHODS:
        kn = FA.knobs(method)
        check_both(nat, batch, kn, FA.MIN_FINAL, FA.expected_arrays(batch.lists, kn, FA.MIN_FINAL, batch.max_out), (shape, method))


# ---- d. exact ties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FA.ROUTE_SHAPES, ids=str)
def test_exact_ties_keep_first_appearance(nat, shape):
    batch = FA.tie_batch(shape)
    for method in FA.METHODS:
        kn = FA.knobs(method)
        exp = FA.expected_arrays(batch.lists, kn, -math.inf, batch.max_out)
        check_both(nat, batch, kn, -math.inf, exp, (shape, method))


# ---- e. lists that are not descending -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FA.ROUTE_SHAPES, ids=str)
def test_lists_that_are_not_descending(nat, shape):
    """Rank = list position, min / max over the list (oracle keep_order).  All queries shuffled; then exactly one query per
    packed wave — whose wave-mates lose the descending-list shortcut with it and must still give, bit for bit, what they give
    in the all-sorted batch."""
    base = FA.mixed_batch(shape).head(8)
    one = [1, 6]  # <16>: wave 0 segment 1, wave 1 segment 2; <32>: wave 0 segment 1, wave 3 segment 0
    for method in FA.METHODS:
        kn = FA.knobs(method)
        p = params(nat, kn, FA.MIN_FINAL)
        sorted_got = fuse_host(nat, base, p)
        FA.assert_record(sorted_got, FA.head(FA.expected_mixed(shape, method), 8), (shape, method, "sorted"))
        for name, queries in (("all", range(8)), ("one per wave", one)):
            batch = FA.shuffled(base, queries)
            exp = FA.expected_arrays(batch.lists, kn, FA.MIN_FINAL, batch.max_out, keep_order=True)
            got = fuse_host(nat, batch, p)
            FA.assert_record(got, exp, (shape, method, name, "amdr_fuse"))
            FA.assert_record(fuse_dev(nat, batch, p, what=(shape, method, name)), exp, (shape, method, name, "amdr_fuse_device"))
            if queries is one:
                rest = [q for q in range(8) if q not in one]
                FA.assert_record([a[rest] for a in got], [a[rest] for a in sorted_got], (shape, method, "wave-mates"))


# ---- f. route independence ------------------------------------------------------------------------------------------------------
def test_route_independence(nat):
    """One set of lists walked through <16> -> <32> -> fuse_kernel by an all -1 ColBERT block: the first U rows and the count
    do not move, and every form equals the oracle."""
    base = FA.mixed_batch((5, 5, 0)).head(7)
    for method in FA.METHODS:
        kn = FA.knobs(method)
        p = params(nat, kn, FA.MIN_FINAL)
        narrow = fuse_host(nat, base, p)
        exp = FA.expected_arrays(base.lists, kn, FA.MIN_FINAL, base.max_out)
        FA.assert_record(narrow, exp, (method, "narrow"))
        seen = {FA.route(base.max_out, 0)}
        for kc in (6, 7, 22, 23, 60):  # max_out 16, 17, 32, 33, 70
            wide = base.widened(kc)
            seen.add(FA.route(wide.max_out, 0))
            for form, got in (("host", fuse_host(nat, wide, p)), ("device", fuse_dev(nat, wide, p, what=(method, kc)))):
                for name, g, n in zip(("ids", "vals", "mask"), got, narrow):
                    g = g[:, :base.max_out]
                    assert np.array_equal(FA.bits(g), FA.bits(n)) if name == "vals" else np.array_equal(g, n), (method, kc, form, name)
                assert (got[0][:, 10:] == -1).all() and (got[2][:, 10:] == 0).all() and (FA.bits(got[1][:, 10:]) == 0).all()
                assert np.array_equal(got[3], narrow[3]), (method, kc, form)
        assert seen == {FA.P16, FA.P32, FA.LONG_REG}


# ---- g. rerank blend ----------------------------------------------------------------------------------------------------------
def rerank_host(nat, rec, ce, beta):
    ids, vals, mask, count = (a.copy() for a in rec)
    rer = nat.rerank_blend(count, ids, vals, mask, ce, beta)
    return ids, vals, mask, rer


def rerank_dev(nat, rec, ce, beta, what):
    import torch
    nq, mo = rec[0].shape
    top_n = ce.shape[1]
    bufs = [Guarded(nq * mo, 1, torch.int64, SENT_I), Guarded(nq * mo, FA.NVALS, torch.float64, SENT_V),
            Guarded(nq * mo, 1, torch.int32, SENT_I), Guarded(nq * mo, 2, torch.float64, SENT_V)]
    for b, a in zip(bufs, rec[:3]):
        b.t[:a.size] = to_dev(a).reshape(-1)
    count, ce_d = to_dev(rec[3]), to_dev(ce)
    nat.rerank_blend_device(nq, mo, count.data_ptr(), bufs[0].ptr(), bufs[1].ptr(), bufs[2].ptr(), ce_d.data_ptr(), top_n, beta,
                            bufs[3].ptr())
    torch.cuda.synchronize()
    return (bufs[0].host((nq, mo), what), bufs[1].host((nq, mo, FA.NVALS), what), bufs[2].host((nq, mo), what),
            bufs[3].host((nq, mo, 2), what))


def assert_rerank(got, exp, rec, what):
    count = rec[3]
    for name, g, e in zip(("ids", "vals", "mask", "rerank"), got, exp):
        gb, eb = (FA.bits(g), FA.bits(e)) if name in ("vals", "rerank") else (g, e)
        at = FA.first_difference(gb, eb)
        assert at is None, (what, name, "first difference at", at, "got", g[at], "expected", e[at])
    for q in range(len(count)):  # rows [count, max_out) are the input's, and out_rerank is NaN outside the re-ranked hits
        c = int(count[q])
        assert np.array_equal(got[0][q, c:], rec[0][q, c:]) and np.array_equal(got[2][q, c:], rec[2][q, c:]), (what, q)
        assert np.array_equal(FA.bits(got[1][q, c:]), FA.bits(rec[1][q, c:])), (what, q)
        assert np.isnan(got[3][q, c:]).all(), (what, q)


@pytest.mark.parametrize("shape", FA.RERANK_SHAPES, ids=[str(sum(s)) for s in FA.RERANK_SHAPES])
def test_rerank_blend(nat, shape):
    """max_out 1 / 20 / 64 / 65 / 768 (768: more than 48 KiB of LDS, the function-attribute path); counts from 0 to max_out
    inside a batch; top_n below, at and above counts and above max_out; beta 0 / 0.35 / 1; CE scores random, all equal,
    spanning 2^-40 / 2^-39, duplicated.  The inputs are part a's fused records under rrf (tied fused scores: with beta = 0 the
    order comes from the two-stage stable sort alone, and a blended candidate ties with tail hits) and under the blend."""
    mo = sum(shape)
    for method in ("rrf", "rrf_norm_blend"):
        full = FA.rerank_input(shape, method)
        for top_n in FA.top_ns(full[3], mo):
            ce_full = FA.ce_scores(FA.NQ_MAX, top_n)
            for beta in FA.BETAS:
                exp_full = FA.expected_rerank(*full, ce_full, top_n, beta)
                for nq in FA.RERANK_NQS:
                    rec, ce, exp = FA.head(full, nq), ce_full[:nq], FA.head(exp_full, nq)
                    what = (mo, method, top_n, beta, nq)
                    assert_rerank(rerank_host(nat, rec, ce, beta), exp, rec, what + ("amdr_rerank_blend",))
                    assert_rerank(rerank_dev(nat, rec, ce, beta, what), exp, rec, what + ("amdr_rerank_blend_device",))


# ---- h. compaction ------------------------------------------------------------------------------------------------------------
def test_fuse_compact(nat):
    """The first w hits of every query, -1 / 0 / 0 past min(count, w), the clipped counts: against the numpy restatement of
    tests/test_hybrid_step.py, at nq * w on both sides of the blocks of 256 threads."""
    import torch
    from test_hybrid_step import compact
    mo = FA.COMPACT_MAX_OUT
    for nq, w in FA.COMPACT_CASES:
        rec = FA.compact_record(nq)
        exp = compact(*rec, w)
        ins = [to_dev(a) for a in rec]
        outs = [Guarded(nq * w, 1, torch.int64, SENT_I), Guarded(nq * w, 1, torch.float64, SENT_V),
                Guarded(nq * w, 1, torch.int32, SENT_I), Guarded(nq, 1, torch.int32, SENT_I)]
        nat.fuse_compact_device(nq, mo, w, *(t.data_ptr() for t in ins), *(o.ptr() for o in outs))
        torch.cuda.synchronize()
        got = [o.host(s, (nq, w)) for o, s in zip(outs, ((nq, w), (nq, w), (nq, w), (nq,)))]
        for name, g, e in zip(("rows", "scores", "mask", "count"), got, exp):
            e = np.asarray(e)
            assert g.dtype == e.dtype and g.shape == e.shape, (nq, w, name, g.dtype, e.dtype)
            assert np.array_equal(FA.bits(g) if name == "scores" else g, FA.bits(e) if name == "scores" else e), (nq, w, name)


# ---- i. argument errors -------------------------------------------------------------------------------------------------------
def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def raw_fuse(nat, p, nq, ks, outs):
    """amdr_fuse called directly, so that a refused call's outputs can be inspected."""
    chans = []
    for k in ks:
        ids = np.zeros((max(nq, 1), k), dtype=np.int64) if k else None
        sc = np.ones((max(nq, 1), k), dtype=np.float64) if k else None
        chans += [_p(ids, C.c_int64), _p(sc, C.c_double), C.c_int32(k)]
        outs.setdefault("keep", []).extend([ids, sc])
    rc = nat.load().amdr_fuse(C.byref(p) if p is not None else None, C.c_int32(nq), *chans, _p(outs["ids"], C.c_int64),
                              _p(outs["vals"], C.c_double), _p(outs["mask"], C.c_int32), _p(outs["count"], C.c_int32))
    nat._check(rc, "amdr_fuse")


def sentinel_outs(nq, mo):
    return {"ids": np.full((nq, mo), SENT_I, np.int64), "vals": np.full((nq, mo, FA.NVALS), SENT_V), "mask": np.full((nq, mo), SENT_I, np.int32),
            "count": np.full((nq,), SENT_I, np.int32)}


def untouched(outs):
    return all((outs[n] == (SENT_V if n == "vals" else SENT_I)).all() for n in ("ids", "vals", "mask", "count"))


def test_fuse_argument_errors(nat):
    good = nat.make_fuse_params()
    bad_method = nat.FuseParams(4, 60, 0.5, 0.6, 0.4, 0.35, -math.inf)
    for what, p, nq, ks in (("all channels empty", good, 2, (0, 0, 0)), ("a depth of 257", good, 2, (257, 0, 0)),
                            ("a depth of 257 (colbert)", good, 2, (4, 4, 257)), ("method 4", bad_method, 2, (4, 4, 0)),
                            ("method -1", nat.FuseParams(-1, 60, 0.5, 0.6, 0.4, 0.35, 0.0), 2, (4, 4, 0)),
                            ("null params", None, 2, (4, 4, 0)), ("nq < 0", good, -1, (4, 4, 0))):
        outs = sentinel_outs(2, 600)
        with pytest.raises(nat.NativeError):
            raw_fuse(nat, p, nq, ks, outs)
        assert untouched(outs), what
    outs = sentinel_outs(2, 8)
    raw_fuse(nat, good, 0, (4, 4, 0), outs)  # nq = 0: nothing to do
    assert untouched(outs)
    # the device form checks the same arguments before it touches the device
    import torch
    o = Guarded(0, 1, torch.float64, SENT_V)
    for p, nq, d in ((good, 2, (0, 0, 0, 0)), (good, 2, (o.ptr(), o.ptr(), 257, 0)), (bad_method, 2, (o.ptr(), o.ptr(), 4, 0))):
        with pytest.raises(nat.NativeError):
            nat.fuse_device(p, nq, d, None, None, o.ptr(), o.ptr(), o.ptr(), o.ptr())
    nat.fuse_device(good, 0, (o.ptr(), o.ptr(), 4, 0), None, None, o.ptr(), o.ptr(), o.ptr(), o.ptr())
    torch.cuda.synchronize()
    o.host((0,), "fuse_device refusals")


def test_rerank_and_compact_argument_errors(nat):
    import torch
    lib = nat.load()
    nq, mo = 2, 4
    ids, vals = np.full((nq, mo), SENT_I, np.int64), np.full((nq, mo, FA.NVALS), SENT_V)
    mask, count = np.full((nq, mo), SENT_I, np.int32), np.full((nq,), 2, np.int32)
    ce, rer = np.ones((nq, 4)), np.full((nq, mo, 2), SENT_V)

    def host(nq_, mo_, top_n):
        nat._check(lib.amdr_rerank_blend(nq_, mo_, _p(count, C.c_int32), _p(ids, C.c_int64), _p(vals, C.c_double),
                                         _p(mask, C.c_int32), _p(ce, C.c_double), top_n, 0.35, _p(rer, C.c_double)), "amdr_rerank_blend")

    g = [Guarded(nq * mo, 1, torch.int64, SENT_I), Guarded(nq * mo, FA.NVALS, torch.float64, SENT_V),
         Guarded(nq * mo, 1, torch.int32, SENT_I), Guarded(nq * mo, 2, torch.float64, SENT_V)]
    cnt_d, ce_d = to_dev(count), to_dev(ce)

    def device(nq_, mo_, top_n):
        nat.rerank_blend_device(nq_, mo_, cnt_d.data_ptr(), g[0].ptr(), g[1].ptr(), g[2].ptr(), ce_d.data_ptr(), top_n, 0.35, g[3].ptr())

    def all_untouched():
        torch.cuda.synchronize()
        assert (ids == SENT_I).all() and (vals == SENT_V).all() and (mask == SENT_I).all() and (rer == SENT_V).all()
        for b, wd in zip(g, (1, FA.NVALS, 1, 2)):
            assert (b.t.cpu().numpy() == b.fill).all()

    for call in (host, device):
        for mo_, top_n in ((0, 4), (769, 4), (mo, 0), (mo, -3)):
            with pytest.raises(nat.NativeError):
                call(nq, mo_, top_n)
            all_untouched()
        with pytest.raises(nat.NativeError):
            call(-1, mo, 4)
        call(0, mo, 4)  # nq = 0: nothing to do
        all_untouched()

    rec = [to_dev(a) for a in FA.compact_record(nq, mo)]
    outs = [Guarded(nq * mo, 1, torch.int64, SENT_I), Guarded(nq * mo, 1, torch.float64, SENT_V),
            Guarded(nq * mo, 1, torch.int32, SENT_I), Guarded(nq, 1, torch.int32, SENT_I)]

    def compact(nq_, mo_, w):
        nat.fuse_compact_device(nq_, mo_, w, *(t.data_ptr() for t in rec), *(o.ptr() for o in outs))

    for nq_, mo_, w in ((nq, mo, 0), (nq, mo, mo + 1), (nq, 0, 1), (-1, mo, 1)):
        with pytest.raises(nat.NativeError):
            compact(nq_, mo_, w)
    compact(0, mo, 1)  # nq = 0: nothing to do
    torch.cuda.synchronize()
    for o in outs:
        assert (o.t.cpu().numpy() == o.fill).all()

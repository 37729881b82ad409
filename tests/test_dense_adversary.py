"""CPU self-checks of tests/dense_adversary.py: the integer builders keep the 2^24 budget and are summation-order free,
the tie structure and the position coverage are as described, the real-valued builders' gaps hold at every listed
shape, three deliberately wrong model kernels fail the expectations, and form_of switches at the route's thresholds."""
import numpy as np
import pytest

import dense_adversary as DA


def _case(family, n, d, nq, k):
    X, a, meta = DA.integer_X(family, n, d)
    Q, b = DA.integer_Q(family, n, d, nq, k)
    S, es, ei = DA.integer_expect(X, a, Q, b, k)
    return X, Q, S, es, ei, meta


@pytest.mark.parametrize("family", DA.INT_FAMILIES)
@pytest.mark.parametrize("n,d,nq,k", [(257, 260, 9, 10), (65, 4, 33, 68), (1025, 768, 5, 256), (33, 1024, 129, 1)])
def test_integer_builders_are_order_free(family, n, d, nq, k):
    X, Q, S, es, ei, _ = _case(family, n, d, nq, k)  # (asserts the 2^24 budget)
    rng = np.random.default_rng(d + n)
    for t in range(3):  # fp32 arithmetic in three shuffled K orders: the oracle's bits
        got = DA.fp32_scores_in_order(X, Q, rng.permutation(d))
        assert DA.bits_equal(got, S.astype(np.float32)), (family, t)
    assert es.shape == (nq, k) and np.all(ei[:, min(k, n):] == -1) and np.all(es[:, min(k, n):] == -DA.FLT_MAX)
    assert np.all(ei[:, :min(k, n)] >= 0)


def test_the_budget_assertion_can_fail():
    X = np.full((2, 8), 4096, dtype=np.float32)
    Q = np.full((1, 8), 1024, dtype=np.float32)
    with pytest.raises(AssertionError):
        DA.assert_integer_budget(X, Q)
    with pytest.raises(AssertionError):
        DA.assert_integer_budget(X * 0.5 + 0.25, Q)


@pytest.mark.parametrize("form", DA.FORMS)
def test_position_probe_covers_every_position(form):
    whole = set()
    for n, d, nq, k in DA.position_cases(form):
        assert DA.form_of(n, d, nq, k, DA.pins_of(form, nq)) == form, (n, d, nq, k)
        c = DA.position_case(n, d, nq, k)  # (asserts it too)
        assert c["covered"] == set(range(c["positions"])) and c["positions"] == min(n, d), (n, d, nq, k)
        assert np.array_equal(np.count_nonzero(c["X"], axis=1), np.ones(n, dtype=np.int64))
        if n >= d:
            whole.add(d)
    # every matrix shape of the form's cases is probed, and every d it admits on a matrix with a row at all d positions
    assert {(n, d) for n, d, _, _ in DA.position_cases(form)} >= {(n, d) for n, d, _, _ in DA.cases(form)}
    assert whole == set(DA.coverage(form)["d"][1]), (form, sorted(whole))


def test_position_case_refuses_a_batch_that_leaves_positions_out():
    with pytest.raises(AssertionError):
        DA.position_case(1025, 768, 9, 10)


@pytest.mark.parametrize("n,d,k", [(1025, 256, 10), (4099, 64, 10), (16385, 128, 256), (257, 768, 10)])
def test_cancel_ties_straddle_a_tile_boundary_and_the_cut(n, d, k):
    X, Q, S, es, ei, meta = _case("cancel", n, d, 9, k)
    zero, pos = meta["zero"], meta["pos"]
    assert np.all(S[:, zero] == 0) and np.all(S[:, pos] > 0)
    rest = np.setdiff1d(np.arange(n), np.concatenate([zero, pos]))
    assert np.all(S[:, rest] < 0)
    assert len(pos) < k <= len(pos) + len(zero)  # the k-th place is inside the group that ties at exactly 0
    assert len(pos) + len(zero) > k  # ... and the group goes on behind the cut
    for q in range(9):
        tied = ei[q][es[q] == 0]
        assert tied.size and np.array_equal(tied, zero[:tied.size])  # ties: the lower ids, in order
        assert es[q, k - 1] == 0
    # one run of the group crosses a 32-row tile boundary inside the answer
    lo = zero[:k - len(pos)]
    assert np.any((lo[:-1] // 32 != lo[1:] // 32) & (lo[1:] - lo[:-1] == 1)), lo
    for q in range(9):
        assert np.array_equal(ei[q, len(pos):], lo)
    # the large terms really are large: partial sums reach 2^15 before they cancel
    assert np.abs(X).max() >= 1 << 15


def test_scaled_families_stay_normal_and_their_subnormal_products_are_fp32_values():
    for fam in DA.INT_FAMILIES[3:]:
        X, Q, S, es, ei, _ = _case(fam, 65, 128, 5, 10)
        a, b = DA._scale_of(fam)
        assert DA.stats_finite(X)
        if (a, b) in DA.SUBNORMAL_SCALES:
            tiny = float(np.finfo(np.float32).tiny)
            assert -149 <= a + b <= -140 and np.abs(S).max() < 2.0 ** -121
            # every product of small components is an fp32 subnormal; at 2^-149 every score is one, at 2^-140 the sums
            # cross into the normal range
            assert 3 * 3 * 2.0 ** (a + b) < tiny and np.any(np.abs(S) < tiny)
            assert np.all(np.abs(S) < tiny) if a + b == -149 else np.any(np.abs(S) >= tiny)


@pytest.mark.parametrize("kind", DA.REAL_KINDS)
def test_real_builders_gaps_hold_at_every_listed_shape(kind):
    for form, shapes in DA.PLANTED_SHAPES.items():
        for n, d, nq, k in shapes:
            if n > 4200 and kind != "mixture":
                continue  # (the GPU test builds them all; here the largest once, with rows of every kind)
            assert DA.form_of(n, d, nq, k, DA.pins_of(form, nq)) == form, (form, n, d, nq, k)
            c = DA.planted_case(kind, n, d, nq, k)  # (asserts separation and gap)
            assert c["ids"].shape == (nq, k)
    for form, shapes in DA.FULL_SHAPES.items():
        for n, d, nq in shapes:
            assert n <= 256 and DA.form_of(n, d, nq, n, DA.pins_of(form, nq)) == form, (form, n, d, nq)
            X, Q = DA.real_case(kind, n, d, nq)
            B = DA.bound_matrix(X, Q)  # (asserts: no underflow, no overflow)
            assert np.all(B > 0)


def test_real_kinds_are_what_they_say():
    X, Q = DA.real_case("spread", 64, 256, 4)
    e = np.log2(np.abs(X))
    assert e.min() < -18 and e.max() > 18 and np.all(e.max(axis=1) - e.min(axis=1) > 30)
    X, Q = DA.real_case("large", 64, 256, 4)
    assert np.allclose(np.linalg.norm(X.astype(np.float64), axis=1), 1e6, rtol=1e-3)
    X, Q = DA.real_case("small", 64, 256, 4)
    assert np.allclose(np.linalg.norm(X.astype(np.float64), axis=1), 1e-12, rtol=1e-3)
    DA.real_case("cancel", 64, 256, 4)  # (asserts ratio ~ 50 and the sign at the constructed pairs)
    X, Q = DA.real_case("mixture", 256, 128, 4)
    nrm = np.linalg.norm(X.astype(np.float64), axis=1)
    assert nrm.min() < 1e-11 and nrm.max() > 1e5
    with pytest.raises(AssertionError):
        DA.bound_matrix(np.full((1, 4), 1e-30, np.float32), np.full((1, 4), 1e-5, np.float32))


# ---- sensitivity: the expectations must be able to fail -------------------------------------------------------------------
@pytest.mark.parametrize("model", list(DA.WRONG_MODELS))
@pytest.mark.parametrize("d", [64, 260, 768])
def test_wrong_model_kernels_miss_the_integer_expectations(model, d):
    n, nq, k = 1025, 129, 10  # nq k >= d <= n: the position probe covers every K position
    missed, full = {}, {}
    for fam in ("position", "wide", "cancel"):
        X, Q, S, es, ei, _ = _case(fam, n, d, nq, k)
        if fam == "position":
            DA.position_case(n, d, nq, k)  # (this batch covers every position)
        got = DA.WRONG_MODELS[model](X, Q)
        gs, gi = DA.oracle_topk(got.astype(np.float64), k)
        missed[fam] = not (np.array_equal(gi, ei) and DA.bits_equal(gs, es))  # what a search sees
        full[fam] = not DA.bits_equal(got, S.astype(np.float32))  # what the full-matrix probe (score_rows) sees
    # the probes made for each error find it, in the top-k and in the full matrix
    meant = ("wide", "cancel") if model == "fp16 operands" else ("position", "wide")
    for fam in meant:
        assert missed[fam] and full[fam], (fam, missed, full)
    # the correct fp32 model passes the same comparison
    X, Q, S, es, ei, _ = _case("wide", n, d, nq, k)
    gs, gi = DA.oracle_topk(DA.fp32_scores_in_order(X, Q, np.arange(d)).astype(np.float64), k)
    assert np.array_equal(gi, ei) and DA.bits_equal(gs, es)


@pytest.mark.parametrize("model", list(DA.WRONG_MODELS))
@pytest.mark.parametrize("kind", DA.REAL_KINDS)
def test_wrong_model_kernels_exceed_the_real_bound(model, kind):
    n, d, nq = 255, 768, 5
    X, Q = DA.real_case(kind, n, d, nq)
    S, B = DA.exact_scores(X, Q), DA.bound_matrix(X, Q)
    ids = np.tile(np.arange(n), (nq, 1))
    assert DA.check_bound(DA.WRONG_MODELS[model](X, Q), ids, S, B) > 1.0
    ok = DA.check_bound(DA.fp32_scores_in_order(X, Q, np.random.default_rng(1).permutation(d)), ids, S, B)
    assert ok <= 1.0, ok  # a real fp32 evaluation, in a shuffled order, is inside


def test_wrong_model_kernels_miss_the_planted_ids_or_the_bound():
    c = DA.planted_case("mixture", 1025, 768, 33, 10)
    for model, f in DA.WRONG_MODELS.items():
        got = f(c["X"], c["Q"])
        gs, gi = DA.oracle_topk(got.astype(np.float64), 10)
        assert not np.array_equal(gi, c["ids"]) or DA.check_bound(gs, gi, c["S"], c["bound"]) > 1.0, model
    gs, gi = DA.oracle_topk(DA.fp32_scores_in_order(c["X"], c["Q"], np.arange(768)).astype(np.float64), 10)
    assert np.array_equal(gi, c["ids"]) and DA.check_bound(gs, gi, c["S"], c["bound"]) <= 1.0


def test_full_view_check_rejects_a_wrong_order():
    X, Q = DA.real_case("large", 33, 64, 2)
    S, B = DA.exact_scores(X, Q), DA.bound_matrix(X, Q)
    s, i = DA.oracle_topk(S, 33)
    assert DA.check_full_view(s, i, S, B) <= 1.0
    with pytest.raises(AssertionError):
        DA.check_full_view(s[:, ::-1].copy(), i[:, ::-1].copy(), S, B)
    j = i.copy()
    j[0, 0] = j[0, 1]
    with pytest.raises(AssertionError):
        DA.check_full_view(s, j, S, B)


# ---- the route ------------------------------------------------------------------------------------------------------------
def test_form_of_at_the_route_thresholds():
    f = DA.form_of
    none = {}
    # few queries: one wave per (query, row) up to 16 384 rows, the scan beyond
    for nq in (1, 4):
        assert f(16384, 128, nq, 10, none) == DA.ROWWAVES and f(16385, 128, nq, 10, none) == DA.SCAN
    # a dimension outside the MFMA forms: the same at any batch size
    for d in (4, 60, 68, 260):
        for nq in (5, 96, 129):
            assert f(16384, d, nq, 10, none) == DA.ROWWAVES and f(16385, d, nq, 10, none) == DA.SCAN
    # from 5 queries: tiles; from 96: the panel kernel (pinned off: tiles; pinned on: from the first batched size)
    assert f(1025, 768, 4, 10, none) == DA.ROWWAVES and f(1025, 768, 5, 10, none) == DA.TILES
    assert f(1025, 768, 95, 10, none) == DA.TILES and f(1025, 768, 96, 10, none) == DA.PANEL
    assert f(1025, 768, 96, 10, {"AMDR_DENSE_PANEL": "0"}) == DA.TILES
    assert f(1025, 768, 5, 10, {"AMDR_DENSE_PANEL": "1"}) == DA.PANEL
    # the exact two-level form, pinned: from 2 k tiles
    two = DA.PINS[DA.TWOLEVEL]
    assert f(32 * 19 + 1, 64, 5, 10, two) == DA.TWOLEVEL and f(32 * 19, 64, 5, 10, two) == DA.TILES
    assert f(32 * 19 + 1, 64, 4, 10, two) == DA.ROWWAVES
    assert f(4099, 64, 96, 10, dict(two, AMDR_DENSE_TWO_LEVEL="0")) == DA.PANEL
    # the fp16 first pass, pinned: d % 128 == 0, 2 (k + max(k, 96) + 1) tiles, k <= 127, finite statistics
    hi = DA.PINS[DA.HI]
    assert f(32 * 213 + 1, 128, 5, 10, hi) == DA.HI and f(32 * 213, 128, 5, 10, hi) == DA.TILES
    assert f(6917, 192, 5, 10, hi) == DA.TILES and f(6917, 128, 5, 10, hi, finite=False) == DA.TILES
    assert f(16385, 128, 5, 127, hi) == DA.HI and f(16385, 128, 5, 128, hi) == DA.TILES
    assert f(6917, 128, 5, 10, dict(hi, AMDR_DENSE_TWO_LEVEL="0")) == DA.TILES
    # unpinned, neither two-level form is taken by a matrix that the caches hold
    assert f(16385, 128, 129, 1, none) == DA.PANEL
    # the two-pass form of a short corpus: from AMDR_DENSE_SMALL_HI_MIN queries, <= 1 024 rows, k <= 12, d % 128 == 0
    sm = lambda nq: DA.pins_of(DA.SMALL, nq)
    assert f(1024, 128, 96, 12, sm(96)) == DA.SMALL and f(1025, 128, 96, 12, sm(96)) == DA.PANEL
    assert f(1024, 128, 96, 13, sm(96)) == DA.PANEL and f(1024, 192, 96, 12, sm(96)) == DA.PANEL
    assert f(1024, 128, 95, 12, sm(96)) == DA.TILES and f(1024, 128, 4200, 12, none) == DA.SMALL
    assert f(1024, 128, 96, 12, dict(sm(96), AMDR_DENSE_SMALL_HI="0")) == DA.PANEL
    assert f(1024, 128, 96, 12, sm(96), finite=False) == DA.PANEL


def test_every_listed_edge_occurs_in_every_form_that_admits_it():
    print(DA.coverage_table())
    for form in DA.FORMS:
        for axis, (hit, adm) in DA.coverage(form).items():
            assert hit == adm, (form, axis, hit, adm)
        for n, d, nq, k in DA.cases(form):
            assert DA.form_of(n, d, nq, k, DA.pins_of(form, nq)) == form
    # what the forms admit, as the route's thresholds say
    cov = {f: DA.coverage(f) for f in DA.FORMS}
    assert cov[DA.SCAN]["n"][1] == [16385] and cov[DA.SCAN]["d"][1] == list(DA.DS) and cov[DA.ROWWAVES]["d"][1] == list(DA.DS)
    assert cov[DA.TILES]["d"][1] == [d for d in DA.DS if d % 64 == 0] == cov[DA.PANEL]["d"][1]
    assert cov[DA.HI]["d"][1] == [128, 256, 768, 1024] == cov[DA.SMALL]["d"][1]
    assert set(cov[DA.PANEL]["nq"][1]) >= {96, 97, 129} and set(cov[DA.TILES]["nq"][1]) >= {5, 8, 9, 31, 32, 33, 95, 96, 97, 129}
    assert set(cov[DA.SCAN]["nq"][1]) == set(DA.NQS) == set(cov[DA.ROWWAVES]["nq"][1])


def test_plan_texts_map_to_forms():
    assert DA.form_from_plan("dense_scan_topk_kernel<NQ=4> grid=8x1 + merge_parts_kernel") == DA.SCAN
    assert DA.form_from_plan("dense_all_scores_kernel (one wave per query x row) + scores_slab_topk_kernel") == DA.ROWWAVES
    assert DA.form_from_plan("dense_mfma_scores_kernel query-tiles-in-LDS grid=1x1 queries_per_launch=5 + x") == DA.TILES
    assert DA.form_from_plan("dense_mfma_scores_kernel tile-maxima grid=1x1 queries_per_launch=5 two-level: top-1") == DA.TWOLEVEL
    assert DA.form_from_plan("dense_panel_scores_kernel nb=8 parts=1 blocks=1 queries_per_launch=96 + x") == DA.PANEL
    assert DA.form_from_plan("dsh_scores_kernel fp16 first pass ...; exact form: dense_panel_scores_kernel") == DA.SMALL
    assert DA.form_from_plan("dense_hi_image_tilemax_kernel (resident fp16 image) fp16 first pass") == DA.HI
    with pytest.raises(AssertionError):
        DA.form_from_plan("empty index")

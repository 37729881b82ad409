"""CPU self-checks of tests/maxsim_adversary.py: every case of the GPU driver holds its exactness certificate and equals
the fp64 oracle bit for bit, the tie shares and the two-pass separations are as described, form_of switches where
ms_route does, the coverage table is complete, and every wrong-kernel model changes the expectations of the family
named for it."""
import numpy as np
import pytest

import maxsim_adversary as MA
import rounding_adversary as RA

CASES = {c["name"]: c for c in MA.cases()}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_certificate_and_oracle(name):
    """view() asserts the certificate; the oracle's fp64 scores, rounded to fp32, are the expected matrices — of both
    arithmetic forms, except in the both-wide families, where only the fp32-input forms return the oracle's value."""
    from oracle import maxsim as OM
    case = CASES[name]
    c = MA.case_view(case)
    n = len(c["doc_ptr"]) - 1
    assert c["exp_split"].shape == c["exp_f32"].shape == (case["nq"], n) and c["Q"].shape[1] == case["q_len"]
    ref = OM.maxsim_scores(c["Q"], c["D"], c["doc_ptr"])
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) or case["family"] in ("both_wide", "rounded_lo")
    assert MA.same_scores(ref.astype(np.float32), c["exp_f32"])
    if case["family"] in ("both_wide", "rounded_lo"):
        assert np.any(_bits(c["exp_split"]) != _bits(c["exp_f32"]))
        assert np.max(np.abs(c["exp_split"].astype(np.float64) - ref)) <= 2.0 ** -21  # the dropped lo.lo term and one rounding
    else:
        assert MA.same_scores(ref.astype(np.float32), c["exp_split"])
    if case["family"] == "integers" and not (case["sd"] or case["sq"]):
        assert np.all(np.abs(c["D"]) <= 15) and np.abs(c["D"]).max() == 15 and np.all(np.abs(c["Q"]).max(axis=(1, 2)) == 15)
        assert np.array_equal(ref, np.round(ref)) and np.abs(ref).max() < 2 ** 20


def test_the_certificate_can_fail():
    c = MA.view("integers", None, 9, 2, 17)
    with pytest.raises(AssertionError):  # 24-bit components: the split is not exact
        MA.split_expected(c["D"] + np.float32(2.0 ** -20), c["doc_ptr"], c["Q"])
    with pytest.raises(AssertionError):  # a budget of 2^12 units is too small for sums of 128 products of 4-bit integers
        MA.split_expected(c["D"], c["doc_ptr"], c["Q"], limit=1 << 12)
    with pytest.raises(AssertionError):
        MA.f32_expected(c["D"], c["doc_ptr"], c["Q"], limit=1 << 12)
    w = MA.view("both_wide", None, None, 9, 1)
    with pytest.raises(AssertionError):  # both sides wide: the fold rounds
        MA.split_expected(w["D"], w["doc_ptr"], w["Q"], fold_exact=True)
    r = MA.view("rounded_lo", None, None, 9, 1)
    with pytest.raises(AssertionError):
        MA.split_expected(r["D"], r["doc_ptr"], r["Q"], fold_exact=False, split_exact=True)


@pytest.mark.parametrize("name", [n for n, c in sorted(CASES.items()) if c["family"] in ("integers", "short") and not c["sd"] and not c["sq"]])
def test_at_least_half_of_the_cuts_fall_inside_a_tie_group(name):
    case = CASES[name]
    c = MA.case_view(case)
    ks = list(MA.case_depths(case, c).values())
    n = len(c["doc_ptr"]) - 1
    if any(k < n for k in ks):
        assert MA.tie_share(c["exp_split"], ks) >= 0.5, (name, ks)


def test_short_store_profile():
    c = MA.short_store()
    assert len(c["doc_ptr"]) - 1 == MA.SELECT_ROWS_MAX + 1 and c["doc_ptr"][-1] <= 40000
    lens = np.diff(c["doc_ptr"])
    assert lens.min() == 1 and lens.max() == 12


@pytest.mark.parametrize("kind", ["listed", "overflow", "mixed"])
@pytest.mark.parametrize("nq", [16, 17])
def test_two_pass_statuses(kind, nq):
    """By the fp64 model of the candidate rule (RA.maxsim_eps, RA.ms_cand_cap): a listed query's k + 4 best are more than
    2 eps above the rest, an overflowed query has more than ms_cand_cap(k) documents tie exactly at its cut; in the mixed
    batch the two alternate, so every pass-1 wave (queries 2 w, 2 w + 1) holds one of each."""
    c = MA.view("twopass", kind, None, nq, 32)
    n = len(c["doc_ptr"]) - 1
    for k in (MA.TP_K, 1):
        st = MA.twopass_status(c, k, nq)
        assert 4 * k <= n and MA.form_of(n, nq, k, True, MA.P_DEF) == MA.TWOPASS
        want = {"listed": np.ones(nq), "overflow": -np.ones(nq), "mixed": np.where(np.arange(nq) % 2 == 1, 1, -1)}[kind]
        assert np.array_equal(st, want), (kind, k, st)
    assert RA.ms_cand_cap(MA.TP_K) == 64 and MA.TP_CLONES > 64
    # an overflowed query's list is the lowest ids of the tie group
    _, ids = MA.topk_expected(c["exp_split"], MA.TP_K)
    for b in np.nonzero(MA.twopass_status(c, MA.TP_K, nq) < 0)[0]:
        tied = np.nonzero(c["exp_split"][b] == c["exp_split"][b].max())[0]
        assert tied.size == MA.TP_CLONES and np.array_equal(ids[b], tied[:MA.TP_K])


def test_form_of_against_hand_checked_routes():
    F, H, O, D7 = MA.P_F32, MA.P_DEF, MA.P_ONE, {"AMDR_MAXSIM_DOCS": "7"}
    table = [
        # n_docs, nq, k, want_topk, pins, finite -> form
        (25, 1, 1, True, H, True, MA.PAIRHALF), (25, 7, 1, True, H, True, MA.PAIRHALF), (25, 7, 1, False, H, True, MA.PAIRHALF),
        (25, 7, 1, True, F, True, MA.PAIRF32), (25, 7, 10, True, H, False, MA.PAIRF32), (25, 7, 1, False, F, True, MA.PAIRF32),
        (25, 8, 1, True, F, True, MA.BLOCKED), (25, 33, 30, True, F, True, MA.BLOCKED), (25, 8, 1, False, H, False, MA.BLOCKED),
        (25, 8, 6, True, H, False, MA.BLOCKED),
        (25, 8, 1, False, H, True, MA.RING), (25, 8, 6, True, O, True, MA.RING), (25, 8, 7, True, H, True, MA.RING),
        (25, 8, 25, True, H, True, MA.RING), (25, 8, 28, True, H, True, MA.RING), (3, 8, 1, True, H, True, MA.RING),
        (25, 8, 6, True, H, True, MA.TWOPASS), (24, 8, 6, True, H, True, MA.TWOPASS), (23, 8, 6, True, H, True, MA.RING),
        (4, 8, 1, True, H, True, MA.TWOPASS), (2049, 8, 65, True, D7, True, MA.TWOPASS), (640, 9, 160, True, H, True, MA.TWOPASS),
        (640, 9, 161, True, H, True, MA.RING), (640, 7, 10, True, H, True, MA.PAIRHALF),
        (640, 8, 10, True, {"AMDR_MAXSIM_TWOPASS": "1"}, True, MA.TWOPASS), (640, 8, 10, True, {"AMDR_MAXSIM_F16X3": "1"}, True, MA.TWOPASS),
        (640, 8, 10, True, {**F, **O}, True, MA.BLOCKED),
        (8 * 65535 + 1, 8, 1, True, F, True, MA.PAIRF32),  # more blocks than a grid's y holds: one wave per pair
    ]
    for n, nq, k, topk, pins, finite, want in table:
        assert MA.form_of(n, nq, k, topk, pins, finite) == want, (n, nq, k, topk, pins, finite)
    assert MA.form_from_plan("maxsim_hi2_ring_kernel split-fp16 two-pass top-k (k <= n_docs / 4): ... full score rows: "
                             "maxsim_scores_ring_kernel") == MA.TWOPASS
    assert MA.form_from_plan("maxsim_scores_kernel fp32-input (v_mfma_f32_16x16x4_f32) + rowscores_topk_kernel") == MA.PAIRF32
    assert MA.form_from_plan("maxsim_scores_h_kernel split-fp16 (hi + lo/2048, ...)") == MA.PAIRHALF


def test_coverage_table():
    """Every listed edge occurs in every form that admits it."""
    tab = MA.coverage_table()
    for form in MA.FORMS:
        want = MA.admitted(form)
        for axis, edges in want.items():
            assert edges <= tab[form][axis], (form, axis, sorted(edges - tab[form][axis], key=str))
    assert set(MA.DOC_LENS) == set(np.diff(MA.integers_store()["doc_ptr"]).tolist())
    for form in (MA.PAIRF32, MA.PAIRHALF):
        assert all(q < MA.K_MSQ for q in tab[form]["nq"])
    for form in (MA.BLOCKED, MA.RING, MA.TWOPASS):
        assert all(q >= MA.K_MSQ for q in tab[form]["nq"])


def test_position_store_decides_every_slot():
    c = MA.position_store()
    comps, rows, qrows = MA.position_coverage(c)
    assert comps == set(range(128)) and rows == set(range(32)) and qrows == set(range(32))
    S = MA.view("position", None, None, 8, 32)["exp_split"]
    for b in range(8):  # 32 distinct positive scores per query, the other 96 documents tie at 0
        pos = S[b][S[b] > 0]
        assert pos.size == 32 and np.unique(pos).size == 32 and np.sum(S[b] == 0) == 96
    assert {int(d) for d in range(128) if np.nonzero(c["D"][c["doc_ptr"][d]:c["doc_ptr"][d + 1]])[0][0] >= 32} == set(range(96, 128))


def test_bait_stores():
    for R in MA.BAIT_REMAINDERS:
        c = MA.view("bait", R, None, 9, 32)
        ptr, D, Q = c["doc_ptr"], c["D"], c["Q"]
        n = len(ptr) - 1
        assert np.diff(ptr)[-1] == R and n == 2 * len(MA.BAIT_REMAINDERS) + 1
        for d in list(range(0, n - 1, 2)) + [n - 1]:
            sims = Q.reshape(-1, 128).astype(np.float64) @ D[ptr[d]:ptr[d + 1]].astype(np.float64).T
            assert np.all(sims < 0) and all(np.unique(r).size == r.size for r in sims)
            assert np.all(sims.argmax(axis=1) == sims.shape[1] - 1)  # the least negative: the document's last token
            if d < n - 1:
                bait = Q.reshape(-1, 128).astype(np.float64) @ D[ptr[d + 1]:ptr[d + 1] + 64].astype(np.float64).T
                assert ptr[d + 2] - ptr[d + 1] == 64 and bait.min() >= 100
        assert np.array_equal(c["exp_split"][:, n - 1], c["exp_split"][:, 2 * MA.BAIT_REMAINDERS.index(R)])


MODEL_VIEWS = {"integers": ("integers", None, 9, 3, 17), "position": ("position", None, None, 8, 32), "bait": ("bait", 17, None, 2, 31),
               "wide": ("wide", None, None, 3, 32), "wide_rev": ("wide_rev", None, None, 3, 32),
               "both_wide": ("both_wide", None, None, 9, 1), "rounded_lo": ("rounded_lo", None, None, 9, 1)}
CAUGHT_BY = {"max0": "bait", "mask_gt": "bait", "nomask": "bait", "early16": "bait", "dropk": "position", "qrows": "integers",
             "lo_trunc": "rounded_lo", "cross_al": "wide", "cross_ah": "wide_rev", "inv1024": "wide", "tie_high": "integers",
             "cut_first": "integers"}


@pytest.mark.parametrize("family", sorted(MODEL_VIEWS))
def test_the_model_as_written_returns_the_expected_bits(family):
    c = MA.view(*MODEL_VIEWS[family])
    assert MA.same_scores(MA.model_scores(c["D"], c["doc_ptr"], c["Q"]), c["exp_split"])


@pytest.mark.parametrize("fault", MA.FAULTS)
def test_a_wrong_kernel_changes_the_expectations(fault):
    assert set(CAUGHT_BY) == set(MA.FAULTS)
    family = CAUGHT_BY[fault]
    if fault in MA.SCORE_FAULTS:
        c = MA.view(*MODEL_VIEWS[family])
        got = MA.model_scores(c["D"], c["doc_ptr"], c["Q"], fault)
        assert not MA.same_scores(got, c["exp_split"]), fault
        n = c["exp_split"].shape[1]
        if family in ("bait", "position"):  # ... and the ids of a full list with them
            assert not np.array_equal(MA.topk_expected(got, n)[1], MA.topk_expected(c["exp_split"], n)[1])
        return
    c = MA.view("integers", None, 25, 9, 32)
    hit = 0
    for k in MA.depths(c["exp_split"], 25).values():
        s, i = MA.topk_expected(c["exp_split"], k)
        fs, fi = MA.model_topk(c["exp_split"], k, fault)
        assert MA.same_scores(fs, s)  # the scores alone do not tell
        hit += int(not np.array_equal(fi, i))
    assert hit >= 3, fault


def test_an_exact_split_cannot_tell_a_truncated_lo():
    """Why rounded_lo exists: on exactly split inputs truncation and rounding of lo are the same function."""
    for family in ("wide", "both_wide"):
        c = MA.view(*MODEL_VIEWS[family])
        assert MA.same_scores(MA.model_scores(c["D"], c["doc_ptr"], c["Q"], "lo_trunc"), c["exp_split"])


@pytest.mark.parametrize("kind", MA.NONFINITE_KINDS)
def test_non_finite_rule(kind):
    """The rule of include/amdretrieval.h, applied: never a NaN; a NaN token in a longer document is ignored, a one-token
    NaN document scores -inf (q_len >= 2 times -FLT_MAX), inf x 0 is a NaN similarity (ignored), +inf wins its row;
    every other document scores what it scores in the store with the bad token zeroed."""
    c, bad, clean = MA.nonfinite_case(kind, 9)
    want = MA.nonfinite_expected(c["D"], c["doc_ptr"], c["Q"])
    ref = MA.f32_expected(clean, c["doc_ptr"], c["Q"])
    others = np.arange(want.shape[1]) != bad
    assert np.array_equal(_bits(want[:, others]), _bits(ref[:, others])) and not np.isfinite(c["D"]).all()
    if kind == "nan-document":
        assert np.all(want[:, bad] == -np.inf)
    elif kind.endswith("-nonzero"):
        assert np.all(want[:, bad] == np.inf)
    else:  # the bad token drops out: the document scores its other tokens
        lo, hi = int(c["doc_ptr"][bad]), int(c["doc_ptr"][bad + 1])
        keep = np.array([t for t in range(lo, hi) if np.isfinite(c["D"][t]).all()])
        sub = MA.f32_expected(c["D"][keep], np.array([0, keep.size]), c["Q"])
        assert np.array_equal(_bits(want[:, bad]), _bits(sub[:, 0]))
    s, i = MA.topk_expected(want, 12)
    assert np.all(i[:, 9:] == -1) and np.all(s[:, 9:] == -MA.FLT_MAX)
    if want[0, bad] == np.inf:
        assert np.all(i[:, 0] == bad)
    if want[0, bad] == -np.inf:
        assert np.all(i[:, 8] == bad)

"""The MaxSim two-pass top-k (csrc/maxsim.hip) where its candidate rule `first-pass score >= T - 2 eps_q` and its kernels'
thresholds had no test: every case compares (a) the fp64 oracle, (b) the one-pass form pinned with AMDR_MAXSIM_TWOPASS=0
and (c) the two-pass form — asserted to be the two-pass form — and wants (c) ids == the oracle's where the construction
fixes them and (c) scores == (b) bit for bit (RA.ms_forms / RA.ms_check, the driver test_rounding_adversary_gpu.py uses).

A. Scale range.  The inversion store (fp16 ranks competitors above the exact top-k; only the bound keeps the latter among
   the candidates) times exact powers of two, 2^-90 .. 2^70: the bound's norms are taken on the scaled operands, so it has
   no range of its own.  (Taken on the raw fp32 components they squared to 0 below ~2^-75 — every true top-k document
   lost — and to infinity above ~2^63; tests/test_rounding_adversary.py shows on the CPU that the collapsed bound loses a
   target of every query.)  Past fp32's own range (the product of the two unscales no normal number) there is no bound
   and the two forms still agree.
B. Degenerate queries inside a two-pass batch: an all-zero, all-NaN, one-infinity, one-NaN query shares its pass-1 wave
   with a healthy one and leaves every other query's ids and score bits alone; what it returns itself is stated.
C. Shape edges on random unit rows: documents of 14 .. 32 tiles (the items kernel's last cost class, the last tile of the
   store reading into the padding), corpus sizes on and across the select kernel's row-selector thresholds, depths on
   and across the candidate-list capacities, the route boundary 4 k == n_docs, overflowed and listed queries in one wave,
   documents that are candidates of exactly 8, 9, 16, 17, 24 queries (1, 2, 2, 3, 3 items), one handle across calls of
   different shapes."""
import numpy as np
import pytest

import rounding_adversary as RA

pytestmark = pytest.mark.gpu

TOL = 1e-4  # north_star's bar, against the fp64 oracle
FLT_MAX = np.float32(3.4028234663852886e38)
DOCS7 = [{}, {"AMDR_MAXSIM_DOCS": "7"}]


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    return _native


# ---- references, computed once ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inversion():
    """(k, nc) -> the inversion store of 8 (k + nc) documents, 16 queries of 16 tokens."""
    return {(k, nc): RA.maxsim_inversion(np.random.default_rng(910), 16, k, groups=8, reps=2, nc=nc)
            for k, nc in ((1, 4), (10, 12))}


@pytest.fixture(scope="module")
def short():
    c = RA.maxsim_short_docs(np.random.default_rng(2100), 2100, 24)
    c["exact"] = RA.exact_maxsim(c["Q"], c["D"], c["doc_ptr"])
    return c


@pytest.fixture(scope="module")
def depth():
    c = RA.maxsim_depth_docs(np.random.default_rng(1100), 9)
    c["exact"] = RA.exact_maxsim(c["Q"], c["D"], c["doc_ptr"])
    return c


def _vs_oracle(s, i, exact, k, rows=None):
    """As test_maxsim_matches_oracle: k distinct ids, every reported score within TOL of the oracle's score of the
    reported id, ranks equal to the oracle's wherever its neighbouring scores are more than 2 TOL apart — at most 10 %
    of the positions are not."""
    es, ei = RA.topk_exact(exact, k)
    skipped = 0
    rows = range(len(s)) if rows is None else rows
    for b in rows:
        assert len(set(i[b].tolist())) == k and i[b].min() >= 0 and i[b].max() < exact.shape[1]
        assert np.max(np.abs(s[b] - exact[b, i[b]])) <= TOL, b
        sep = RA.oracle_rank_mask(es[b], TOL)
        assert np.all((i[b] == ei[b])[sep]), b
        skipped += int((~sep).sum())
    assert skipped <= 0.10 * k * len(rows), (skipped, k)


# ---- A. scale range ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sd,sq", RA.MAXSIM_SCALE_PAIRS)
@pytest.mark.parametrize("k,nc", [(1, 4), (10, 12)])
def test_scale_range_on_the_inversion_store(nat, monkeypatch, inversion, k, nc, sd, sq):
    c = RA.maxsim_scaled(inversion[(k, nc)], sd, sq)
    assert len(c["doc_ptr"]) - 1 == 8 * (k + nc) >= 4 * k and c["doc_ptr"][-1] <= 8 * (k + nc) * (16 + 39)
    RA.ms_check(nat, monkeypatch, c["D"], c["doc_ptr"], c["Q"], k, c["top"], DOCS7)


@pytest.mark.parametrize("sd,sq", [(-70, -70), (64, 72)])
def test_scales_past_fp32_take_no_bound(nat, monkeypatch, inversion, sd, sq):
    """The product of the two unscales is below 2^-126 / above 2^127: the scores themselves leave fp32's range (they
    flush to multiples of 2^-149, or overflow), no margin can be stated in fp32 — every document is re-scored and the
    two-pass form returns the one-pass form's ids and bits, whatever they are."""
    c = RA.maxsim_scaled(inversion[(10, 12)], sd, sq)
    d_scale, q_scale = RA.maxsim_scales(c["Q"], c["D"])
    un = 1.0 / (d_scale * q_scale)
    assert np.all(un < 2.0 ** -126) or np.all(un >= 2.0 ** 128)
    RA.ms_forms(nat, monkeypatch, c["D"], c["doc_ptr"], c["Q"], 10, DOCS7)


# ---- B. degenerate queries ---------------------------------------------------------------------------------------------------
def _degenerate(Q, kind):
    Q = Q.copy()
    if kind == "zero":
        Q[5] = 0.0
    elif kind == "nan":
        Q[5] = np.nan
    elif kind == "inf":
        Q[5, 3, 17] = np.inf
    elif kind == "nan-token0":
        Q[5, 0, 40] = np.nan
    return Q


@pytest.fixture(scope="module")
def healthy(nat, inversion):
    """The unmodified batch on the (10, 12) inversion store, unscaled and x 2^70: (case, scores, ids) of the one-pass form
    (test_scale_range_on_the_inversion_store holds the two-pass form to the same bits)."""
    out = {}
    mp = pytest.MonkeyPatch()
    try:
        for sd in (0, 70):
            c = RA.maxsim_scaled(inversion[(10, 12)], sd, 0)
            s, i = RA.ms_check(nat, mp, c["D"], c["doc_ptr"], c["Q"], 10, c["top"], [{}])
            out[sd] = (c, s, i)
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("kind,sd", [("zero", 0), ("zero", 70), ("nan", 0), ("inf", 0), ("nan-token0", 0), ("nan-token0", 70)])
def test_degenerate_query_in_a_two_pass_batch(nat, monkeypatch, healthy, kind, sd):
    """Query 5 (the second query of pass 1's wave 2, beside query 4) is degenerate.  First the neighbours: the other
    fifteen return the ids and bits of the healthy batch, in the one-pass form and in every two-pass variant.  Then
    query 5 itself, the same in both forms: the zero query ids 0 .. k-1 at score 0.0 (every document ties: lower id
    first) — also on the store x 2^70, where a bound from raw norms was 0 x inf; a query with a NaN or an infinity has no
    bound (its norm sum is not finite), so every document is re-scored in the full form and the final top-k ranks what
    the one-pass form ranks ("Queries without a bound"): k hits, here every document at the same score —
    the NaN products never win a lane's maximum, which stays at -FLT_MAX and swamps the sum — so ids 0 .. k-1."""
    k = 10
    c, s0, i0 = healthy[sd]
    n_docs = len(c["doc_ptr"]) - 1
    Q = _degenerate(c["Q"], kind)
    others = np.arange(len(Q)) != 5
    # what a non-finite query 5 scores on every document: each token with a NaN product contributes -FLT_MAX times the two
    # unscales (the query's from its finite components; 1 if it holds an infinity or nothing finite), which absorbs the
    # other tokens' sums (< 2^12 unscales against an ulp of 2^104 unscales) or overflows to -inf
    d_scale, _ = RA.maxsim_scales(c["Q"], c["D"])
    fin = np.abs(Q[5][np.isfinite(Q[5])]).astype(np.float64)
    un_q = 1.0 if kind == "inf" or fin.size == 0 else 1.0 / float(RA.pow2_scale(fin.max()))
    v = -float(FLT_MAX) * (un_q / d_scale) * (Q.shape[1] if kind == "nan" else 1)
    want = np.float32(-np.inf) if v < -float(FLT_MAX) else np.float32(v)
    two = []
    s, i = RA.ms_forms(nat, monkeypatch, c["D"], c["doc_ptr"], Q, k, RA.MS_VARIANTS, rows=others, two_pass=two)
    assert np.array_equal(i[others], i0[others]) and np.array_equal(i0[others], c["top"][others])
    assert np.array_equal(s[others].view(np.uint32), s0[others].view(np.uint32))
    print(f"OBS degenerate {kind} sd={sd}: one pass ids {i[5].tolist()} scores {s[5].tolist()}")
    for s2, i2 in two:
        print(f"OBS degenerate {kind} sd={sd}: two-pass ids {i2[5].tolist()} scores {s2[5].tolist()}")
    for s5, i5 in [(s[5], i[5])] + [(s2[5], i2[5]) for s2, i2 in two]:
        if kind == "zero":
            assert i5.tolist() == list(range(k)) and np.all(s5 == 0.0)
            continue
        hit = i5 >= 0
        assert np.all(i5[hit] < n_docs) and len(set(i5[hit].tolist())) == int(hit.sum())
        assert np.all(i5[~hit] == -1) and np.all(s5[~hit] == -FLT_MAX)
        assert not np.any(hit[1:] & ~hit[:-1])  # paddings behind the hits
        assert np.array_equal(i5, i[5]) and np.array_equal(s5.view(np.uint32), s[5].view(np.uint32))  # both forms: the same
        assert i5.tolist() == list(range(k)) and np.all(s5 == want), (s5, want)


# ---- C. shape edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,q_len", [(9, 32), (16, 17)])
def test_long_documents(nat, monkeypatch, nq, q_len):
    k = 5
    c = RA.maxsim_long_docs(np.random.default_rng(1000 + nq), nq, q_len)
    exact = RA.exact_maxsim(c["Q"], c["D"], c["doc_ptr"])
    _, ei = RA.topk_exact(exact, k)
    assert len(set(ei.ravel().tolist()) & set(c["long"].tolist())) >= 5 and np.diff(c["doc_ptr"])[-1] == 513
    s, i = RA.ms_forms(nat, monkeypatch, c["D"], c["doc_ptr"], c["Q"], k, RA.MS_VARIANTS)
    _vs_oracle(s, i, exact, k)
    assert i[0, 0] == 79  # planted at the store's very last token, alone in its tile


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("n_docs", [640, 641, 1280, 1281, 2048, 2049, 2100])
def test_selector_thresholds(nat, monkeypatch, short, n_docs, k):
    D, ptr = RA.maxsim_prefix(short, n_docs)
    assert ptr[-1] <= 15000
    s, i = RA.ms_forms(nat, monkeypatch, D, ptr, short["Q"][:8], k, [{}])
    _vs_oracle(s, i, short["exact"][:8, :n_docs], k)


@pytest.mark.parametrize("k", [32, 33, 64, 65, 128, 256])
def test_depth_thresholds(nat, monkeypatch, depth, k):
    assert len(depth["doc_ptr"]) - 1 == 1100 and depth["doc_ptr"][-1] <= 15000
    s, i = RA.ms_forms(nat, monkeypatch, depth["D"], depth["doc_ptr"], depth["Q"], k, [{}])
    _vs_oracle(s, i, depth["exact"], k)


def test_route_boundary(nat, monkeypatch, short):
    n, nq = 40, 8
    D, ptr = RA.maxsim_prefix(short, n)
    Q, exact = short["Q"][:nq], short["exact"][:nq, :n]
    rows = (nq * n * 4 + 255) // 256 * 256
    assert nat.maxsim_workspace_plan(n, True, nq, 10, nq, 10)[1] > rows  # 4 k == n_docs: two passes
    assert nat.maxsim_workspace_plan(n, True, nq, 11, nq, 11)[1] == rows  # one pass inside
    s, i = RA.ms_forms(nat, monkeypatch, D, ptr, Q, 10, RA.MS_VARIANTS)
    _vs_oracle(s, i, exact, 10)
    out = {}
    for pin in (None, "0"):
        if pin:
            monkeypatch.setenv("AMDR_MAXSIM_TWOPASS", pin)
        idx = nat.MaxSimIndex(D, ptr)
        out[pin] = idx.search(Q, 11)
        idx.close()
    monkeypatch.delenv("AMDR_MAXSIM_TWOPASS")
    assert np.array_equal(out[None][1], out["0"][1]) and np.array_equal(out[None][0].view(np.uint32), out["0"][0].view(np.uint32))
    _vs_oracle(out[None][0], out[None][1], exact, 11)


def test_overflowed_and_listed_queries_in_one_wave(nat, monkeypatch):
    k = 10
    c = RA.maxsim_mixed_overflow(np.random.default_rng(77))
    Q, D, ptr = c["Q"], c["D"], c["doc_ptr"]
    approx, eps = RA.model_maxsim_hi(Q, D, ptr), RA.maxsim_eps(Q, D)
    n_cand = np.array([len(RA.candidates(approx[b], eps[b], k)) for b in range(16)])
    aimed = np.zeros(16, bool)
    aimed[c["aimed"]] = True
    assert np.all(n_cand[aimed] > 2 * RA.ms_cand_cap(k)) and np.all(n_cand[~aimed] < RA.ms_cand_cap(k) / 2), n_cand
    assert np.all(aimed[0::2]) and not np.any(aimed[1::2])  # queries 2 w and 2 w + 1 share a pass-1 wave
    s, i = RA.ms_forms(nat, monkeypatch, D, ptr, Q, k, RA.MS_VARIANTS)
    exact = RA.exact_maxsim(Q, D, ptr)
    # the random queries rank like the oracle; an aimed query's hits are near-ties by construction (the duplicates differ
    # in the 4th decimal of a token): scores within TOL, and nothing reported that is TOL below the oracle's k-th best
    _vs_oracle(s, i, exact, k, rows=np.nonzero(~aimed)[0])
    es, _ = RA.topk_exact(exact, k)
    for b in np.nonzero(aimed)[0]:
        assert len(set(i[b].tolist())) == k and set(i[b].tolist()) <= set(c["cluster"].tolist())
        assert np.max(np.abs(s[b] - exact[b, i[b]])) <= TOL and np.all(exact[b, i[b]] >= es[b, -1] - TOL)


def test_documents_shared_by_many_queries(nat, monkeypatch):
    """A document that is a candidate of c queries is re-scored in ceil(c / 8) items: c = 8, 9, 16, 17, 24 copies of one
    query in a batch of 24 (tests/test_rounding_adversary.py: the planted document is a candidate of exactly the
    copies).  Every copy returns the bits that the query returns in a batch that holds it once, and so do the others."""
    k = 10
    c = RA.maxsim_shared(np.random.default_rng(24))
    D, ptr, pool = c["D"], c["doc_ptr"], c["pool"]
    once = RA.maxsim_shared_batch(pool, 1)
    exact = RA.exact_maxsim(once, D, ptr)
    s1, i1 = RA.ms_forms(nat, monkeypatch, D, ptr, once, k, [{}])
    _vs_oracle(s1, i1, exact, k)
    assert np.all(i1[0, 0] == RA.MS_SHARED_DOC)
    for copies in (8, 9, 16, 17, 24):
        s, i = RA.ms_forms(nat, monkeypatch, D, ptr, RA.maxsim_shared_batch(pool, copies), k, [{}])
        # position p of this batch is position max(0, p - copies + 1) of the batch that holds query 0 once
        src = np.maximum(0, np.arange(24) - copies + 1)
        assert np.array_equal(i, i1[src]), copies
        assert np.array_equal(s.view(np.uint32), s1[src].view(np.uint32)), copies


def test_one_handle_across_calls_of_different_shapes(nat, monkeypatch, short):
    """Search A (24 queries, k = 10), B (8 queries, k = 33: another workspace layout over the same bytes), A again on ONE
    index: the second A returns the first's bits (per-document counters reset, no stale lists, flags or items), and
    each equals the one-pass form on a fresh index."""
    n = 640
    D, ptr = RA.maxsim_prefix(short, n)
    QA, QB = short["Q"], short["Q"][8:16]
    for nq, k in ((24, 10), (8, 33)):
        assert nat.maxsim_workspace_plan(n, True, nq, k, nq, k)[1] > (nq * n * 4 + 255) // 256 * 256
    idx = nat.MaxSimIndex(D, ptr)
    assert "two-pass" in idx.plan_info(24) and "two-pass" in idx.plan_info(8)
    a1 = idx.search(QA, 10)
    b1 = idx.search(QB, 33)
    a2 = idx.search(QA, 10)
    idx.close()
    assert np.array_equal(a1[1], a2[1]) and np.array_equal(a1[0].view(np.uint32), a2[0].view(np.uint32))
    monkeypatch.setenv("AMDR_MAXSIM_TWOPASS", "0")
    idx = nat.MaxSimIndex(D, ptr)
    for (s, i), Q, k in ((a1, QA, 10), (b1, QB, 33)):
        s_one, i_one = idx.search(Q, k)
        assert np.array_equal(i, i_one) and np.array_equal(s.view(np.uint32), s_one.view(np.uint32)), k
    idx.close()
    monkeypatch.delenv("AMDR_MAXSIM_TWOPASS")
    _vs_oracle(a1[0], a1[1], short["exact"][:, :n], 10)
    _vs_oracle(b1[0], b1[1], short["exact"][8:16, :n], 33)

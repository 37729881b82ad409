"""The worst-case rounding data of tests/rounding_adversary.py is what it claims to be (CPU only): every generated
component rounds by >= 0.45 fp16 ulp in its intended direction, the modelled first-pass error comes within a constant
factor of the kernels' bound without crossing it, a flushed subnormal operand or a smaller bound would cross it, the
inversion cases really reverse the order across the cut in fp16 while the exact order holds in fp32, and the candidate
counts stay inside the fast paths' limits — so the GPU tests built on this data cannot pass vacuously."""
import numpy as np
import pytest

import rounding_adversary as RA


def _dir_ok(vals, away):
    sh = RA.rounding_shift(vals)
    nz = vals != 0
    return np.all(sh[nz] >= 0.45) if away else np.all(sh[nz] <= -0.45)


def test_generators_round_half_an_ulp_in_the_chosen_direction():
    rng = np.random.default_rng(0)
    for away in (False, True):
        b = rng.integers(1, 15, size=5000)
        v = RA.normal_values(b, rng.integers(0, 1000, 5000), np.full(5000, away), rng, rng.choice([-1.0, 1.0], 5000))
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)  # exact in fp32
        assert _dir_ok(v, away)
        sub = RA.subnormal_values(5000, rng, away=away, sign=rng.choice([-1.0, 1.0], 5000))
        assert np.all(np.abs(sub) < RA.MIN_NORMAL) and _dir_ok(sub, away)
        assert np.array_equal(sub.astype(np.float32).astype(np.float64), sub)
    # relative size of the rounding in the normal binades: ~2^-11
    v = RA.normal_values(np.full(100, 3), np.zeros(100, int), np.zeros(100, bool), rng)
    rel = (v - v.astype(np.float16)) / v
    assert np.all(rel > 0.45 * 2.0 ** -11) and np.all(rel < 2.0 ** -11)


def _scaled_dirs(X, Q):
    x_scale, q_scale, _ = RA.dense_scales(X, Q)
    return np.asarray(X, np.float64) * x_scale, np.asarray(Q, np.float64) * q_scale[:, None]


@pytest.mark.parametrize("d", [128, 768, 1024])
@pytest.mark.parametrize("away", [False, True])
def test_dense_coherent_case_comes_close_to_the_bound(d, away):
    rng = np.random.default_rng(d + away)
    X, Q, row = RA.dense_coherent(rng, d, 24, away=away)
    Xs, Qs = _scaled_dirs(X, Q)
    assert np.all(np.abs(Xs).max() < 1) and np.abs(Xs).max() >= 0.5
    assert _dir_ok(Xs, away) and _dir_ok(Qs, away)
    err = np.abs(RA.model_dense_hi(X, Q) - RA.exact_dense(X, Q))
    eps = RA.dense_eps(X, Q)
    ratio = err / eps[:, None]
    assert ratio.max() <= 1.0
    pred = 1 / 1.125 * 2.0 ** -10 / (2.0 ** -10 + 2 * (d + 8) * 2.0 ** -24)  # 0.81 at d = 768
    assert 0.7 <= ratio.max() <= pred, (ratio.max(), pred)
    assert ratio[np.arange(24), row].min() >= 0.7


@pytest.mark.parametrize("d,mirror", [(768, False), (768, True), (1024, False), (1024, True)])
def test_dense_subnormal_case_exceeds_eps_only_under_ftz(d, mirror):
    rng = np.random.default_rng(d + mirror)
    X, Q, row = RA.dense_subnormal(rng, d, 16, mirror)
    Xs, Qs = _scaled_dirs(X, Q)
    small = Qs if not mirror else Xs
    assert np.mean(np.abs(small) < RA.MIN_NORMAL) > 0.99
    exact, eps = RA.exact_dense(X, Q), RA.dense_eps(X, Q)
    ok = np.abs(RA.model_dense_hi(X, Q) - exact) / eps[:, None]
    ftz = np.abs(RA.model_dense_hi(X, Q, ftz=True) - exact) / eps[:, None]
    assert ok.max() < 0.05
    assert ftz[np.arange(16), row].min() > 1.2, ftz[np.arange(16), row].min()


@pytest.mark.parametrize("d", [768, 1024])
def test_dense_outlier_case_puts_rows_in_the_subnormal_range(d):
    rng = np.random.default_rng(5 * d)
    X, Q, row = RA.dense_outlier(rng, d, 12)
    Xs, _ = _scaled_dirs(X, Q)
    assert np.mean(np.abs(Xs[1:]) < RA.MIN_NORMAL) > 0.99 and 0.5 <= np.abs(Xs).max() < 1
    exact, eps = RA.exact_dense(X, Q), RA.dense_eps(X, Q)
    assert (np.abs(RA.model_dense_hi(X, Q) - exact) / eps[:, None]).max() < 0.05
    assert (np.abs(RA.model_dense_hi(X, Q, ftz=True) - exact) / eps[:, None])[np.arange(12), row].min() > 1.0


def _fp32_dots(X, Q):
    """fp32 scores in three summation orders (sequential, pairwise, blocked by 128): what the exact kernels may do."""
    X32, Q32 = np.asarray(X, np.float32), np.asarray(Q, np.float32)
    seq = np.zeros((Q.shape[0], X.shape[0]), np.float32)
    for c in range(X.shape[1]):
        seq = seq + np.outer(Q32[:, c], X32[:, c]).astype(np.float32)
    blk = sum(((Q32[:, c:c + 128] @ X32[:, c:c + 128].T).astype(np.float32) for c in range(0, X.shape[1], 128)),
              np.zeros_like(seq))
    return seq, (Q32 @ X32.T).astype(np.float32), blk


def check_inversion(approx, exact, eps, top, comp, k, fp32=()):
    """Per query: the exact top-k is `top` (in order), the competitors sit below it, the fp16 pass ranks every
    competitor above every target, and the candidate rule under the bound keeps the targets.  Returns the candidate
    counts and how many queries a bound of HALF the size would have lost a target for."""
    counts, lost_half = [], 0
    for b in range(exact.shape[0]):
        order = np.argsort(-exact[b], kind="stable")
        assert np.array_equal(order[:k], top[b])
        assert exact[b, top[b][-1]] > exact[b, comp[b]].max()
        assert approx[b, comp[b]].min() > approx[b, top[b]].max()  # inverted in fp16
        for s in fp32:
            assert np.array_equal(np.argsort(-s[b].astype(np.float64), kind="stable")[:k], top[b])
        c = RA.candidates(approx[b], eps[b], k)
        assert set(top[b].tolist()) <= set(c.tolist())
        counts.append(len(c))
        lost_half += not set(top[b].tolist()) <= set(RA.candidates(approx[b], eps[b] / 2, k).tolist())
    return np.array(counts), lost_half


@pytest.mark.parametrize("d,k", [(256, 1), (256, 10), (256, 12), (768, 1), (768, 10), (768, 12)])
def test_dense_inversion_for_the_two_pass_step(d, k):
    rng = np.random.default_rng(100 * d + k)
    case = RA.dense_inversion(rng, d, k, groups=6, reps=2)
    X, Q = case["X"], case["Q"]
    Xs, Qs = _scaled_dirs(X, Q)
    assert np.all(np.abs(RA.rounding_shift(Xs[Xs != 0])) >= 0.45) and np.all(np.abs(RA.rounding_shift(Qs)) >= 0.45)
    counts, lost = check_inversion(RA.model_dense_hi(X, Q), RA.exact_dense(X, Q), RA.dense_eps(X, Q), case["top"],
                                   case["comp"], k, _fp32_dots(X, Q))
    assert counts.max() <= 32  # dense_hi_select_fuse_kernel's candidate slots per query
    assert lost == len(Q)  # a halved bound drops a target of EVERY query: the GPU test sees it in the ids


@pytest.mark.parametrize("d,k", [(256, 10), (768, 10), (768, 1)])
def test_dense_inversion_for_the_large_scan(d, k):
    rng = np.random.default_rng(7 * d + k)
    tiles = 281
    case = RA.dense_inversion(rng, d, k, groups=4, reps=2, n_total=9017, tiles=tiles)
    X, Q = case["X"], case["Q"]
    approx, exact, eps = RA.model_dense_hi(X, Q), RA.exact_dense(X, Q), RA.dense_eps(X, Q)
    counts, lost = check_inversion(approx, exact, eps, case["top"], case["comp"], k)
    assert lost == len(Q)
    for b in range(len(Q)):  # a query's special rows in distinct tiles; tiles above the cut below the list capacity
        t = np.concatenate([case["top"][b], case["comp"][b]]) // 32
        assert len(set(t.tolist())) == len(t)
        tm = np.maximum.reduceat(approx[b], np.arange(0, X.shape[0], 32))
        tk = np.sort(tm)[::-1][k - 1]
        assert np.sum(tm >= tk - 2 * eps[b]) <= k + max(k, 22)


def test_maxsim_coherent_case_comes_close_to_the_bound():
    rng = np.random.default_rng(31)
    c = RA.maxsim_coherent(rng, 6, 16)
    err = np.abs(RA.model_maxsim_hi(c["Q"], c["D"], c["doc_ptr"]) - RA.exact_maxsim(c["Q"], c["D"], c["doc_ptr"]))
    ratio = err / RA.maxsim_eps(c["Q"], c["D"])[:, None]
    assert ratio.max() <= 1 / 1.5
    assert ratio[np.arange(6), c["doc_of"]].min() >= 0.6, ratio[np.arange(6), c["doc_of"]]


@pytest.mark.parametrize("k,nc", [(1, 4), (10, 12)])
def test_maxsim_inversion(k, nc):
    rng = np.random.default_rng(40 + k)
    c = RA.maxsim_inversion(rng, 16, k, groups=3, reps=2, nc=nc)
    Q, D, ptr = c["Q"], c["D"], c["doc_ptr"]
    approx, exact, eps = RA.model_maxsim_hi(Q, D, ptr), RA.exact_maxsim(Q, D, ptr), RA.maxsim_eps(Q, D)
    counts, _ = check_inversion(approx, exact, eps, c["top"], c["comp"], k)
    assert counts.max() <= RA.ms_cand_cap(k) and 4 * k <= len(ptr) - 1
    # the bound's reach: error differences of two documents reach ~0.89 eps, so 0.4 eps would lose a target
    lost = sum(not set(c["top"][b].tolist()) <= set(RA.candidates(approx[b], 0.4 * eps[b], k).tolist())
               for b in range(len(Q)))
    assert lost == len(Q)
    err = np.abs(approx - exact) / eps[:, None]
    assert 0.4 <= err.max() <= 1 / 1.5


def test_maxsim_subnormal_queries_need_honoured_subnormals():
    rng = np.random.default_rng(9)
    k = 4
    c = RA.maxsim_subnormal(rng, 8, 24, k, 60)
    Q, D, ptr = c["Q"], c["D"], c["doc_ptr"]
    _, q_scale = RA.maxsim_scales(Q, D)
    Qs = Q * q_scale[:, None, None]
    assert np.mean((np.abs(Qs) < RA.MIN_NORMAL)[:, 1:]) > 0.99
    exact, eps = RA.exact_maxsim(Q, D, ptr), RA.maxsim_eps(Q, D)
    ok = RA.model_maxsim_hi(Q, D, ptr)
    ftz = RA.model_maxsim_hi(Q, D, ptr, ftz=True)
    assert (np.abs(ok - exact) / eps[:, None]).max() < 0.05
    lost = 0
    for b in range(len(Q)):
        srt = np.sort(exact[b])[::-1]
        assert srt[k - 1] - srt[k] > 1e-4 * srt[0]  # no near-tie at the cut: the fp32 re-scoring orders it like fp64
        top = np.argsort(-exact[b], kind="stable")[:k]
        assert set(top.tolist()) <= set(RA.candidates(ok[b], eps[b], k).tolist())
        lost += not set(top.tolist()) <= set(RA.candidates(ftz[b], eps[b], k).tolist())
    assert lost >= len(Q) // 2


# ---------------------------------------------------------------------------------------------------------------------
# the scale range of the MaxSim bound

@pytest.fixture(scope="module", params=[(1, 4), (10, 12)], ids=["k1", "k10"])
def ms_inversion_case(request):
    k, nc = request.param
    return k, RA.maxsim_inversion(np.random.default_rng(910), 16, k, groups=8, reps=2, nc=nc)


@pytest.mark.parametrize("sd,sq", RA.MAXSIM_SCALE_PAIRS)
def test_maxsim_scale_range(ms_inversion_case, sd, sq):
    """The inversion store times exact powers of two: the oracle's top-k and the candidate rule under the restated
    bound are those of the unscaled case, the scores stay in fp32's normal range — and what is left of the bound when a
    norm collapses to 0 (its subnormal term) loses a target of EVERY query, at every scale, so a kernel whose norms
    underflow returns other ids.  The bound in the kernels' fp32 arithmetic on the scaled operands follows the fp64
    restatement at every pair; on the raw components it is 0-normed, infinite or NaN outside ~2^-75 .. 2^63."""
    k, base = ms_inversion_case
    c = RA.maxsim_scaled(base, sd, sq)
    Q, D, ptr, top = c["Q"], c["D"], c["doc_ptr"], c["top"]
    exact = RA.exact_maxsim(Q, D, ptr)
    assert np.all(np.abs(exact) >= 2.0 ** -126) and np.all(np.abs(exact) < 2.0 ** 127)
    assert np.array_equal(RA.topk_exact(exact, k)[1], top)  # 1
    approx, eps, sub = RA.model_maxsim_hi(Q, D, ptr), RA.maxsim_eps(Q, D), RA.maxsim_eps_subnormal_term(Q, D)
    # the scaling is exact: scores, model and bound are the unscaled ones times 2^(sd + sq)
    f = 2.0 ** (sd + sq)
    assert np.array_equal(exact, RA.exact_maxsim(base["Q"], base["D"], ptr) * f)
    assert np.array_equal(approx, RA.model_maxsim_hi(base["Q"], base["D"], ptr) * f)
    assert np.allclose(eps, RA.maxsim_eps(base["Q"], base["D"]) * f, rtol=1e-12, atol=0)
    for b in range(len(Q)):
        assert set(top[b].tolist()) <= set(RA.candidates(approx[b], eps[b], k).tolist())  # 2
        assert not set(top[b].tolist()) <= set(RA.candidates(approx[b], sub[b], k).tolist())  # 3
    # fp32, scaled operands: the 1.0001 of the bound covers the rounding of the norms (never below the fp64 bound without it)
    e32 = RA.maxsim_eps_f32(Q, D)
    assert np.all(np.isfinite(e32)) and np.all(e32 >= eps / 1.0001) and np.allclose(e32, eps, rtol=1e-5, atol=0)
    raw = RA.maxsim_eps_f32(Q, D, scaled=False)
    if min(sd, sq) <= -75:
        assert np.allclose(raw, sub, rtol=1e-6, atol=0)  # a norm is exactly 0
    elif max(sd, sq) >= 70:
        assert np.all(np.isinf(raw))
    else:
        assert np.allclose(raw, eps, rtol=1e-5, atol=0)


def test_maxsim_zero_query_on_a_huge_store_has_a_bound():
    """0 x inf: an all-zero query on the store x 2^70 — raw norms give eps = NaN (no document passes a NaN threshold),
    scaled norms the subnormal term."""
    c = RA.maxsim_scaled(RA.maxsim_inversion(np.random.default_rng(911), 16, 1, groups=2, reps=1, nc=4), 70, 0)
    Q = c["Q"].copy()
    Q[1] = 0.0
    assert np.isnan(RA.maxsim_eps_f32(Q, c["D"], scaled=False)[1])
    e = RA.maxsim_eps_f32(Q, c["D"])[1]
    assert np.isfinite(e) and np.isclose(e, RA.maxsim_eps_subnormal_term(Q, c["D"])[1], rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# shape edges of the MaxSim two-pass top-k: the data is what tests/test_maxsim_two_pass_edges_gpu.py says it is

TOL = 1e-4


def _skipped(exact, k):
    es, _ = RA.topk_exact(exact, k)
    return float(np.mean([~RA.oracle_rank_mask(row, TOL) for row in es]))


@pytest.mark.parametrize("nq,q_len", [(9, 32), (16, 17)])
def test_maxsim_long_docs_reach_the_top(nq, q_len):
    c = RA.maxsim_long_docs(np.random.default_rng(1000 + nq), nq, q_len)
    ptr, lens = c["doc_ptr"], np.diff(c["doc_ptr"])
    assert len(lens) == 80 and lens[-1] == 513 and set((1, 448, 449, 480, 481, 511, 512, 513, 640, 1000)) <= set(lens.tolist())
    assert sorted(lens[c["long"]].tolist()) == sorted(RA.MS_LONG_LENS) and {0, 79} <= set(c["long"].tolist())
    exact = RA.exact_maxsim(c["Q"], c["D"], ptr)
    _, ids = RA.topk_exact(exact, 5)
    assert len(set(ids.ravel().tolist()) & set(c["long"].tolist())) >= 5
    assert ids[0, 0] == 79  # query 0's planted tokens: the last token of the store among them
    assert _skipped(exact, 5) <= 0.10
    # the long documents are candidates of the first pass too (not only of the oracle)
    approx, eps = RA.model_maxsim_hi(c["Q"], c["D"], ptr), RA.maxsim_eps(c["Q"], c["D"])
    cand = set().union(*[set(RA.candidates(approx[b], eps[b], 5).tolist()) for b in range(nq)])
    assert len(cand & set(c["long"].tolist())) >= 5


def test_maxsim_short_docs_rank_gaps():
    """Random unit rows at the selector and depth shapes: at most 10 % of the compared rank positions sit in a near-tie."""
    c = RA.maxsim_short_docs(np.random.default_rng(2100), 2100, 24)
    exact = RA.exact_maxsim(c["Q"], c["D"], c["doc_ptr"])
    assert _skipped(exact[:, :640], 10) <= 0.10 and _skipped(exact[8:16, :640], 33) <= 0.10  # the handle-reuse calls
    assert c["doc_ptr"][-1] <= 15000
    for n in (40, 640, 641, 1280, 1281, 2048, 2049, 2100):
        for k in (1, 10):
            assert _skipped(exact[:8, :n], k) <= 0.10, (n, k)
    assert _skipped(exact[:, :40], 11) <= 0.10
    c = RA.maxsim_depth_docs(np.random.default_rng(1100), 9)
    assert len(c["doc_ptr"]) == 1101 and c["doc_ptr"][-1] <= 15000
    exact = RA.exact_maxsim(c["Q"], c["D"], c["doc_ptr"])
    for k in (32, 33, 64, 65, 128, 256):
        print(k, _skipped(exact, k))
        assert _skipped(exact, k) <= 0.10, k


def test_maxsim_mixed_overflow_case():
    k = 10
    c = RA.maxsim_mixed_overflow(np.random.default_rng(77))
    Q, D, ptr = c["Q"], c["D"], c["doc_ptr"]
    approx, eps = RA.model_maxsim_hi(Q, D, ptr), RA.maxsim_eps(Q, D)
    cap = RA.ms_cand_cap(k)
    for b in range(16):
        n = len(RA.candidates(approx[b], eps[b], k))
        if b in c["aimed"]:
            assert n > 2 * cap, (b, n)
        else:
            assert n < cap / 2, (b, n)
    assert sorted(c["aimed"].tolist()) == list(range(0, 16, 2))  # one of each kind in every pass-1 wave (queries 2 w, 2 w + 1)


@pytest.mark.parametrize("copies", [1, 8, 9, 16, 17, 24])
def test_maxsim_shared_document_is_a_candidate_of_exactly_the_copies(copies):
    k = 10
    c = RA.maxsim_shared(np.random.default_rng(24))
    Q = RA.maxsim_shared_batch(c["pool"], copies)
    assert Q.shape == (24, 32, 128)
    approx, eps = RA.model_maxsim_hi(Q, c["D"], c["doc_ptr"]), RA.maxsim_eps(Q, c["D"])
    st = np.array([RA.candidate_status(approx[b], eps[b], k, 1e-2)[RA.MS_SHARED_DOC] for b in range(24)])
    assert np.all(st[:copies] == 1) and np.all(st[copies:] == -1), st  # by a margin 1 000 x the fp32 summation noise
    exact = RA.exact_maxsim(Q, c["D"], c["doc_ptr"])
    assert np.all(np.argmax(exact[:copies], axis=1) == RA.MS_SHARED_DOC)
    assert np.diff(c["doc_ptr"])[RA.MS_SHARED_DOC] == 70 and 4 * k <= len(c["doc_ptr"]) - 1
    if copies == 1:
        assert _skipped(exact, k) <= 0.10

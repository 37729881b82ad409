"""The MMR oracle and its cases (tests/mmr_adversary.py) checked on the CPU: the certificates of the real-valued cases, the
oracle against a differently written restatement, and every wrong-kernel model against the committed cases: a model the
cases cannot tell from the definition would mean the GPU tests prove nothing about that mistake."""
import math

import numpy as np
import pytest

import mmr_adversary as M


def test_cos_bound_is_the_dense_bar():
    assert M.cos_bound(768) == pytest.approx(1.0e-4, rel=0.02)


def test_integer_gram_is_exact_in_fp32():
    """Entries in {-2 .. 2}: the fp32 Gram in two summation orders equals the fp64 one (largest entry far below 2^24)."""
    for d in (768, 1024):
        X = M.int_matrix(200, d)
        assert set(np.unique(X)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        G64 = X.astype(np.float64) @ X.astype(np.float64).T
        assert np.abs(G64).max() <= 4 * d < 2 ** 24
        assert (X @ X.T == G64).all() and (M.gram32_other_order(X, range(64)) == G64[:64, :64]).all()


@pytest.mark.parametrize("d", M.REAL_DIMS)
@pytest.mark.parametrize("lam", M.REAL_LAMS)
def test_real_cases_are_certified(d, lam):
    """Every committed seed: the lead exceeds 2 (1 - lam) E, the selection reorders the list, an fp32 Gram in another
    summation order selects the same positions, and its values are inside the bounds the GPU test asserts."""
    seeds = M.REAL_SEEDS[(d, lam)]
    assert len(seeds) >= 3 and all(0 <= s < M.REAL_TRIED for s in seeds)
    for s in seeds:
        case, lead = M.real_case(s, d, lam)
        assert M.certified(s, d, lam) and lead > 2.0 * (1.0 - lam) * M.cos_bound(d), (s, lead)
        assert np.abs(np.linalg.norm(case.X.astype(np.float64), axis=1) - 1.0).max() < 1e-6
        pos = case.exp[0][0]
        assert case.exp[3][0] == M.REAL_K and (pos != np.arange(M.REAL_K)).any(), (s, "the plain ranking")
        p, v, sim, _ = M.mmr_one(case.X, case.rows[0], case.rel[0], M.REAL_POOL, M.REAL_POOL, M.REAL_K, lam,
                                 gram=M.gram32_other_order)
        other = (np.array([p], dtype=np.int32), np.array([v]), np.array([sim]), case.exp[3])
        M.assert_close(other, case.exp, lam, d, (s, d, lam))


def brute(X, rows, rel, count, pool, k_sel, lam):
    """The definition once more, written from the whole cosine matrix and a sort per step."""
    m = min(max(int(count), 0), pool)
    n = len(X)
    R = np.stack([X[r].astype(np.float64) if 0 <= r < n else np.zeros(X.shape[1]) for r in rows[:m]]) if m else None
    picked, out = [], []
    for _ in range(min(k_sel, m)):
        G = (R @ R.T).astype(np.float32).astype(np.float64)
        with np.errstate(all="ignore"):
            den = np.sqrt(np.outer(np.diag(G), np.diag(G)))
            cos = np.where(np.isfinite(den) & (den > 0) & np.isfinite(G), G / den, 0.0)
        cand = []
        for i in range(m):
            if i in picked:
                continue
            ms = max(cos[i, j] for j in picked) if picked else 0.0
            v = float(lam) * float(rel[i]) - (1.0 - float(lam)) * float(ms)
            cand.append((math.isnan(v), -v if not math.isnan(v) else 0.0, i, v, ms))
        cand.sort(key=lambda c: c[:3])
        picked.append(cand[0][2])
        out.append((cand[0][2], cand[0][3], cand[0][4]))
    return out


def test_oracle_matches_brute_force_at_small_pools():
    n_checked = 0
    for pool in (1, 2, 3, 4, 5, 6):
        for t, kind in enumerate(M.REL_KINDS):
            case = M.int_case(7, 8, 12, pool, pool, M.LAMS[(t + pool) % 4], seed=pool * 10 + t, order=M.ORDERS[t % 3],
                              rel_kind=kind, ld_extra=2)
            pos, val, sim, cnt = case.exp
            for q in range(case.nq):
                exp = brute(case.X, case.rows[q], case.rel[q], case.count[q], pool, pool, case.lam)
                assert cnt[q] == len(exp) and (pos[q, len(exp):] == -1).all()
                assert (val[q, len(exp):] == 0.0).all() and (sim[q, len(exp):] == 0.0).all()
                for j, (p, v, s) in enumerate(exp):
                    assert pos[q, j] == p, (case.name, q, j)
                    assert M.same_bits(val[q, j], v) and M.same_bits(sim[q, j], s), (case.name, q, j)
                    n_checked += 1
    assert n_checked > 500


def test_pinned_consequences():
    """lambda = 1 on a descending rel returns 0, 1, 2, ...; the same row twice has cosine exactly 1 between the copies."""
    case = M.int_case(50, 124, 5, 33, 33, 1.0, rel_kind="desc", count_kind="full", seed=7)
    assert (case.exp[0] == np.arange(33)).all()
    X = M.int_matrix(7, 8)
    pos, val, sim, _ = M.mmr_oracle(X, np.array([[4, 4, 5]]), np.array([[3.0, 2.0, 1.0]]), [3], 3, 3, 0.5)
    assert pos[0].tolist()[0] == 0 and sim[0][list(pos[0]).index(1)] == 1.0


@pytest.mark.parametrize("model", M.MODELS)
def test_wrong_kernel_models_are_caught(model):
    hit = [c.name for c in M.model_cases() if M.differs(c.model(model), c.exp)]
    assert hit, f"no committed case tells the model '{model}' from the definition"


def test_fma_contraction_changes_a_selection_or_only_bits():
    """The case built for the contraction: lambda and rel with full mantissas, so lambda * rel is inexact and the single
    rounding of a fused multiply-add shows in the bits of out_mmr from the second step on (exact rational arithmetic)."""
    case = M.int_case(50, 132, 6, 33, 32, M.LAM_ODD, seed=101, rel_kind="random", ld_extra=4)
    for model in ("fma_rel", "fma_sim"):
        got = case.model(model)
        assert (~M.same_bits(got[1], case.exp[1])).sum() >= 10, model
        assert M.same_bits(got[1][:, 0], case.exp[1][:, 0]).all(), "the first step has maxsim = 0: nothing to contract"

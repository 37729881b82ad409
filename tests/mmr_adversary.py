"""The MMR selection of include/amdretrieval.h (csrc/mmr.hip) restated in fp64 Python, and the batches it is tested on.
numpy only.

mmr_oracle is the definition: an fp32 Gram matrix of the candidate rows (here: the fp64 product rounded to fp32, the
correctly rounded inner product), the fp64 cosine, the greedy loop with ties to the lower position and NaN last.

Integer cases: matrix entries in {-2 .. 2}, so every fp32 Gram entry is an integer below 2^24 (at most 4 * 1024) and exact
in ANY summation order: the oracle is the kernel's answer bit for bit.  `rel` is arbitrary doubles, value edges included.

Real-valued cases: unit rows around 12 centres, so near-duplicates exist.  A kernel's fp32 Gram differs from the oracle's
by rounding, so its cosines differ by at most E = cos_bound(d) and every mmr value by (1 - lam) * E: a step whose winner
leads the runner-up by more than 2 * (1 - lam) * E has the same winner under any summation order.  real_case returns the
smallest such lead over all steps; REAL_SEEDS lists, per (d, lam), only seeds whose lead exceeds the bar (the certificate,
re-checked by tests/test_mmr_adversary.py), so no case is ever set aside on the GPU.

A NaN result is compared as "NaN on both sides": the payload and sign of a NaN born from inf * 0 or handed through from
`rel` differ between processors and are not part of the contract.  Every other value is compared by its bits."""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

MAX_POOL = 64  # AMDR_MMR_MAX_POOL
MODELS = ("dot", "sum", "no_exclude", "tie_high", "neg_inf", "nan_first", "missing_row0", "ignore_pool", "fma_rel",
          "fma_sim")


def cos_bound(d: int) -> float:
    """First-order bound on the cosine error of an fp32 Gram of unit rows, any summation order, 10 % slack: each of the
    three Gram entries of a cosine carries at most d * 2^-24 relative to the row norms (gamma_d with u = 2^-24), the two
    diagonal ones enter through a square root at half weight: (1 + 1/2 + 1/2) * d * 2^-24 = 2 d 2^-24, times 1.1."""
    return 2.2 * d * 2.0 ** -24


def _fma(a: float, b: float, c: float) -> float:
    """round(a * b + c) with ONE rounding, for finite operands (float(Fraction) rounds to nearest even)."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    r = Fraction(a) * Fraction(b) + Fraction(c)
    return float(r) if r != 0 else a * b + c


def _gram(X: np.ndarray, rows, model=None) -> np.ndarray:
    n, d = X.shape
    R = np.zeros((len(rows), d), dtype=np.float64)
    has = np.zeros(len(rows), dtype=bool)
    for i, r in enumerate(rows):
        if 0 <= r < n:
            R[i], has[i] = X[r], True
        elif model == "missing_row0":
            R[i], has[i] = X[0], True
    with np.errstate(all="ignore"):
        G = (R @ R.T).astype(np.float32)
    G[~has, :] = 0.0
    G[:, ~has] = 0.0
    return G


def _cos(G: np.ndarray, i: int, j: int, model=None) -> float:
    gij = float(G[i, j])
    if model == "dot":
        return gij if math.isfinite(gij) else 0.0
    prod = float(G[i, i]) * float(G[j, j])
    den = math.sqrt(prod) if prod >= 0.0 else math.nan
    if not (math.isfinite(den) and den > 0.0 and math.isfinite(gij)):
        return 0.0
    return gij / den


def mmr_one(X, rows, rel, count, pool, k_sel, lam, model=None, gram=None):
    """One query -> (pos, mmr, maxsim, lead): lists of min(k_sel, m) entries and the smallest lead of a winner over the
    runner-up (inf when a step had no runner-up, NaN-valued candidates not counted).  gram(X, rows): another Gram matrix
    than the correctly rounded one."""
    m = max(int(count), 0) if model == "ignore_pool" else min(max(int(count), 0), int(pool))
    rows = [int(r) for r in rows[:m]]
    rel = [float(x) for x in rel[:m]]
    G = gram(X, rows) if gram is not None else _gram(X, rows, model)
    lam = float(lam)
    om = 1.0 - lam
    maxsim = [-math.inf if model == "neg_inf" else 0.0] * m
    taken = [False] * m
    pos, val, sim, lead = [], [], [], math.inf
    for step in range(min(int(k_sel), m)):
        best, bv, second = -1, 0.0, -math.inf
        for i in range(m):
            if taken[i] and model != "no_exclude":
                continue
            if model == "fma_rel":
                v = _fma(lam, rel[i], -(om * maxsim[i]))
            elif model == "fma_sim":
                v = _fma(-om, maxsim[i], lam * rel[i])
            else:
                v = lam * rel[i] - om * maxsim[i]
            if best < 0:
                wins = True
            elif model == "nan_first" and (math.isnan(v) or math.isnan(bv)):
                wins = math.isnan(v) and not math.isnan(bv)
            elif math.isnan(v):
                wins = False
            elif math.isnan(bv):
                wins = True
            else:
                wins = v >= bv if model == "tie_high" else v > bv
            if wins:
                if best >= 0 and not math.isnan(bv):
                    second = max(second, bv)
                best, bv = i, v
            elif not math.isnan(v):
                second = max(second, v)
        if not math.isnan(bv) and second > -math.inf:
            lead = min(lead, bv - second) if math.isfinite(bv - second) else lead
        pos.append(best)
        val.append(bv)
        sim.append(maxsim[best])
        taken[best] = True
        for i in range(m):
            c = _cos(G, i, best, model)
            if model == "sum":
                maxsim[i] = maxsim[i] + c
            elif step == 0 and model != "neg_inf":
                maxsim[i] = c
            else:
                maxsim[i] = c if c > maxsim[i] else maxsim[i]
    return pos, val, sim, lead


def mmr_oracle(X, rows, rel, count, pool, k_sel, lam, model=None):
    """-> (out_pos i32 [nq, k_sel], out_mmr f64, out_maxsim f64, out_count i32 [nq]) as the kernel writes them.
    model: None = the definition; a name of MODELS = one deliberately wrong kernel."""
    nq = len(count)
    pos = np.full((nq, k_sel), -1, dtype=np.int32)
    val = np.zeros((nq, k_sel), dtype=np.float64)
    sim = np.zeros((nq, k_sel), dtype=np.float64)
    cnt = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        p, v, s, _ = mmr_one(X, rows[q], rel[q], count[q], pool, k_sel, lam, model)
        p, v, s = p[:k_sel], v[:k_sel], s[:k_sel]
        cnt[q] = len(p)
        pos[q, :len(p)], val[q, :len(p)], sim[q, :len(p)] = p, v, s
    return pos, val, sim, cnt


def same_bits(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def differs(got, exp) -> bool:
    return not ((got[0] == exp[0]).all() and (got[3] == exp[3]).all() and same_bits(got[1], exp[1]).all()
                and same_bits(got[2], exp[2]).all())


def assert_exact(got, exp, what):
    """Positions, counts and the bits of mmr and maxsim, whole rows including the fill."""
    assert (got[3] == exp[3]).all(), (what, "out_count", got[3][got[3] != exp[3]][:4], exp[3][got[3] != exp[3]][:4])
    bad = np.argwhere(got[0] != exp[0])
    assert bad.size == 0, (what, "out_pos", bad[0], got[0][bad[0][0]], exp[0][bad[0][0]])
    for name, g, e in (("out_mmr", got[1], exp[1]), ("out_maxsim", got[2], exp[2])):
        bad = np.argwhere(~same_bits(g, e))
        assert bad.size == 0, (what, name, bad[0], g[tuple(bad[0])].hex(), e[tuple(bad[0])].hex())


def assert_close(got, exp, lam, d, what):
    """A certified real-valued case: equal positions and counts, maxsim within E, mmr within (1 - lam) * E."""
    E = cos_bound(d)
    assert (got[3] == exp[3]).all(), (what, "out_count")
    bad = np.argwhere(got[0] != exp[0])
    assert bad.size == 0, (what, "out_pos", bad[0], got[0][bad[0][0]], exp[0][bad[0][0]])
    e_sim, e_mmr = np.abs(got[2] - exp[2]).max(initial=0.0), np.abs(got[1] - exp[1]).max(initial=0.0)
    assert e_sim <= E, (what, "out_maxsim", e_sim, E)
    assert e_mmr <= (1.0 - lam) * E, (what, "out_mmr", e_mmr, (1.0 - lam) * E)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


class Case:
    """X [n, d] f32; rows i64 [nq, ld]; rel f64 [nq, ld]; count i32 [nq]; pool, k_sel, lam; exp = the oracle's record."""

    def __init__(self, X, rows, rel, count, pool, k_sel, lam, name=""):
        self.X, self.rows, self.rel, self.count = frozen(np.ascontiguousarray(X, dtype=np.float32),
                                                         np.ascontiguousarray(rows, dtype=np.int64),
                                                         np.ascontiguousarray(rel, dtype=np.float64),
                                                         np.ascontiguousarray(count, dtype=np.int32))
        self.pool, self.k_sel, self.lam, self.name = int(pool), int(k_sel), float(lam), name
        self.nq = len(self.count)

    @functools.cached_property
    def exp(self):
        return frozen(*self.model(None))

    def model(self, model):
        return mmr_oracle(self.X, self.rows, self.rel, self.count, self.pool, self.k_sel, self.lam, model)


# ---- integer cases -------------------------------------------------------------------------------------------------------
LAM_ODD = 0.7351028367  # not representable in a few bits
REL_EDGES = (0.0, -0.0, math.inf, -math.inf, math.nan, 1.0, 1.0, 0.5, 0.5, -3.25, 2.0 ** -1070, 1e300)


@functools.lru_cache(maxsize=None)
def int_matrix(n: int, d: int, seed: int = 0) -> np.ndarray:
    """Entries in {-2 .. 2}; row 3 (when there is one) all zero; rows 1 and 2 equal up to scale (cosine exactly 1)."""
    rng = np.random.default_rng([seed, n, d, 0x11])
    X = rng.integers(-2, 3, size=(n, d)).astype(np.float32)
    if n > 3:
        X[3] = 0.0
        X[2] = 2.0 * np.sign(X[1])
        X[1] = np.sign(X[1])
    return frozen(X)


def int_case(n, d, nq, pool, k_sel, lam, *, seed=0, order="random", rel_kind="random", ld_extra=0, count_kind="ragged",
             name=""):
    """rows: 'random' (with replacement: repeats occur), 'descending', 'repeated' (one row many times), each with a -1, an
    n, the zero row and a row used twice planted in the first positions of some queries.
    rel: 'random' arbitrary doubles, 'desc' descending, 'ties' few distinct values, 'edges' +-0 / +-inf / NaN / ties mixed in.
    count: 'ragged' in [0, pool + 3] (0 and values above the pool included), 'full' = pool, 'short' < k_sel for some."""
    rng = np.random.default_rng([seed, n, d, nq, pool, k_sel, 0x22])
    ld = pool + ld_extra
    X = int_matrix(n, d)
    if order == "descending":
        rows = np.tile(np.arange(n - 1, n - 1 - ld, -1, dtype=np.int64) % n, (nq, 1)) - rng.integers(0, n, size=(nq, 1))
        rows %= n
    elif order == "repeated":
        rows = np.tile(rng.integers(0, n, size=(nq, 1)), (1, ld))
        rows[:, ::3] = rng.integers(0, n, size=rows[:, ::3].shape)
    else:
        rows = rng.integers(0, n, size=(nq, ld))
    rows = rows.astype(np.int64)
    for q in range(nq):
        plant = [(-1, n, min(3, n - 1), 1, 1, 2 % n), (n, -1), (min(3, n - 1),), (), (5 % n, 5 % n), (-7, n + 9, 2 ** 40)][q % 6]
        at = rng.permutation(ld)[:len(plant)]
        rows[q, at[:len(plant)]] = plant[:len(at)]
    if rel_kind == "desc":
        rel = -np.sort(-rng.uniform(0.05, 1.0, size=(nq, ld)), axis=1)
    elif rel_kind == "ties":
        rel = rng.integers(0, 3, size=(nq, ld)).astype(np.float64) * 0.25
    elif rel_kind == "edges":
        rel = rng.standard_normal((nq, ld))
        pick = rng.integers(0, len(REL_EDGES), size=(nq, ld))
        use = rng.random((nq, ld)) < 0.5
        rel[use] = np.array(REL_EDGES)[pick[use]]
    else:
        rel = rng.standard_normal((nq, ld)) * 10.0 ** rng.integers(-3, 4, size=(nq, ld))
    if count_kind == "full":
        count = np.full(nq, pool)
    elif count_kind == "short":
        count = rng.integers(0, max(k_sel, 1) + 1, size=nq)
    else:
        count = rng.integers(0, pool + 4, size=nq)
        count[::5] = pool
        if nq > 1:
            count[1] = 0
        if nq > 2:
            count[2] = pool + 3
    return Case(X, rows, rel, count, pool, k_sel, lam, name or f"int n={n} d={d} nq={nq} pool={pool} k={k_sel} lam={lam} "
                f"{order}/{rel_kind}/{count_kind}")


def tiled(case: Case, nq: int):
    """A batch of nq queries that repeats the queries of `case` with its (odd) period, and its record: the oracle runs on
    the distinct queries only.  -> (rows, rel, count, exp)"""
    idx = np.arange(nq) % case.nq
    return case.rows[idx], case.rel[idx], case.count[idx], tuple(a[idx] for a in case.exp)


# ---- real-valued cases ---------------------------------------------------------------------------------------------------
REAL_POOL, REAL_K, REAL_N, REAL_CENTRES, REAL_NOISE = 30, 10, 240, 12, 0.35
REAL_DIMS, REAL_LAMS = (128, 768, 1024), (0.3, 0.5, 0.7)


@functools.lru_cache(maxsize=None)
def real_matrix(d: int, seed: int) -> np.ndarray:
    """Unit rows: one of 12 unit centres plus Gaussian noise of expected norm 0.35, normalised."""
    rng = np.random.default_rng([seed, d, 0x33])
    C = rng.standard_normal((REAL_CENTRES, d))
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    X = C[rng.integers(0, REAL_CENTRES, size=REAL_N)] + REAL_NOISE / math.sqrt(d) * rng.standard_normal((REAL_N, d))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return frozen(X.astype(np.float32))


@functools.lru_cache(maxsize=None)
def real_case(seed: int, d: int, lam: float):
    """-> (Case of one query, the smallest lead of a winner over its runner-up).  Relevances descend, as fused scores do."""
    rng = np.random.default_rng([seed, d, int(lam * 1000), 0x44])
    X = real_matrix(d, seed)
    rows = rng.permutation(REAL_N)[:REAL_POOL][None, :]
    rel = -np.sort(-rng.uniform(0.2, 0.9, size=(1, REAL_POOL)), axis=1)
    case = Case(X, rows, rel, [REAL_POOL], REAL_POOL, REAL_K, lam, f"real seed={seed} d={d} lam={lam}")
    lead = mmr_one(case.X, case.rows[0], case.rel[0], REAL_POOL, REAL_POOL, REAL_K, lam)[3]
    return case, lead


def certified(seed: int, d: int, lam: float) -> bool:
    return real_case(seed, d, lam)[1] > 2.0 * (1.0 - lam) * cos_bound(d)


# per (d, lam): seeds of range(REAL_TRIED) that certify — generated with certified(), re-checked by test_mmr_adversary.py
REAL_TRIED = 12
REAL_SEEDS = {
    (128, 0.3): (0, 1, 2, 3), (128, 0.5): (0, 1, 2, 3), (128, 0.7): (0, 1, 2, 3),
    (768, 0.3): (0, 1, 5, 6), (768, 0.5): (0, 1, 2, 3), (768, 0.7): (0, 1, 2, 3),
    (1024, 0.3): (0, 1, 2, 4), (1024, 0.5): (0, 1, 2, 3), (1024, 0.7): (0, 1, 2, 3),
}


def real_cases(d: int, lam: float) -> list:
    """The committed (certified) cases of one cell, one query each: every seed has a matrix of its own."""
    return [real_case(s, d, lam)[0] for s in REAL_SEEDS[(d, lam)]]


def gram32_other_order(X, rows):
    """An fp32 Gram in another summation order than BLAS or the kernel: a plain fp32 running sum, column by column."""
    R = X[np.asarray(rows)].astype(np.float32)
    G = np.zeros((len(rows), len(rows)), dtype=np.float32)
    for k in range(R.shape[1] - 1, -1, -1):
        G += np.outer(R[:, k], R[:, k]).astype(np.float32)
    return G


# ---- the committed integer cases -------------------------------------------------------------------------------------------
POOLS = (1, 2, 3, 31, 32, 33, 63, 64)   # the tile (16, 32, 48) and wave edges
DIMS = (4, 124, 128, 132, 768, 1024)    # slice remainders of the 128-column K slice
LAMS = (0.0, 1.0, 0.5, LAM_ODD)
ORDERS = ("random", "descending", "repeated")
REL_KINDS = ("random", "desc", "ties", "edges")


def k_sels(pool: int):
    return sorted({1, pool, max(1, pool // 2)})


@functools.lru_cache(maxsize=None)
def grid_cases(d: int, n: int) -> tuple:
    """Every pool x every k_sel of k_sels(pool), nq = 3 (1 for the first pool); lambda, row order, rel kind and count kind
    cycle so that each occurs with small and large pools."""
    out, t = [], 0
    for pool in POOLS:
        for k in k_sels(pool):
            out.append(int_case(n, d, 1 if pool == 1 else 3, pool, k, LAMS[t % 4], seed=t, order=ORDERS[t % 3],
                                rel_kind=REL_KINDS[(t // 2) % 4], ld_extra=(0, 4)[t % 2],
                                count_kind=("ragged", "full", "short")[(t // 3) % 3]))
            t += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def model_cases() -> tuple:
    """What the wrong-kernel models are run against: small pools, every rel kind, lambda 0.5 and the odd one."""
    out = []
    for t, kind in enumerate(REL_KINDS):
        for pool, d in ((3, 4), (6, 124), (33, 132)):
            out.append(int_case(7 if pool < 33 else 50, d, 6, pool, max(1, pool - 1), (0.5, LAM_ODD)[t % 2], seed=100 + t,
                                order=ORDERS[t % 3], rel_kind=kind, ld_extra=4))
    return tuple(out) + tuple(real_case(REAL_SEEDS[(128, 0.5)][0], 128, 0.5)[:1])

"""Inputs that steer the register top-k selectors of csrc/topk.hpp, and a numpy model of their cut.

Both selectors (wave_select_small: one row per wave, reached through select_row / select_row_any;
wave_select_small_pair32: two rows per wave, 32 lanes each, through select_row_pair / select_row_pair_any) take the k-th
best of the LANE maxima as a cut T, gather every key at or above T into 64 (32) slots, sort those with a 16-, 32- or
64-lane network and give up (-1: the caller ranks the row with the staged selector) when more keys survive than there
are slots.  What they do therefore depends on how the good scores fall over the LANES — random rows leave "a few more
than k" survivors and never reach the wider sorts, the slot limit or the give-up branch.  The rows built here have an
exact, chosen number of survivors.

Every value is an integer with |v| <= 4096 (exact in fp32); pattern j is column j of a matrix X[n, d] and query b the
unit vector of its pattern's column, so the score row IS the column whatever the summation order, and a result is
compared with oracle.dense.topk_desc of the column: ids with ==, scores by bits.

Not a test module (no test_ prefix): tests/test_selector_adversary.py checks the model and the rows on the CPU,
tests/test_selector_adversary_gpu.py runs them on the device.
"""
from __future__ import annotations

import numpy as np

FLT_MAX = np.finfo(np.float32).max
VMAX = 4096  # |value| of every crafted score

SINGLE, PAIR = "single", "pair"
SLOTS = {SINGLE: 64, PAIR: 32}  # survivors a selector holds; one more and it gives up
LANES = {SINGLE: 64, PAIR: 32}

# rows up to which select_row_any / select_row_pair_any compile V keys per lane (topk.hpp)
SINGLE_V = ((256, 4), (640, 10), (1024, 16), (1280, 20), (2048, 32))
PAIR_V = ((256, 8), (512, 16), (640, 20), (1024, 32))


# ---------------------------------------------------------------------------------------------------------------------
# the lane maps, from the code

def lane_slot(n: int, selector: str, lo: int = 0):
    """(lane, slot) of rows lo .. n-1.  select_row: row r of a slab starting at lo sits in lane (r - lo) % 64, key
    register (r - lo) // 64.  select_row_pair: a lane loads four consecutive scores per 512-byte piece of its half's
    row — lane (r % 128) // 4 of the half, key register 4 (r // 128) + r % 4."""
    r = np.arange(lo, n, dtype=np.int64)
    if selector == SINGLE:
        return (r - lo) % 64, (r - lo) // 64
    return (r % 128) // 4, 4 * (r // 128) + r % 4


def keys_per_lane(n: int, selector: str) -> int:
    for rows, v in (SINGLE_V if selector == SINGLE else PAIR_V):
        if n <= rows:
            return v
    raise ValueError(f"{n} rows: beyond the {selector} selector")


def ord32(x) -> np.ndarray:
    """topk.hpp ord32: order-preserving 32-bit key of an fp32 score; -0.0 == +0.0, NaN -> 1 (behind -inf, ahead of the
    padding key 0)."""
    x = np.asarray(x, np.float32) + np.float32(0.0)
    u = x.view(np.uint32).astype(np.uint64)
    key = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(x), 1, key).astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# the model of the cut

def survivors(row, k: int, selector: str) -> int:
    """Keys that reach the selector's sort for score row `row` at depth k.
    single: candidates are composites (ord32(score), ~id); T = the k-th best lane maximum (lane 63's when k > 64) and a
            key survives unless T is better — an equal score with a higher id than T's is out;
    pair:   the lane maxima, their sort and the cut look at the score key only — every equal score survives;
    either: fewer populated lanes than k -> T is padding and every row survives."""
    row = np.asarray(row, np.float32)
    n = len(row)
    lane, _ = lane_slot(n, selector)
    key = ord32(row)
    if selector == SINGLE:
        key = (key << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64))
    best = np.zeros(LANES[selector], np.uint64)
    np.maximum.at(best, lane, key)
    t = np.sort(best)[::-1][min(k, LANES[selector]) - 1]
    t = max(int(t), 1)  # (every real key is > 0: padding as the cut lets all of them through)
    return int(np.count_nonzero(key >= np.uint64(t)))


def gives_up(row, k: int, selector: str) -> bool:
    return survivors(row, k, selector) > SLOTS[selector]


def sort_width(s: int, selector: str) -> int:
    """Lanes of the network that sorts s survivors (s <= SLOTS)."""
    assert s <= SLOTS[selector]
    return 16 if s <= 16 else 32 if s <= 32 or selector == PAIR else 64


def lanes_populated(n: int, selector: str) -> int:
    return len(np.unique(lane_slot(n, selector)[0]))


# ---------------------------------------------------------------------------------------------------------------------
# rows with a chosen number of survivors

def realisable(n: int, k: int, s: int, selector: str) -> bool:
    """craft(n, k, s, selector) exists: k hot lanes, the cut value alone in one of them, the other s - 1 survivors
    in the rows of the other k - 1 (at least one each)."""
    lane, _ = lane_slot(n, selector)
    sizes = np.sort(np.bincount(lane, minlength=LANES[selector]))[::-1]
    if k > np.count_nonzero(sizes):
        return s == n  # T is padding: every row survives
    return k <= s <= n and s - 1 <= int(sizes[:k - 1].sum()) and (k > 1 or s == 1)


def craft(n: int, k: int, s: int, selector: str, rng) -> np.ndarray:
    """A row of n distinct integer-valued fp32 scores, |v| <= VMAX, with exactly s survivors at depth k: the s best
    values sit in k hot lanes — the smallest of them alone in its lane, so that it is the k-th best lane maximum, the
    others spread over the rows of the other k - 1 hot lanes, at least one each — and every other row lies below."""
    if not realisable(n, k, s, selector):
        raise ValueError(f"no row of {n} scores with {s} survivors at k = {k} ({selector})")
    values = np.sort(rng.choice(2 * VMAX + 1, size=n, replace=False) - VMAX).astype(np.float32)  # ascending
    row = np.empty(n, np.float32)
    lane, _ = lane_slot(n, selector)
    rows_of = [np.nonzero(lane == l)[0] for l in range(LANES[selector])]
    populated = [l for l in range(LANES[selector]) if len(rows_of[l])]
    if k > len(populated):
        return values[rng.permutation(n)]
    lone = int(rng.choice(populated))
    others = [l for l in populated if l != lone]
    hot = [others[i] for i in rng.permutation(len(others))[:k - 1]]
    if sum(len(rows_of[l]) for l in hot) < s - 1:  # not enough room in a random choice: the fullest lanes
        hot = sorted(others, key=lambda l: -len(rows_of[l]))[:k - 1]
    top = [int(rng.choice(rows_of[lone]))]  # the cut value's row
    first = [int(rng.choice(rows_of[l])) for l in hot]  # one survivor per hot lane ...
    pool = np.setdiff1d(np.concatenate([rows_of[l] for l in hot]) if hot else np.empty(0, np.int64), first)
    more = rng.choice(pool, size=s - 1 - len(first), replace=False).tolist() if s - 1 > len(first) else []  # ... the rest anywhere in them
    upper = np.array(first + more, dtype=np.int64)
    row[top[0]] = values[n - s]
    row[upper[rng.permutation(len(upper))]] = values[n - s + 1:]
    rest = np.setdiff1d(np.arange(n), np.concatenate([top, upper]).astype(np.int64))
    row[rest[rng.permutation(len(rest))]] = values[:n - s]
    return row


def _rank_rows(row: np.ndarray) -> np.ndarray:
    """Row ids, best first (score descending, lower id first among equals)."""
    return np.lexsort((np.arange(len(row)), -row.astype(np.float64)))


def tie_survivors(row: np.ndarray, s: int) -> np.ndarray:
    """The s best of a crafted row all equal (the value of the best)."""
    out = row.copy()
    order = _rank_rows(row)
    out[order[:s]] = row[order[0]]
    return out


def tie_block(row: np.ndarray, pos: int, before: int = 3, after: int = 3) -> np.ndarray:
    """A block of equal scores that straddles rank `pos` (1-based) of a crafted row: ranks pos - before .. pos + after
    take the value of rank pos.  pos = k: the tie straddles the end of the result (the lower ids must win);
    pos = s: it straddles the selector's cut (the tied rows below it join the survivors, or — single selector — those
    with higher ids than the cut's stay out)."""
    out = row.copy()
    order = _rank_rows(row)
    a, b = max(0, pos - 1 - before), min(len(row), pos + after)
    out[order[a:b]] = row[order[min(pos, len(row)) - 1]]
    return out


def plain_patterns(n: int) -> dict:
    """Rows every selector meets in some lane distribution: each new row the best so far, the reverse, the same values
    in every 64 (128) rows — a lane (a half-wave's piece) holds one value only —, and one value everywhere."""
    r = np.arange(n)
    return {"ascending": (r - n // 2).astype(np.float32), "descending": (n // 2 - r).astype(np.float32),
            "sawtooth64": (r % 64).astype(np.float32), "sawtooth128": (r % 128).astype(np.float32),
            "all_equal": np.full(n, 7.0, np.float32)}


def spread_ties(n: int, piece: int = 256, waves: int = 4) -> np.ndarray:
    """Two tie blocks for the staged selector behind several waves (wave_topk_sweep4: wave w sweeps the pieces of
    `piece` rows w, w + waves, ...): the best value at rows 0, piece + 1, 2 (piece + 1), ... — one row in each
    successive piece, hence in each wave in turn —, the second best at every 7th row of the rest, every other row
    distinct and below.  The lower ids of each block have to win across the waves' lists."""
    row = (np.arange(n) % 2000 - 3000).astype(np.float32)
    row[np.arange(0, n, 7)] = 3000.0
    row[np.arange(0, n, piece + 1)] = 4000.0
    return row


# ---------------------------------------------------------------------------------------------------------------------
# special values

def special_column(n: int, rng) -> np.ndarray:
    """A column with +inf, -inf, +-FLT_MAX and NaN rows (each several times, spread over the row) among distinct
    integers.  Queries are power-of-two multiples of the column's unit vector: no 0 x inf arises."""
    col = rng.permutation(np.arange(n) - n // 2).astype(np.float32)
    specials = [np.inf, -np.inf, FLT_MAX, -FLT_MAX, np.nan]
    m = min(n, 25)
    where = rng.choice(n, size=m, replace=False)
    for j, r in enumerate(where):
        col[r] = specials[j % 5]
    return col


def topk_full_order(col, k: int):
    """(scores, ids) of the full dense forms on a column that may hold NaN: score descending, NaN behind -inf and ahead
    of the padding, the lower id first among equals and among NaNs; -FLT_MAX / -1 behind the hits."""
    col = np.asarray(col, np.float32)
    n = len(col)
    nan = np.isnan(col)
    key = np.where(nan, -np.inf, col).astype(np.float64)
    order = np.lexsort((np.arange(n), -key, nan))[:k]
    s = np.full(k, -FLT_MAX, np.float32)
    i = np.full(k, -1, np.int64)
    s[:len(order)] = col[order]
    i[:len(order)] = order
    return s, i


def topk_nan_is_padding(col, k: int):
    """The two-level form's convention: a NaN score is never a hit (padding behind the real hits)."""
    col = np.asarray(col, np.float32)
    real = np.nonzero(~np.isnan(col))[0]
    s, i = topk_full_order(col[real], k)
    i[i >= 0] = real[i[i >= 0]]
    return s, i


# ---------------------------------------------------------------------------------------------------------------------
# the harness: patterns as columns, unit-vector queries, the oracle on the column

class Columns:
    """Named score rows of one length n, laid out as the columns of integer matrices X[n, d] (d columns per matrix:
    `matrices()`), with what the model says about each."""

    def __init__(self, n: int, d: int = 64):
        self.n, self.d = n, d
        self.cols, self.meta = [], []

    def add(self, col, **meta) -> int:
        col = np.asarray(col, np.float32)
        assert col.shape == (self.n,)
        self.cols.append(col)
        self.meta.append(meta)
        return len(self.cols) - 1

    def matrices(self):
        """[(first column id, X[n, d])]: columns c0 .. c0 + d - 1 of the set (the last matrix padded with zero columns)."""
        out = []
        for c0 in range(0, len(self.cols), self.d):
            X = np.zeros((self.n, self.d), np.float32)
            for j, col in enumerate(self.cols[c0:c0 + self.d]):
                X[:, j] = col
            out.append((c0, X))
        return out

    def queries(self, ids, c0: int = 0, scale=1.0) -> np.ndarray:
        """Unit vectors (times `scale`, a power of two) of columns `ids` of the matrix that starts at column c0."""
        Q = np.zeros((len(ids), self.d), np.float32)
        for b, c in enumerate(ids):
            assert c0 <= c < c0 + self.d
            Q[b, c - c0] = scale
        return Q


def reference(col, k: int):
    """oracle.dense.topk_desc on the column, padded as the kernels pad (-FLT_MAX / -1)."""
    from oracle import dense as OD
    s, i = OD.topk_desc(np.asarray(col, np.float32)[None, :], k)
    s = s.astype(np.float32)
    s[i < 0] = -FLT_MAX
    return s[0], i[0]


def assert_same(got_s, got_i, exp_s, exp_i, what=None):
    """ids ==, scores bit for bit (any NaN equals any NaN: the kernels do not keep a NaN's payload)."""
    got_s, exp_s = np.asarray(got_s, np.float32), np.asarray(exp_s, np.float32)
    assert np.array_equal(np.asarray(got_i), np.asarray(exp_i)), (what, np.asarray(got_i).tolist(), np.asarray(exp_i).tolist())
    nan = np.isnan(exp_s)
    assert np.array_equal(np.isnan(got_s), nan), (what, got_s.tolist(), exp_s.tolist())
    assert np.array_equal(got_s[~nan].view(np.uint32), exp_s[~nan].view(np.uint32)), (what, got_s.tolist(), exp_s.tolist())


# ---------------------------------------------------------------------------------------------------------------------
# the cases both test files use

A_N = (1, 63, 64, 65, 255, 256, 257, 639, 640, 641, 1023, 1024, 1025, 1279, 1280, 1281, 2047, 2048)
A_K = (1, 2, 10, 16, 17, 32, 33, 63, 64)
A_S = (16, 17, 32, 33, 64, 65, 100)  # beside S = k
B_N = (1, 31, 32, 33, 100, 127, 128, 255, 256, 257, 511, 512, 513, 639, 640, 641, 1023, 1024)
B_K = (1, 2, 5, 10, 16, 17, 31, 32)
B_S = (16, 17, 32, 33, 40)  # beside S = k


def case_columns(n: int, selector: str, seed: int = 0) -> Columns:
    """Every pattern of one n: per k the crafted rows of every realisable S (meta: k, s, kind "craft"), of those the
    tie variants of the smallest S above k and of the S next to the slot limit (kinds "tie_all", "tie_k", "tie_cut"),
    a random row where fewer lanes are populated than k (kind "all_survive"), and the plain patterns (meta k None)."""
    ks, ss = (A_K, A_S) if selector == SINGLE else (B_K, B_S)
    rng = np.random.default_rng(1000 * n + seed + (0 if selector == SINGLE else 7))
    cs = Columns(n)
    for name, col in plain_patterns(n).items():
        cs.add(col, k=None, kind=name)
    for k in ks:
        if k > lanes_populated(n, selector):
            cs.add(craft(n, k, n, selector, rng), k=k, s=n, kind="all_survive")
            continue
        made = []
        for s in sorted({k, *ss}):
            if realisable(n, k, s, selector):
                cs.add(craft(n, k, s, selector, rng), k=k, s=s, kind="craft")
                made.append(s)
        ties = {t for t in (min([s for s in made if s > k], default=None), max([s for s in made if s <= SLOTS[selector]], default=None),
                            min([s for s in made if s > SLOTS[selector]], default=None)) if t is not None}
        for s in sorted(ties):
            base = craft(n, k, s, selector, rng)
            cs.add(tie_survivors(base, s), k=k, s=None, kind="tie_all")
            cs.add(tie_block(base, k), k=k, s=None, kind="tie_k")
            cs.add(tie_block(base, s), k=k, s=None, kind="tie_cut")
    return cs

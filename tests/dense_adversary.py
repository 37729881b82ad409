"""Inputs on which the EXACT dense forms have one right answer (tests/test_dense_adversary*.py; numpy only).

The exact forms — the GEMV scan (dense_scan_topk_kernel), one wave per (query, row) (dense_row_dot), the 32 x 32 fp32-MFMA
tiles (dense_mfma.hip), the panel kernel (dense_panel.hip), the exact two-level top-k — are what every approximate form
is compared with.  Two families pin their arithmetic without a measured number:

- INTEGER data with max|Q| * sum_i |X[r, i]| < 2^24 for every row: every product and every partial sum, in any order,
  with or without FMA, is an integer below 2^24 (times one power of two), exact in fp32.  Every form must return the fp64
  oracle's score BIT FOR BIT and the exact order, ties to the lower id.  Builders: position (one-hot rows, in batches
  whose top-k lists hold every K position: a dropped or doubled K slot, a permutation of one operand only), wide (odd components of 12-13 bits that fp16 / bf16 cannot hold, at
  the first, last and chunk-boundary columns), cancel (+- pairs of large integers that leave a small integer or 0; many
  rows tie at 0 across tile boundaries and the cut), scaled (wide times powers of two, down to fp32-subnormal products).
- REAL edge data against the proven bound of an fp32 dot product in ANY order: |s - exact| <= gamma sum_i |q_i x_i|,
  gamma = u (d + 8) / (1 - u (d + 8)), u = 2^-24 (Higham's gamma_n; + 8 for the cross-lane fold), valid while no product
  underflows and nothing overflows — which the builders assert.  Two views: the full matrix (k = n), and a planted
  top-k whose k + 4 best rows per query are separated by more than 4 bounds, so the expected ids are exact.

form_of restates the route of csrc/dense.hip (dense_route + batched_pass_form); cases() lists the shapes of each form and
coverage_table() shows that every listed d, n, nq and k edge occurs in every form that admits it."""
from __future__ import annotations

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
LIMIT = 1 << 24
U = 2.0 ** -24

# ---- the route --------------------------------------------------------------------------------------------------------
SCAN, ROWWAVES, TILES, PANEL, TWOLEVEL, HI, SMALL = "Scan", "RowWaves", "Tiles", "Panel", "TwoLevel", "Hi", "SmallTwoPass"
FORMS = (SCAN, ROWWAVES, TILES, PANEL, TWOLEVEL, HI, SMALL)
BATCHED_MIN, ROW_WAVES_MAX, PANEL_MIN, MAX_K = 5, 16384, 96, 256
HI_EXTRA_MAX = 96  # the widest candidate cut of the fp16 first pass: kc_max = k + max(k, 96) + 1

# what each form is pinned with (the other pins are deleted for the call)
PINS = {
    SCAN: {}, ROWWAVES: {},
    TILES: {"AMDR_DENSE_PANEL": "0", "AMDR_DENSE_TWO_LEVEL": "0", "AMDR_DENSE_SMALL_HI": "0"},
    PANEL: {"AMDR_DENSE_PANEL": "1", "AMDR_DENSE_TWO_LEVEL": "0", "AMDR_DENSE_SMALL_HI": "0"},
    TWOLEVEL: {"AMDR_DENSE_TWO_LEVEL": "1", "AMDR_DENSE_HI": "0"},
    HI: {"AMDR_DENSE_HI": "1"},
    SMALL: {"AMDR_DENSE_SMALL_HI": "1", "AMDR_DENSE_TWO_LEVEL": "0"},  # + AMDR_DENSE_SMALL_HI_MIN = nq: pins_of()
}
PIN_NAMES = ("AMDR_DENSE_PANEL", "AMDR_DENSE_TWO_LEVEL", "AMDR_DENSE_HI", "AMDR_DENSE_SMALL_HI", "AMDR_DENSE_SMALL_HI_MIN",
             "AMDR_DENSE_NT", "AMDR_DENSE_HI_LEVEL", "AMDR_DENSE_HI_IMAGE")


def pins_of(form, nq):
    p = dict(PINS[form])
    if form == SMALL:
        p["AMDR_DENSE_SMALL_HI_MIN"] = str(nq)
    return p


def _pin(pins, name):
    v = pins.get(name)
    return v[0] if v and v[0] in "01" else ""


def stats_finite(X):
    """DenseFp16Stats::finite of a matrix the fp16 passes support: both maxima finite, |e| < 100 for the largest
    |component| = f 2^e, 1/2 <= f < 1."""
    X = np.asarray(X, dtype=np.float32)
    amax = float(np.max(np.abs(X))) if X.size else 0.0
    with np.errstate(over="ignore"):
        rmax = float(np.sqrt(np.max(np.sum(X.astype(np.float32) ** 2, axis=1, dtype=np.float32)))) if X.size else 0.0
    e = int(np.frexp(np.float32(amax))[1]) if 0.0 < amax <= FLT_MAX else 0
    return bool(amax <= FLT_MAX and rmax <= FLT_MAX and -100 < e < 100)


def form_of(n, d, nq, k, pins, finite=True):
    """The form a fresh handle of an n x d matrix takes for nq queries at depth k under the environment `pins`
    (csrc/dense.hip dense_route, then batched_pass_form without a fusion tail).  finite: stats_finite of the matrix."""
    nt_pin = _pin(pins, "AMDR_DENSE_NT")
    nt = nt_pin == "1" if nt_pin else n * d * 4 > (256 << 20)
    mfma_ok = 64 <= d <= 1024 and d % 64 == 0
    hi_ok = 128 <= d <= 1024 and d % 128 == 0
    if nq >= BATCHED_MIN and n > 0 and mfma_ok:
        chunk = max(32, ((4 << 30) // (n * 4)) // 32 * 32)
        m = min(nq, chunk)
        panel_pin = _pin(pins, "AMDR_DENSE_PANEL")
        panel = panel_pin != "0" and (m >= 1 if panel_pin == "1" else m >= PANEL_MIN)  # (d % 32 == 0 follows from mfma_ok)
        two, hi = _pin(pins, "AMDR_DENSE_TWO_LEVEL"), _pin(pins, "AMDR_DENSE_HI")
        if two != "0":
            tiles = (n + 31) // 32
            kc_max = k + max(k, HI_EXTRA_MAX) + 1
            if (hi != "0" and hi_ok and finite and kc_max <= MAX_K and tiles < (1 << 26) and
                    (tiles >= 2 * kc_max if hi == "1" else nt and tiles >= 64 * kc_max)):
                return HI
            if tiles >= 2 * k if two == "1" else (not panel and nt and tiles >= 64 * k):
                return TWOLEVEL
        slabs = _topk_slabs(n, m)
        small_min = int(pins.get("AMDR_DENSE_SMALL_HI_MIN", "0") or 0)
        if (slabs == 1 and _pin(pins, "AMDR_DENSE_SMALL_HI") != "0" and m >= (small_min if small_min > 0 else 4096) and
                1 <= n <= 1024 and hi_ok and 1 <= k <= 12 and finite):
            return SMALL
        return PANEL if panel else TILES
    if 0 < n <= ROW_WAVES_MAX:
        return ROWWAVES
    return SCAN


def _topk_slabs(n, nq):
    """Slabs of the top-k pass over a score matrix (dense_mfma_plan): >= 16 Ki rows each."""
    sl = max(1, min((256 * 8 + nq - 1) // nq, (n + 16383) // 16384))
    per = ((n + sl - 1) // sl + 63) // 64 * 64
    return max(1, (n + per - 1) // per)


def form_from_plan(text):
    """The form amdr_dense_plan_info reports."""
    for mark, form in (("dense_hi_image_tilemax_kernel", HI), ("dense_hi_tilemax_kernel", HI), ("two-level:", TWOLEVEL),
                       ("dsh_scores_kernel", SMALL), ("dense_all_scores_kernel", ROWWAVES),
                       ("dense_panel_scores_kernel nb=", PANEL), ("dense_mfma_scores_kernel query-tiles-in-LDS", TILES),
                       ("dense_scan_topk_kernel", SCAN)):
        if mark in text:
            return form
    raise AssertionError(f"unknown plan: {text}")


# ---- the shapes ---------------------------------------------------------------------------------------------------------
DS = (4, 60, 64, 68, 128, 192, 256, 260, 320, 768, 832, 1024)
NS = (1, 31, 32, 33, 63, 65, 255, 257, 1023, 1025)
N_SWITCH = (16384, 16385)  # RowWaves -> Scan; d <= 128 there
# one multi-slab n per form, from its plan: the scan cuts slabs of >= 16 rows x 4 waves, the tile kernel gives each wave
# >= 1 tile of a slab, the panel kernel parts of <= 8 x 16 rows, the two-level form ranks >= 2 k tiles; the top-k pass
# over a score matrix has a second slab from 16 385 rows on (N_SWITCH)
N_MULTI = {SCAN: 16385, ROWWAVES: 4099, TILES: 4099, PANEL: 4099, TWOLEVEL: 4099, HI: 6917, SMALL: 1023}
NQS = (1, 4, 5, 8, 9, 31, 32, 33, 95, 96, 97, 129)
K_FULL = -1   # min(n, 256)
K_OVER = -2   # one k > n
KS = (1, 10, K_FULL, K_OVER)
# the largest matrices: 16 385 x 128, or a few thousand rows x 1 024.  One exception: the scan exists only beyond 16 384
# rows, and its loads are compiled per 256-column chunk count (CH = 1 ... 4) — a last float4 dropped at d % 256 != 0 shows
# only at d > 256 — so the scan alone takes every listed d at 16 385 rows (67 MB at d = 1 024, one case each).
MAX_ELEMS, MAX_ROWS_WIDE = 16385 * 128, 6917


def _k_of(kk, n):
    if kk == K_FULL:
        return min(n, MAX_K)
    if kk == K_OVER:
        return n + 3 if n + 3 <= 12 else (n + 7 if n + 7 <= MAX_K else 0)
    return kk


def admits(form, n, d, nq, k):
    """The route gives `form` under its pins and the shape is within the size limit."""
    if k < 1 or k > MAX_K or (n * d > MAX_ELEMS and n > MAX_ROWS_WIDE and not (form == SCAN and n == N_MULTI[SCAN])):
        return False
    return form_of(n, d, nq, k, pins_of(form, nq)) == form


def cases(form, seed=0):
    """A seeded subset of the cross product in which every listed d, n, nq and k that `form` admits occurs: list of
    (n, d, nq, k), grouped by matrix shape."""
    rng = np.random.default_rng(1000 + seed + FORMS.index(form))
    ns = sorted(set(NS + N_SWITCH + (N_MULTI[form],)))
    axes = {"n": ns, "d": list(DS), "nq": list(NQS), "k": list(KS)}
    chosen, seen = [], {a: set() for a in axes}

    def take(n, d, nq, kk):
        k = _k_of(kk, n)
        if (n, d, nq, k) in [(c[0], c[1], c[2], c[3]) for c in chosen] or not admits(form, n, d, nq, k):
            return False
        chosen.append((n, d, nq, k))
        for a, v in (("n", n), ("d", d), ("nq", nq), ("k", kk)):
            seen[a].add(v)
        return True

    # every value of every axis, each completed by a few seeded draws of the other axes
    for axis, vals in axes.items():
        for v in vals:
            if v in seen[axis]:
                continue
            for _ in range(400):
                c = {a: (v if a == axis else vs[int(rng.integers(len(vs)))]) for a, vs in axes.items()}
                if take(c["n"], c["d"], c["nq"], c["k"]):
                    break
    chosen.sort(key=lambda c: (c[0] * c[1], c[1], c[2], c[3]))
    return chosen


def k_labels(k, n):
    """The listed k edges a depth k is on an n-row matrix."""
    return {kk for kk in KS if (kk > 0 and k == kk) or (kk == K_FULL and k == min(n, MAX_K)) or (kk == K_OVER and k > n)}


def coverage(form):
    """{axis: (listed values that occur in cases(form), listed values the form admits anywhere in the cross product)}."""
    ns = sorted(set(NS + N_SWITCH + (N_MULTI[form],)))
    hit = {"d": set(), "n": set(), "nq": set(), "k": set()}
    for n, d, nq, k in cases(form):
        hit["d"].add(d), hit["n"].add(n), hit["nq"].add(nq), hit["k"].update(k_labels(k, n))
    adm = {"d": set(), "n": set(), "nq": set(), "k": set()}
    for n in ns:
        for d in DS:
            for nq in NQS:
                for kk in KS:
                    if admits(form, n, d, nq, _k_of(kk, n)):
                        adm["d"].add(d), adm["n"].add(n), adm["nq"].add(nq), adm["k"].add(kk)
    order = {"d": DS, "n": ns, "nq": NQS, "k": KS}
    return {a: ([v for v in order[a] if v in hit[a]], [v for v in order[a] if v in adm[a]]) for a in order}


def coverage_table():
    name = {K_FULL: "min(n,256)", K_OVER: "k>n"}
    lines = []
    for form in FORMS:
        lines.append(f"{form}: {len(cases(form))} cases")
        for axis, (hit, adm) in coverage(form).items():
            miss = [name.get(v, v) for v in adm if v not in hit]
            lines.append(f"  {axis:>2}: {[name.get(v, v) for v in hit]}" + (f"  MISSING {miss}" if miss else ""))
    return "\n".join(lines)


# ---- the integer family -----------------------------------------------------------------------------------------------
def oracle_topk(S, k):
    """fp64 scores [nq, n] -> (scores f32 [nq, k], ids i64 [nq, k]): descending, ties to the lower id, -FLT_MAX / -1
    behind k > n."""
    nq, n = S.shape
    out_s = np.full((nq, k), -FLT_MAX, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    kk = min(k, n)
    for q in range(nq):
        # candidates: every row at or above the kk-th largest value (all of its ties), then the full order among them
        cand = np.nonzero(S[q] >= np.partition(S[q], n - kk)[n - kk])[0] if 0 < kk < n else np.arange(n)
        order = cand[np.lexsort((cand, -S[q, cand]))[:kk]]
        out_i[q, :kk] = order
        out_s[q, :kk] = S[q, order].astype(np.float32)
    return out_s, out_i


def exact_scores(X, Q):
    return Q.astype(np.float64) @ X.astype(np.float64).T


def assert_integer_budget(X, Q, scale=1.0):
    """max|Q| * max_r sum_i |X[r, i]| < 2^24 on the unscaled integers (scale: the power of two both were multiplied by
    in total, taken out again exactly)."""
    Xi, Qi = X.astype(np.float64), Q.astype(np.float64)
    assert np.array_equal(Xi, np.rint(Xi)) and np.array_equal(Qi, np.rint(Qi)), "integer family: not integers"
    budget = float(np.max(np.abs(Qi), initial=0.0) * np.max(np.sum(np.abs(Xi), axis=1), initial=0.0))
    assert budget < LIMIT, budget
    return budget


def bits_equal(a, b):
    """fp32 arrays equal as uint32 bits, -0.0 and +0.0 counted as equal."""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).copy()
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.uint32).copy()
    a[a == 0x80000000] = 0
    b[b == 0x80000000] = 0
    return np.array_equal(a, b)


def position_X(n, d):
    """One-hot rows: row r = w_r e_{j(r)}, j(r) = r mod d.  Each position has one champion row (w = 3; the others 1 or 2),
    in lap j mod (complete laps), so that the champions sit in every part of the matrix."""
    X = np.zeros((n, d), dtype=np.float32)
    r = np.arange(n)
    j = r % d
    laps = max(1, n // d)
    w = 1 + (r % 2)
    w[(r // d) == (j % laps)] = 3
    X[r, j] = w
    return X


def position_Q(n, d, nq, k, seed=0):
    """Queries with a different integer in every component, another permutation per query: query q holds its k largest
    values, H + k - t, at the window of positions (P - k + q k + t) mod P (P = positions that have a row; query 0 takes the
    last ones) and a seeded permutation of small distinct integers elsewhere; H > d + 2 k puts the champions of exactly
    that window on top.  Returns (Q, the positions the batch covers by construction)."""
    rng = np.random.default_rng(7000 + seed)
    P = min(n, d)
    kw = min(k, P)
    H = d + 2 * k + 1
    Q = np.empty((nq, d), dtype=np.float32)
    small = np.arange(d) - d // 2
    covered = set()
    for q in range(nq):
        win = (P - kw + q * kw + np.arange(kw)) % P  # query 0: the LAST positions, query 1: the first, ...
        rest = np.setdiff1d(np.arange(d), win)
        Q[q, rest] = rng.permutation(small)[:rest.size]
        Q[q, win] = H + kw - np.arange(kw)
        covered.update(int(x) for x in win)
    return Q, covered


def position_case(n, d, nq, k, seed=0):
    X = position_X(n, d)
    Q, want = position_Q(n, d, nq, k, seed)
    assert_integer_budget(X, Q)
    for q in range(nq):
        assert np.unique(Q[q]).size == d
    S = exact_scores(X, Q)
    es, ei = oracle_topk(S, k)
    # coverage: EVERY K position that has a row lies in the top-k of at least one query of the batch
    P = min(n, d)
    got = {int(i) % d for i in ei[ei >= 0]}
    assert want == set(range(P)) and got == set(range(P)), (n, d, nq, k, sorted(set(range(P)) - got)[:8])
    return {"X": X, "Q": Q, "S": S, "scores": es, "ids": ei, "covered": got, "positions": P}


# rows of the matrix that gives every listed d of a form a row at EVERY position (n >= d)
N_ALL_POSITIONS = {SCAN: 16385, ROWWAVES: 1025, TILES: 1025, PANEL: 1025, TWOLEVEL: 1025, HI: 6917, SMALL: 1024}


def position_batch(form, n, d):
    """The cheapest (nq, k) the form admits on an n x d matrix with nq k >= min(n, d): the batch whose windows reach every
    position that has a row.  (129 x 10 for the batched forms — inside k <= 12 of the short-corpus two-pass form and
    k <= 127 of the fp16 first pass —, 4 x 256 where only four queries reach the form.)"""
    P = min(n, d)
    best = None
    for nq in NQS:
        for k in (1, 2, 4, 8, 10, 12, 16, 32, 64, 127, 256):
            if nq * min(k, P) >= P and admits(form, n, d, nq, k) and (best is None or nq * k < best[0] * best[1]):
                best = (nq, k)
    assert best is not None, (form, n, d)
    return best


def position_cases(form):
    """The position family's own cases: every matrix shape of cases(form), and for every d the form admits one with a row
    at every position, each with the batch of position_batch — so that no K slot of any form goes unobserved."""
    shapes = sorted({(n, d) for n, d, _, _ in cases(form)} |
                    {(N_ALL_POSITIONS[form], d) for d in coverage(form)["d"][1]}, key=lambda c: (c[0] * c[1], c[1]))
    return [(n, d) + position_batch(form, n, d) for n, d in shapes]


EDGE_COLS = (0, 3) + tuple(range(28, 36)) + tuple(range(60, 68)) + tuple(range(124, 132)) + tuple(range(252, 260))


def edge_columns(d):
    """The first, last and chunk-boundary columns: 0, 3, 28-35, 60-67, 124-131, 252-259, d-4 ... d-1."""
    return np.array(sorted({c for c in EDGE_COLS if c < d} | {d - 4, d - 3, d - 2, d - 1}), dtype=np.int64)


def wide_X(n, d, seed=0):
    """Components in [-3, 3]; per row up to 16 odd components of magnitude in [2049, 8191] — more bits than fp16 or bf16
    hold — at the edge columns."""
    rng = np.random.default_rng(8000 + seed + 31 * d + n)
    X = rng.integers(-3, 4, size=(n, d)).astype(np.float32)
    cols = edge_columns(d)
    m = min(16, cols.size)
    pick = cols[np.argsort(rng.random((n, cols.size)), axis=1)[:, :m]]  # m distinct edge columns per row
    X[np.arange(n)[:, None], pick] = (2 * rng.integers(1024, 4096, size=(n, m)) + 1) * rng.choice([-1, 1], size=(n, m))
    return X


def wide_Q(d, nq, seed=0):
    """Components in [-3, 3], non-zero at the edge columns (the wide components always count)."""
    rng = np.random.default_rng(8500 + seed + 31 * d + nq)
    Q = rng.integers(-3, 4, size=(nq, d)).astype(np.float32)
    cols = edge_columns(d)
    Q[:, cols] = rng.integers(1, 4, size=(nq, cols.size)) * rng.choice([-1, 1], size=(nq, cols.size))
    return Q


def cancel_X(n, d, k, seed=0):
    """Column i and column i + d/2 hold +L and -L (up to 8 pairs per row, L odd in [2^15, 2^17]); cancel_Q repeats its first
    half in its second, so the pairs cancel exactly whatever the query.  What is left: rho_r at column 0 (weight 3 in
    every query) and rho'_r in {-1, 0, 1} at column 1 (weight in [-1, 1]).  Rows with r mod 64 in [30, 46) have both zero:
    they tie at exactly 0 for every query, in runs that straddle every other 32-row boundary; min(k / 2, n / 4) rows are
    positive and the rest negative, so that the k-th place falls inside the zero group whenever there are enough of them —
    at k = 10 the answer holds five positive rows and rows 30 ... 34, across the boundary at row 32.
    Returns (X, zero rows, positive rows)."""
    rng = np.random.default_rng(9000 + seed + 31 * d + n)
    h = d // 2
    X = np.zeros((n, d), dtype=np.float32)
    m = min(8, h)
    c = np.argsort(rng.random((n, h)), axis=1)[:, :m]  # m distinct columns of the first half per row
    L = (2 * rng.integers(1 << 14, 1 << 16, size=(n, m)) + 1) * rng.choice([-1, 1], size=(n, m))
    X[np.arange(n)[:, None], c] = L
    X[np.arange(n)[:, None], c + h] = -L
    rows = np.arange(n)
    zero = rows[(rows % 64 >= 30) & (rows % 64 < 46)]
    other = np.setdiff1d(rows, zero)
    npos = min(k // 2, n // 4, other.size)
    pos = np.sort(rng.choice(other, size=npos, replace=False)) if npos else np.zeros(0, dtype=np.int64)
    rho = -rng.integers(1, 4, size=n)
    rho[pos] = rng.integers(1, 4, size=pos.size)
    rho[zero] = 0
    rho2 = rng.integers(-1, 2, size=n)
    rho2[zero] = 0
    X[:, 0] += rho
    X[:, 1] += rho2
    return X, zero, pos


def cancel_Q(d, nq, seed=0):
    rng = np.random.default_rng(9500 + seed + 31 * d + nq)
    h = d // 2
    half = rng.integers(-3, 4, size=(nq, h)).astype(np.float32)
    half[:, 0] = 3
    half[:, 1] = rng.integers(-1, 2, size=nq)
    return np.concatenate([half, half], axis=1)


# (a, b): X 2^a, Q 2^b — normal and exactly scaled; the last two leave every product an fp32 subnormal or next to one
SCALES = ((40, -40), (-60, 20), (30, 30))
SUBNORMAL_SCALES = ((-80, -69), (-75, -65))  # 2^(a + b) = 2^-149, 2^-140


def scaled(X, Q, a, b):
    Xs, Qs = np.ldexp(X, a).astype(np.float32), np.ldexp(Q, b).astype(np.float32)
    assert np.array_equal(np.ldexp(Xs.astype(np.float64), -a), X) and np.array_equal(np.ldexp(Qs.astype(np.float64), -b), Q)
    tiny = float(np.finfo(np.float32).tiny)
    for A in (Xs, Qs):  # the operands themselves stay normal
        assert np.all((A == 0) | (np.abs(A) >= tiny)) and np.all(np.abs(A) <= FLT_MAX)
    return Xs, Qs


INT_FAMILIES = ("position", "wide", "cancel") + tuple(f"scale{a:+d}{b:+d}" for a, b in SCALES + SUBNORMAL_SCALES)


def integer_X(family, n, d, k_hint=10):
    """(X fp32, power of two it was scaled by, meta) of an integer family on an n x d matrix."""
    if family == "position":
        return position_X(n, d), 0, {}
    if family == "cancel":
        X, zero, pos = cancel_X(n, d, k_hint)
        return X, 0, {"zero": zero, "pos": pos}
    X = wide_X(n, d)
    if family == "wide":
        return X, 0, {}
    a, b = _scale_of(family)
    return np.ldexp(X, a).astype(np.float32), a, {}


def _scale_of(family):
    for a, b in SCALES + SUBNORMAL_SCALES:
        if family == f"scale{a:+d}{b:+d}":
            return a, b
    raise KeyError(family)


def integer_Q(family, n, d, nq, k):
    """(Q fp32, power of two it was scaled by)."""
    if family == "position":
        return position_Q(n, d, nq, k)[0], 0
    if family == "cancel":
        return cancel_Q(d, nq), 0
    Q = wide_Q(d, nq)
    if family == "wide":
        return Q, 0
    a, b = _scale_of(family)
    return np.ldexp(Q, b).astype(np.float32), b


def integer_expect(X, a, Q, b, k):
    """The fp64 oracle of an integer case: asserts the 2^24 budget on the unscaled integers and that the scaled scores
    are fp32 values (exactly); returns (S fp64 [nq, n], scores f32 [nq, k], ids)."""
    Xi, Qi = np.ldexp(X.astype(np.float64), -a), np.ldexp(Q.astype(np.float64), -b)
    assert_integer_budget(Xi, Qi)
    S = np.ldexp(Qi @ Xi.T, a + b)
    assert np.array_equal(S.astype(np.float32).astype(np.float64), S), "the scaled scores are not fp32 values"
    es, ei = oracle_topk(S, k)
    return S, es, ei


def fp32_scores_in_order(X, Q, perm):
    """S[q][r] accumulated in fp32, one product at a time, in the K order `perm` (numpy fp32 arithmetic: every product and
    every partial sum rounded to fp32)."""
    acc = np.zeros((Q.shape[0], X.shape[0]), dtype=np.float32)
    for i in perm:
        acc = (acc + np.multiply.outer(Q[:, i], X[:, i]).astype(np.float32)).astype(np.float32)
    return acc


# ---- models of wrong kernels (the tests must be able to fail) ------------------------------------------------------------
def model_fp16_operands(X, Q):
    """Both operands rounded to fp16 (values beyond its range clamp), exact products and sums."""
    f = lambda A: np.clip(A.astype(np.float64), -65504, 65504).astype(np.float16).astype(np.float64)
    return (f(Q) @ f(X).T).astype(np.float32)


def model_drop_last4(X, Q):
    return exact_scores(X[:, :-4], Q[:, :-4]).astype(np.float32) if X.shape[1] > 4 else np.zeros((Q.shape[0], X.shape[0]), np.float32)


def model_permute_one_operand(X, Q):
    """The K order of X alone reversed within the first 32-float chunk (columns 0 ... min(d, 32) - 1)."""
    w = min(32, X.shape[1])
    Xp = X.copy()
    Xp[:, :w] = X[:, :w][:, ::-1]
    return exact_scores(Xp, Q).astype(np.float32)


WRONG_MODELS = {"fp16 operands": model_fp16_operands, "last four columns dropped": model_drop_last4,
                "one operand permuted within a 32-float chunk": model_permute_one_operand}


# ---- the real-valued family ---------------------------------------------------------------------------------------------
def gamma(d):
    return (d + 8) * U / (1.0 - (d + 8) * U)


def bound_matrix(X, Q):
    """bound[q][r] = gamma(d) sum_i |Q[q, i] X[r, i]| in fp64; asserts that no product underflows (a non-zero product
    below 2^-100 in magnitude would carry an absolute, not a relative, rounding error) and that nothing overflows."""
    Xa, Qa = np.abs(X.astype(np.float64)), np.abs(Q.astype(np.float64))
    A = Qa @ Xa.T
    assert np.all(np.isfinite(A)) and float(A.max(initial=0.0)) < 2.0 ** 120, "overflow"
    xmin = np.where(Xa > 0, Xa, np.inf).min(initial=np.inf)
    qmin = np.where(Qa > 0, Qa, np.inf).min(initial=np.inf)
    assert xmin * qmin > 2.0 ** -100, "a product may underflow"
    return gamma(X.shape[1]) * A


REAL_KINDS = ("spread", "cancel", "large", "small", "mixture")


def _real_rows(kind, rng, n, d, Q):
    g = rng.standard_normal((n, d))
    g[np.abs(g) < 1e-3] = 1e-3  # (no accidental tiny components: the underflow assertion is about the construction)
    if kind == "spread":  # magnitudes over 2^-20 ... 2^20 within a row
        return np.sign(g) * np.exp2(rng.uniform(-20, 20, size=(n, d)))
    if kind == "large":
        return g / np.linalg.norm(g, axis=1, keepdims=True) * 1e6
    if kind == "small":
        return g / np.linalg.norm(g, axis=1, keepdims=True) * 1e-12
    if kind == "cancel":
        # row r against query r mod nq: x_i = s_i |g_i| sign(q_i), the positive terms scaled so that the score is
        # -(sum |q x|) / 50
        q = Q[np.arange(n) % Q.shape[0]].astype(np.float64)
        s = rng.choice([-1.0, 1.0], size=(n, d))
        s[:, 0], s[:, 1] = 1.0, -1.0
        a = np.abs(q) * np.abs(g)
        f = (a * (s < 0)).sum(axis=1) * 49.0 / ((a * (s > 0)).sum(axis=1) * 51.0)
        X = s * np.abs(g) * np.where(s > 0, f[:, None], 1.0) * np.where(q < 0, -1.0, 1.0)
        return X
    raise KeyError(kind)


def real_case(kind, n, d, nq, seed=0):
    """(X, Q) fp32 of one kind of real-valued edge data."""
    rng = np.random.default_rng(11000 + seed + 131 * d + 7 * n + nq + 1009 * REAL_KINDS.index(kind))
    Q = rng.standard_normal((nq, d))
    Q[np.abs(Q) < 1e-3] = 1e-3
    Q = Q.astype(np.float32)
    if kind == "mixture":
        parts = ("spread", "cancel", "large", "small")
        X = np.empty((n, d))
        which = rng.integers(0, 4, size=n)
        for p, name in enumerate(parts):
            X[which == p] = _real_rows(name, rng, int(np.count_nonzero(which == p)), d, Q)
    else:
        X = _real_rows(kind, rng, n, d, Q)
    X = X.astype(np.float32)
    if kind == "cancel":  # the constructed pairs: sum |q x| is 50 times the score's magnitude, the score negative
        S, A = exact_scores(X, Q), np.abs(Q.astype(np.float64)) @ np.abs(X.astype(np.float64)).T
        r = np.arange(n)
        ratio = A[r % nq, r] / np.abs(S[r % nq, r])
        assert np.all(S[r % nq, r] < 0) and np.all((ratio > 45) & (ratio < 55)), (ratio.min(), ratio.max())
    return X, Q


def planted_case(kind, n, d, nq, k, seed=0):
    """Real-valued data of `kind` with k + 4 planted rows per query (disjoint between queries, anywhere in the matrix):
    their fp64 scores are apart by more than 4 bounds, and every other row stays below the k-th by more than both bounds —
    asserted here — so a kernel inside the bound returns exactly these ids.  The planted part of a row is a multiple of the
    query's column of pinv(Q) (no effect on the other queries) when nq <= d, of the query itself beyond."""
    rng = np.random.default_rng(12000 + seed + 131 * d + 7 * n + 17 * nq + k)
    X, Q = real_case(kind, n, d, nq, seed)
    m = k + 4
    assert n >= nq * m, (n, nq, m)
    S0 = exact_scores(X, Q)
    c = 8.0 * float(np.max(np.abs(S0)))
    rows = rng.choice(n, size=nq * m, replace=False).reshape(nq, m)
    Qd = Q.astype(np.float64)
    dirs = np.linalg.pinv(Qd) if nq <= d else (Qd / np.sum(Qd * Qd, axis=1, keepdims=True)).T  # [d, nq]: Q[q] . dirs[:, q] = 1
    Xd = X.astype(np.float64)
    for q in range(nq):
        level = c * (4.0 + (m - np.arange(m)) / m)  # descending: rows[q][0] is the best
        Xd[rows[q]] += (level - S0[q, rows[q]])[:, None] * dirs[:, q][None, :]  # the row's score for q becomes level
    X = Xd.astype(np.float32)
    S = exact_scores(X, Q)
    B = bound_matrix(X, Q)
    ids = np.empty((nq, k), dtype=np.int64)
    for q in range(nq):
        cand = np.nonzero(S[q] >= np.partition(S[q], n - m)[n - m])[0] if m < n else np.arange(n)
        top = cand[np.lexsort((cand, -S[q, cand]))][:m]
        assert set(top.tolist()) == set(rows[q].tolist()), (kind, n, d, nq, k, q)
        sp, bp = S[q, top], B[q, top]
        assert np.all(sp[:-1] - sp[1:] > 4 * np.maximum(bp[:-1], bp[1:])), (kind, n, d, nq, k, q, "planted rows too close")
        cut, bcut = sp[k - 1], bp[k - 1]
        rest = np.ones(n, dtype=bool)
        rest[top[:k]] = False
        assert np.all(S[q, rest] + B[q, rest] < cut - bcut), (kind, n, d, nq, k, q, "a row reaches the cut")
        ids[q] = top[:k]
    return {"X": X, "Q": Q, "S": S, "bound": B, "ids": ids}


# shapes of the real-valued views, per form (n, d, nq[, k])
FULL_SHAPES = {
    ROWWAVES: ((31, 68, 4), (33, 1024, 1), (255, 768, 3), (256, 260, 9), (65, 4, 129)),
    TILES: ((31, 64, 5), (33, 1024, 33), (255, 768, 32), (256, 320, 95)),
    PANEL: ((31, 64, 96), (33, 1024, 97), (255, 768, 129), (256, 192, 96)),
    SMALL: ((12, 128, 5), (11, 768, 97), (7, 1024, 129)),  # k = n <= 12
}
PLANTED_SHAPES = {
    SCAN: ((16385, 128, 4, 10), (16385, 68, 9, 1), (16385, 4, 2, 10), (16385, 320, 3, 10), (16385, 768, 2, 10),
           (16385, 1024, 1, 10)),  # CH = 1 ... 4
    ROWWAVES: ((1025, 768, 4, 10), (4099, 260, 1, 32), (16384, 60, 33, 1)),
    TILES: ((1025, 768, 33, 10), (4099, 1024, 8, 32), (16385, 64, 95, 10)),
    PANEL: ((2049, 768, 129, 10), (4099, 1024, 96, 1), (16385, 128, 97, 10)),
    TWOLEVEL: ((1025, 768, 33, 10), (4099, 1024, 129, 1), (16385, 128, 9, 32)),
    HI: ((6917, 768, 33, 10), (16385, 128, 129, 1)),
    SMALL: ((1023, 768, 33, 10), (257, 128, 5, 1), (1024, 1024, 64, 12)),
}


def check_bound(scores, ids, S, B):
    """|score - exact[id]| <= bound[id] at every returned place; returns the largest |err| / bound."""
    ex, bd = np.take_along_axis(S, ids, axis=1), np.take_along_axis(B, ids, axis=1)
    ratio = np.abs(scores.astype(np.float64) - ex) / bd
    return float(ratio.max())


def check_full_view(scores, ids, S, B):
    """The full-matrix view (k = n): ids a permutation of [0, n), every score inside its bound, the list descending by the
    kernel's OWN scores with ties to the lower id.  Returns the largest |err| / bound."""
    nq, n = S.shape
    assert scores.shape == (nq, n) and ids.shape == (nq, n)
    for q in range(nq):
        assert np.array_equal(np.sort(ids[q]), np.arange(n)), q
        s, i = scores[q].astype(np.float64), ids[q]
        assert np.all((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (i[:-1] < i[1:]))), q
    return check_bound(scores, ids, S, B)


if __name__ == "__main__":
    print(coverage_table())

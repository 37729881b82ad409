"""Worst-case rounding inputs for the fp16 first passes, and a CPU model of what those passes compute.

Three first passes pick candidates on fp16 roundings of power-of-two-scaled operands and trust a proven per-query bound
eps to decide what to re-score exactly (the dense bound of csrc/dense_fp16.hpp, called by csrc/dense_small_hi.hip
dsh_split_queries_kernel and csrc/dense_hi.hip dense_hi_select_kernel; csrc/maxsim.hip maxsim_select_kernel).  Gaussian test vectors round
like a random walk and sit far below those bounds; the data built here rounds every component by >= 0.45 fp16 ulp in a
chosen direction, so that the first-pass error comes within a constant factor of eps and a bound that is too small (a
dropped factor, a flushed subnormal, a truncating conversion) changes what the kernels return.

Everything is built in the SCALED units of the kernels (largest |component| in [0.5, 1)) and multiplied by powers of
two afterwards: the kernels' own scaling then recovers the scaled values exactly.  Not a test module (no test_ prefix):
tests/test_rounding_adversary.py checks the data on the CPU, tests/test_rounding_adversary_gpu.py runs it on the device.
"""
from __future__ import annotations

import numpy as np

ULP1 = 2.0 ** -10   # fp16 ulp in [1, 2)
SUB = 2.0 ** -24    # fp16 ulp in the subnormal range
MIN_NORMAL = 2.0 ** -14
OFF_Q = 4096        # rounding offsets are multiples of 1/4096 ulp: the scaled values stay exact in fp32


# ---------------------------------------------------------------------------------------------------------------------
# scales and bounds, restated from the kernels (fp64)

def pow2_scale(amax) -> np.ndarray:
    """2^-e with amax = f 2^e, f in [0.5, 1) (frexpf); 1 for amax == 0 — tile_swizzle.hpp pow2_exp / pow2_scale."""
    amax = np.asarray(amax, dtype=np.float64)
    _, e = np.frexp(np.where(amax > 0, amax, 1.0))
    return np.where(amax > 0, np.ldexp(1.0, -e), 1.0)


def dense_scales(X: np.ndarray, Q: np.ndarray):
    """(x_scale, q_scale[nq], R' = largest row norm x x_scale)."""
    X64 = np.asarray(X, np.float64)
    x_scale = float(pow2_scale(np.abs(X64).max()))
    q_scale = pow2_scale(np.abs(np.asarray(Q, np.float64)).max(axis=1))
    r_scaled = float(np.linalg.norm(X64, axis=1).max()) * x_scale
    return x_scale, q_scale, r_scaled


def dense_rel(d: int) -> float:
    """The relative factor of dense_fp16.hpp dense_fp16_eps_scaled, restated (this module is the independent oracle)."""
    return 1.125 * (9.765625e-4 + 2.4e-7 + 2.0 * (d + 8) * 5.9604645e-8)


def dense_eps(X: np.ndarray, Q: np.ndarray) -> np.ndarray:
    """eps_q in the units of the exact score: [rel |q'| R' + 1.125 d 2^-24] / (x_scale q_scale)."""
    d = X.shape[1]
    x_scale, q_scale, r_scaled = dense_scales(X, Q)
    qn = np.linalg.norm(np.asarray(Q, np.float64) * q_scale[:, None], axis=1)
    return (dense_rel(d) * qn * r_scaled + 1.125 * d * 5.9604645e-8) / (x_scale * q_scale)


def maxsim_scales(Q: np.ndarray, D: np.ndarray):
    """(d_scale, q_scale[nq]): the store's power of two and each query's (over all its tokens)."""
    d_scale = float(pow2_scale(np.abs(np.asarray(D, np.float64)).max()))
    q_scale = pow2_scale(np.abs(np.asarray(Q, np.float64)).reshape(Q.shape[0], -1).max(axis=1))
    return d_scale, q_scale


def maxsim_eps(Q: np.ndarray, D: np.ndarray) -> np.ndarray:
    """maxsim_select_kernel, restated in fp64 (this module is the independent oracle): in SCALED units — q' = q q_scale,
    d' = d d_scale, largest |component| in [0.5, 1) —
        [1.5 2^-10 (sum_i |q'_i|) max_t |d'_t| 1.0001 + q_len 256 2^-25] unscale_q unscale_d,
    the bracket times the two unscales 1 / q_scale, 1 / d_scale.  The kernels take both norms on the scaled operands, so
    the bound has no scale range of its own: it holds wherever unscale_q unscale_d is a normal fp32 number."""
    d_scale, q_scale = maxsim_scales(Q, D)
    q_len = Q.shape[1]
    nsum = np.linalg.norm(np.asarray(Q, np.float64) * q_scale[:, None, None], axis=2).sum(axis=1)
    dmax = float(np.linalg.norm(np.asarray(D, np.float64) * d_scale, axis=1).max())
    return (1.5 * 9.765625e-4 * nsum * dmax * 1.0001 + q_len * 256.0 * 2.98023224e-8) / (q_scale * d_scale)


def maxsim_eps_subnormal_term(Q: np.ndarray, D: np.ndarray) -> np.ndarray:
    """The second term of maxsim_eps alone: what is left of the bound when a norm collapses to 0 (norms taken on raw fp32
    components square to 0 below ~2^-75)."""
    d_scale, q_scale = maxsim_scales(Q, D)
    return Q.shape[1] * 256.0 * 2.98023224e-8 / (q_scale * d_scale)


def maxsim_eps_f32(Q: np.ndarray, D: np.ndarray, scaled: bool = True) -> np.ndarray:
    """The bound in the kernels' fp32 arithmetic (ms_tokmax_kernel, ms_split_query_wave, maxsim_select_kernel; the
    summation order inside a row is numpy's, not the lanes').  scaled=False: the norms on the raw components, as the
    kernels took them before — 0, inf or NaN (0 x inf) outside ~2^-75 .. 2^63."""
    f = np.float32
    d_scale, q_scale = maxsim_scales(Q, D)
    ds, qs = f(d_scale), q_scale.astype(f)
    Dx = np.asarray(D, f) * (ds if scaled else f(1))
    Qx = np.asarray(Q, f) * (qs[:, None, None] if scaled else f(1))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        dmax = np.sqrt((Dx * Dx).sum(axis=1, dtype=f)).max()
        nsum = np.sqrt((Qx * Qx).sum(axis=2, dtype=f)).sum(axis=1, dtype=f)
        first = f(1.5) * f(9.765625e-4) * nsum * dmax * f(1.0001)
        second = f(Q.shape[1]) * f(256.0) * f(2.98023224e-8)
        un = (f(1) / qs) * (f(1) / ds)
        return ((first + second) * un if scaled else first + second * un).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the first passes, modelled: fp16 round-to-nearest-even of the scaled operands, exact products, fp64 sums

def to_f16(x: np.ndarray, ftz: bool = False) -> np.ndarray:
    """fp16 image (RNE, as v_cvt_f16_f32) as fp64; ftz: fp16-subnormal results become zero."""
    h = np.asarray(x, np.float32).astype(np.float16).astype(np.float64)
    if ftz:
        h = np.where(np.abs(h) < MIN_NORMAL, 0.0, h)
    return h


def model_dense_hi(X: np.ndarray, Q: np.ndarray, ftz: bool = False) -> np.ndarray:
    """Approximate scores [nq, n] of the dense fp16 first passes, in the units of the exact score."""
    x_scale, q_scale, _ = dense_scales(X, Q)
    Xh = to_f16(np.asarray(X, np.float64) * x_scale, ftz)
    Qh = to_f16(np.asarray(Q, np.float64) * q_scale[:, None], ftz)
    return (Qh @ Xh.T) / (x_scale * q_scale[:, None])


def model_maxsim_hi(Q: np.ndarray, D: np.ndarray, doc_ptr: np.ndarray, ftz: bool = False) -> np.ndarray:
    """Pass 1 of the MaxSim two-pass top-k: hi parts only, max over a document's tokens, sum over query tokens."""
    d_scale, q_scale = maxsim_scales(Q, D)
    Dh = to_f16(np.asarray(D, np.float64) * d_scale, ftz)
    out = np.empty((Q.shape[0], len(doc_ptr) - 1))
    for b in range(Q.shape[0]):
        S = to_f16(np.asarray(Q[b], np.float64) * q_scale[b], ftz) @ Dh.T
        m = np.maximum.reduceat(S, np.asarray(doc_ptr[:-1], np.int64), axis=1)
        out[b] = m.sum(axis=0) / (q_scale[b] * d_scale)
    return out


def exact_dense(X, Q) -> np.ndarray:
    return np.asarray(Q, np.float64) @ np.asarray(X, np.float64).T


def exact_maxsim(Q, D, doc_ptr) -> np.ndarray:
    D64 = np.asarray(D, np.float64)
    out = np.empty((Q.shape[0], len(doc_ptr) - 1))
    for b in range(Q.shape[0]):
        S = np.asarray(Q[b], np.float64) @ D64.T
        out[b] = np.maximum.reduceat(S, np.asarray(doc_ptr[:-1], np.int64), axis=1).sum(axis=0)
    return out


def candidates(approx_row: np.ndarray, eps: float, k: int) -> np.ndarray:
    """The rule all three second passes apply: everything at or above (k-th best approximate score) - 2 eps."""
    tk = np.sort(approx_row)[::-1][k - 1]
    return np.nonzero(approx_row >= tk - 2.0 * eps)[0]


def rounding_shift(x: np.ndarray) -> np.ndarray:
    """How far RNE to fp16 moves each value, in fp16 ulps of its binade; > 0: away from zero, < 0: toward zero."""
    x = np.asarray(x, np.float64)
    h = x.astype(np.float32).astype(np.float16).astype(np.float64)
    a = np.abs(x)
    _, e = np.frexp(np.where(a > 0, a, 1.0))  # a = f 2^e, f in [0.5, 1): binade [2^(e-1), 2^e), ulp 2^(e-11)
    ulp = np.where(a < MIN_NORMAL, SUB, np.ldexp(1.0, e - 11))
    return (np.abs(h) - a) / ulp


# ---------------------------------------------------------------------------------------------------------------------
# value generators (scaled units)

def _offset(rng, size, away: bool) -> np.ndarray:
    """Position inside the ulp, in [0, 1): 1/2 -+ tau with tau in [0.005, 0.03] — RNE moves by 1/2 - tau >= 0.47 ulp."""
    t = rng.integers(20, 123, size=size)
    return ((OFF_Q // 2 + t) if away else (OFF_Q // 2 - t)) / OFF_Q


def normal_values(binade: np.ndarray, mant: np.ndarray, away: np.ndarray, rng, sign=None) -> np.ndarray:
    """2^-j (1 + (m + 1/2 -+ tau) 2^-10): RNE to fp16 moves it by ~2^-11 relative, toward or away from zero."""
    binade = np.asarray(binade)
    off = np.where(away, _offset(rng, binade.shape, True), _offset(rng, binade.shape, False))
    v = np.ldexp(1.0 + (np.asarray(mant) + off) * ULP1, -binade)
    return v if sign is None else v * sign


def subnormal_values(size, rng, away: bool = False, sign=None) -> np.ndarray:
    """(k + 1/2 -+ tau) 2^-24 just below fp16's smallest normal 2^-14 (k in [960, 1022])."""
    k = rng.integers(960, 1022, size=size)
    v = (k + _offset(rng, size, away)) * SUB
    return v if sign is None else v * sign


def _binades(rng, n: int, levels=(1, 2, 3, 4)) -> np.ndarray:
    """The same multiset of binades for every vector (equal norms up to the mantissas), shuffled."""
    b = np.resize(np.asarray(levels), n)
    return rng.permutation(b)


def _tune(x: np.ndarray, binade: np.ndarray, mant: np.ndarray, q: np.ndarray, target: float, mmax: int = 40) -> np.ndarray:
    """Move the mantissas of x's non-zero components (their rounding offsets unchanged) until q . x hits `target`
    to ~1e-8 relative.  x's signs equal q's on every non-zero component, so every step raises the score."""
    mant = mant.copy()
    frac = x / np.ldexp(1.0, -binade)  # 1 + (m + off) 2^-10
    off = np.where(x != 0, (np.abs(frac) - 1.0) / ULP1 - mant, 0.0)
    step = np.where(x != 0, np.abs(q) * np.ldexp(ULP1, -binade), 0.0)
    r = target - float(np.dot(q, x))
    for c in np.argsort(-step):
        if step[c] == 0.0:
            break
        dm = int(np.clip(np.round(r / step[c]), -mant[c], mmax - mant[c]))
        mant[c] += dm
        r -= dm * step[c]
    return np.sign(x) * np.ldexp(1.0 + (mant + off) * ULP1, -binade)


# ---------------------------------------------------------------------------------------------------------------------
# dense cases.  Every builder returns fp32 X [n, d], Q [nq, d] (scaled by powers of two) and what the tests need.

def _pow2(rng, n, lo, hi) -> np.ndarray:
    return np.ldexp(1.0, rng.integers(lo, hi + 1, size=n))


def dense_coherent(rng, d: int, nq: int, n_extra: int = 40, away: bool = False):
    """Row q is query q's direction; every component of both rounds toward zero (away: away from zero):
    err ~ -+2^-10 |q'||x'| (0.81 eps at d = 768).  Returns (X, Q, row_of_query)."""
    n = nq + n_extra
    Xs = np.empty((n, d))
    Qs = np.empty((nq, d))
    for r in range(n):
        b, s = _binades(rng, d), rng.choice([-1.0, 1.0], size=d)
        m = rng.integers(0, 4, size=d)
        Xs[r] = normal_values(b, m, np.full(d, away), rng, s)
        if r < nq:
            Qs[r] = normal_values(b, m, np.full(d, away), rng, s)
    perm = rng.permutation(n)
    X = Xs[perm] * _pow2(rng, 1, -5, 5)[0]
    Q = Qs * _pow2(rng, nq, -8, 8)[:, None]
    row_of = np.argsort(perm)[:nq]
    return X.astype(np.float32), Q.astype(np.float32), row_of


def dense_subnormal(rng, d: int, nq: int, mirror: bool = False):
    """Query: one component ~0.99, the others just below 2^-14 (fp16 subnormals); row: components ~0.99 of the same
    signs.  Flushing the subnormal operands loses ~(d-1) 2^-14 0.99 (0.046 at d = 768, eps 0.033).  mirror: the roles
    of query and row swapped.  Returns (X, Q, row_of_query)."""
    Xs = np.empty((nq, d))
    Qs = np.empty((nq, d))
    for r in range(nq):
        s = rng.choice([-1.0, 1.0], size=d)
        big = normal_values(np.ones(d, int), rng.integers(1000, 1020, size=d), np.zeros(d, bool), rng, s)
        sub = subnormal_values(d, rng, away=bool(r & 1), sign=s)
        p = int(rng.integers(0, d))
        sub[p] = big[p]
        Xs[r], Qs[r] = (sub, big) if mirror else (big, sub)
    perm = rng.permutation(nq)
    X = Xs[perm] * _pow2(rng, 1, -5, 5)[0]
    Q = Qs * _pow2(rng, nq, -8, 8)[:, None]
    return X.astype(np.float32), Q.astype(np.float32), np.argsort(perm)


def dense_outlier(rng, d: int, nq: int, n: int = 300):
    """One sparse row (a single component ~0.9) sets the matrix scale; every other row sits in fp16's subnormal range
    after scaling, with the signs of a query whose components round toward zero.  Returns (X, Q, row_of_query)."""
    Xs = np.zeros((n, d))
    Qs = np.empty((nq, d))
    for r in range(nq):
        s = rng.choice([-1.0, 1.0], size=d)
        Qs[r] = normal_values(_binades(rng, d), rng.integers(0, 4, size=d), np.zeros(d, bool), rng, s)
        Xs[r + 1] = subnormal_values(d, rng, sign=s)
    for r in range(nq + 1, n):
        Xs[r] = subnormal_values(d, rng, sign=rng.choice([-1.0, 1.0], size=d))
    Xs[0, int(rng.integers(0, d))] = 0.9
    X = Xs * 2.0 ** 12
    Q = Qs * _pow2(rng, nq, -6, 6)[:, None]
    return X.astype(np.float32), Q.astype(np.float32), np.arange(1, nq + 1)


DENSE_G0, DENSE_GT, DENSE_GC = 2.4e-5, 4e-5, 3e-6  # relative gaps: k-th target / first competitor, between targets, competitors


def _split_query(rng, d):
    """A query whose components in A round toward zero and in B away from zero (|A| = |B| = d/2, the same binades)."""
    s = rng.choice([-1.0, 1.0], size=d)
    half = d // 2
    A = rng.permutation(d)[:half]
    inA = np.zeros(d, bool)
    inA[A] = True
    b = np.empty(d, int)
    b[inA] = _binades(rng, half)
    b[~inA] = _binades(rng, d - half)
    m = rng.integers(0, 4, size=d)
    q = normal_values(b, m, ~inA, rng, s)
    return q, b, m, s, inA


def _copy_part(rng, q, b, m, s, part, away, base):
    """A copy of q on `part` (zero elsewhere) rounding toward / away from zero, mantissas from `base` up."""
    x = np.zeros_like(q)
    x[part] = normal_values(b[part], m[part] + base, np.full(int(part.sum()), away), rng, s[part])
    return x, m + base


def inversion_rows(rng, q, b, m, s, inA, k: int, nc: int):
    """k targets (copies of q's A part, rounding down, scores s0 (1 + g0/2 + j gt)) and nc competitors (copies of its B
    part, rounding up, s0 (1 - g0/2 - j gc)): exact order targets > competitors, fp16 order the reverse."""
    rows = []
    s0 = None
    for part, away in ((inA, False), (~inA, True)):
        x, _ = _copy_part(rng, q, b, m, s, part, away, 8)
        s0 = float(np.dot(q, x)) if s0 is None else min(s0, float(np.dot(q, x)))
    for j in range(k):
        x, mm = _copy_part(rng, q, b, m, s, inA, False, 8)
        rows.append(_tune(x, b, np.where(inA, mm, 0), q, s0 * (1 + DENSE_G0 / 2 + (k - 1 - j) * DENSE_GT)))
    for j in range(nc):
        x, mm = _copy_part(rng, q, b, m, s, ~inA, True, 8)
        rows.append(_tune(x, b, np.where(~inA, mm, 0), q, s0 * (1 - DENSE_G0 / 2 - j * DENSE_GC)))
    return np.stack(rows)


def dense_inversion(rng, d: int, k: int, groups: int, reps: int, nc: int = 20, n_total=None, tiles=None):
    """`groups` split queries, each `reps` times at different powers of two, with their k targets and nc competitors.
    Layout: a random permutation of the special rows (n_total None: nothing else), or — `tiles` given — special row i in
    32-row tile i mod tiles inside n_total rows of low-scoring filler (a query's rows then lie in distinct tiles).
    Returns dict(X, Q, top[nq, k] (exact order), comp[nq, nc])."""
    qs, blocks = [], []
    for _ in range(groups):
        q, b, m, s, inA = _split_query(rng, d)
        qs.append(q)
        blocks.append(inversion_rows(rng, q, b, m, s, inA, k, nc))
    special = np.concatenate(blocks)
    per = k + nc
    if tiles is None:
        perm = rng.permutation(len(special))
        X = special[perm]
        pos = np.argsort(perm)
    else:
        assert len(special) <= 32 * tiles and per <= tiles and n_total >= 32 * tiles
        i = np.arange(len(special))
        pos = (i % tiles) * 32 + i // tiles
        X = 0.05 * rng.standard_normal((n_total, d)) / np.sqrt(d)
        X[pos] = special
    Q = np.repeat(np.stack(qs), reps, axis=0) * _pow2(rng, groups * reps, -7, 7)[:, None]
    X = X * 2.0 ** int(rng.integers(-4, 5))
    g = np.repeat(np.arange(groups), reps)
    top = np.stack([pos[gi * per: gi * per + k] for gi in g])
    comp = np.stack([pos[gi * per + k: (gi + 1) * per] for gi in g])
    return dict(X=X.astype(np.float32), Q=Q.astype(np.float32), top=top, comp=comp)


# ---------------------------------------------------------------------------------------------------------------------
# MaxSim cases (dim 128).  Returns dict(D [tokens, 128], doc_ptr, Q [nq, q_len, 128], ...)

def _ms_store(rng, docs):
    """Docs given as lists of token rows; a few random extra tokens (low scores, same norm class) make them ragged."""
    out = []
    for toks in docs:
        extra = int(rng.integers(0, 40))
        e = [normal_values(_binades(rng, 128, (3, 4, 5, 6)), rng.integers(0, 8, 128), rng.random(128) < 0.5, rng,
                           rng.choice([-1.0, 1.0], size=128)) for _ in range(extra)]
        rows = list(toks) + e
        out.append(np.stack([rows[i] for i in rng.permutation(len(rows))]))
    doc_ptr = np.concatenate([[0], np.cumsum([len(x) for x in out])]).astype(np.int64)
    return np.concatenate(out), doc_ptr


def maxsim_coherent(rng, nq: int, q_len: int, n_other: int = 20):
    """Document q holds a round-down copy of every token of query q (also rounding down): err ~ -2^-10 sum |q_i||d_i|
    (0.66 eps).  Returns dict(D, doc_ptr, Q, doc_of)."""
    Qs = np.empty((nq, q_len, 128))
    docs = []
    for b in range(nq + n_other):
        toks = []
        for i in range(q_len):
            bb, s, m = _binades(rng, 128), rng.choice([-1.0, 1.0], size=128), rng.integers(0, 4, size=128)
            toks.append(normal_values(bb, m, np.zeros(128, bool), rng, s))
            if b < nq:
                Qs[b, i] = normal_values(bb, m, np.zeros(128, bool), rng, s)
        docs.append(toks)
    order = rng.permutation(len(docs))
    D, doc_ptr = _ms_store(rng, [docs[o] for o in order])
    Q = Qs * _pow2(rng, nq, -6, 6)[:, None, None]
    return dict(D=(D * 2.0 ** 3).astype(np.float32), doc_ptr=doc_ptr, Q=Q.astype(np.float32), doc_of=np.argsort(order)[:nq])


def maxsim_inversion(rng, q_len: int, k: int, groups: int, reps: int, nc: int):
    """Per group a split query (every token: A part rounds down, B part up); k target documents hold A-part copies of
    its tokens (round down), nc competitors B-part copies (round up); exact scores as in inversion_rows.
    Returns dict(D, doc_ptr, Q, top[nq, k], comp[nq, nc])."""
    qs, docs = [], []
    for _ in range(groups):
        parts = [_split_query(rng, 128) for _ in range(q_len)]
        q = np.stack([p[0] for p in parts])
        qs.append(q)
        copies = []
        for part_a, away, base in ((True, False, 8), (False, True, 8)):
            copies.append([_copy_part(rng, p[0], p[1], p[2], p[3], p[4] if part_a else ~p[4], away, base) for p in parts])
        s0 = min(sum(float(np.dot(p[0], c[0])) for p, c in zip(parts, cs)) for cs in copies)

        def doc(part_a, away, score):
            toks = [_copy_part(rng, p[0], p[1], p[2], p[3], p[4] if part_a else ~p[4], away, 8) for p in parts]
            # spread the adjustment over the tokens: token i takes its share of the residual
            cur = sum(float(np.dot(p[0], t[0])) for p, t in zip(parts, toks))
            out = []
            for p, (x, mm) in zip(parts, toks):
                want = float(np.dot(p[0], x)) + (score - cur) / q_len
                sel = p[4] if part_a else ~p[4]
                out.append(_tune(x, p[1], np.where(sel, mm, 0), p[0], want))
            return out
        for j in range(k):
            docs.append(doc(True, False, s0 * (1 + DENSE_G0 / 2 + (k - 1 - j) * DENSE_GT)))
        for j in range(nc):
            docs.append(doc(False, True, s0 * (1 - DENSE_G0 / 2 - j * DENSE_GC)))
    per = k + nc
    order = rng.permutation(len(docs))
    D, doc_ptr = _ms_store(rng, [docs[o] for o in order])
    pos = np.argsort(order)
    g = np.repeat(np.arange(groups), reps)
    Q = np.repeat(np.stack(qs), reps, axis=0) * _pow2(rng, groups * reps, -6, 6)[:, None, None]
    top = np.stack([pos[gi * per: gi * per + k] for gi in g])
    comp = np.stack([pos[gi * per + k: (gi + 1) * per] for gi in g])
    return dict(D=(D * 2.0 ** -2).astype(np.float32), doc_ptr=doc_ptr, Q=Q.astype(np.float32), top=top, comp=comp)


def maxsim_subnormal(rng, nq: int, q_len: int, k: int, n_docs: int):
    """Query tokens in fp16's subnormal range (token 0 has one component ~0.99 and sets the query's scale); each query
    has k target documents whose tokens carry the signs of its subnormal tokens at magnitudes ~0.5-0.99, the other
    documents random signs.  Flushed subnormal operands would drop the targets' whole lead (~0.2 against eps ~0.013).
    Returns dict(D, doc_ptr, Q, top=None)."""
    Qs = np.empty((nq, q_len, 128))
    signs = rng.choice([-1.0, 1.0], size=(nq, q_len, 128))
    for b in range(nq):
        for i in range(q_len):
            Qs[b, i] = subnormal_values(128, rng, away=bool(i & 1), sign=signs[b, i])
        Qs[b, 0] = 0.0
        Qs[b, 0, int(rng.integers(0, 128))] = 0.99
    docs = []
    owner = rng.permutation(n_docs)[: nq * k].reshape(nq, k)
    own = {int(d): b for b in range(nq) for d in owner[b]}
    for dd in range(n_docs):
        toks = []
        for i in range(q_len):
            s = signs[own[dd], i] if dd in own and i > 0 else rng.choice([-1.0, 1.0], size=128)
            toks.append(normal_values(np.ones(128, int), rng.integers(0, 1000, 128), rng.random(128) < 0.5, rng, s))
        docs.append(toks)
    D, doc_ptr = _ms_store(rng, docs)
    Q = Qs * _pow2(rng, nq, -6, 6)[:, None, None]
    return dict(D=(D * 2.0 ** 5).astype(np.float32), doc_ptr=doc_ptr, Q=Q.astype(np.float32), top=None)


def ms_cand_cap(k: int) -> int:
    """maxsim.hip ms_cand_cap: max(64, next_pow2(2 k)); more candidates re-score every document."""
    c = 1
    while c < 2 * k:
        c *= 2
    return max(64, c)


# ---------------------------------------------------------------------------------------------------------------------
# the scale range of the MaxSim bound: a case times exact powers of two

# (store exponent, query exponent); the exact scores of maxsim_inversion stay inside fp32's normal range for all of them
MAXSIM_SCALE_PAIRS = [(0, 0), (-90, 0), (0, -90), (-75, 0), (-45, -45), (70, 0), (0, 70), (45, 45)]


def maxsim_scaled(c: dict, sd: int, sq: int) -> dict:
    """The case with (D 2^sd, Q 2^sq), exactly (no component leaves fp32's normal range): the fp16 images of the scaled
    operands, the first-pass errors relative to the scores and the oracle's order are those of the unscaled case."""
    out = dict(c)
    for name, e in (("D", sd), ("Q", sq)):
        x = np.ldexp(np.asarray(c[name], np.float64), e)
        x32 = x.astype(np.float32)
        nz = x != 0
        assert np.array_equal(x32.astype(np.float64), x) and np.all(np.abs(x[nz]) >= 2.0 ** -126), (name, e)
        out[name] = x32
    return out


# ---------------------------------------------------------------------------------------------------------------------
# shape edges of the MaxSim two-pass top-k (random unit rows)

def unit_rows(rng, n: int, d: int = 128) -> np.ndarray:
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def topk_exact(exact: np.ndarray, k: int):
    """(scores, ids) [nq, k] of an fp64 score matrix: descending, ties -> lower id."""
    ids = np.stack([np.lexsort((np.arange(exact.shape[1]), -row))[:k] for row in exact])
    return np.take_along_axis(exact, ids, axis=1), ids


MS_LONG_LENS = (513, 1000, 481, 511, 512, 640)  # more than 15 tiles of 32 tokens each (maxsim_items_kernel's last class)


def maxsim_long_docs(rng, nq: int, q_len: int):
    """80 documents: lengths 1, 448, 449, 480 (14 and 15 tiles: below and on the items kernel's clamp) and the six of
    MS_LONG_LENS (16 .. 32 tiles) first, in the middle and last — the last document has 513 tokens, one token in its
    final tile, so that tile reads on into the images' padding — the rest 1 .. 60.  Query b's first three tokens are
    planted (noisy copies, renormalised) in long document b mod 6 at tokens b, len / 2 + b and len - 1 - b (query 0: the
    very last token of the store).  Returns dict(D, doc_ptr, Q, long = ids of the documents with more than 15 tiles)."""
    n = 80
    lens = rng.integers(1, 61, size=n)
    place = {0: 1000, 1: 448, 2: 1, 3: 481, 38: 449, 39: 480, 40: 511, 41: 640, 78: 512, 79: 513}
    for i, v in place.items():
        lens[i] = v
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    D = unit_rows(rng, int(doc_ptr[-1]))
    Q = unit_rows(rng, nq * q_len).reshape(nq, q_len, 128)
    long_of = {v: i for i, v in place.items()}
    for b in range(nq):
        d = long_of[MS_LONG_LENS[b % len(MS_LONG_LENS)]]
        ln = int(lens[d])
        for j, pos in enumerate((b, ln // 2 + b, ln - 1 - b)[:min(3, q_len)]):
            v = Q[b, j] + 0.3 * unit_rows(rng, 1)[0]
            D[doc_ptr[d] + pos] = v / np.linalg.norm(v)
    long_ids = np.nonzero((lens + 31) // 32 > 15)[0]
    return dict(D=D, doc_ptr=doc_ptr, Q=Q, long=long_ids)


def maxsim_short_docs(rng, n_docs: int, nq: int, q_len: int = 32):
    """n_docs documents of 1 .. 12 random unit tokens (the first four: 1, 12, 1, 12).  A prefix of the store is a store:
    doc_ptr[:m + 1] and D[:doc_ptr[m]], and the exact scores of the prefix are the first m columns."""
    lens = rng.integers(1, 13, size=n_docs)
    lens[:4] = [1, 12, 1, 12]
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return dict(D=unit_rows(rng, int(doc_ptr[-1])), doc_ptr=doc_ptr, Q=unit_rows(rng, nq * q_len).reshape(nq, q_len, 128))


def maxsim_depth_docs(rng, nq: int, q_len: int = 32):
    """1 100 documents for depths up to 256: 850 of 1 .. 6 tokens and 250 of 12 .. 80, shuffled (under 15 k tokens).  A
    score grows with the length, so the 256 best are the long documents spread over ~2.5 — with equal lengths the top
    quarter of 1 100 random scores sits within ~1 and one rank position in seven is a near-tie at 1e-4."""
    lens = rng.permutation(np.concatenate([rng.integers(1, 7, size=850), rng.integers(12, 81, size=250)]))
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return dict(D=unit_rows(rng, int(doc_ptr[-1])), doc_ptr=doc_ptr, Q=unit_rows(rng, nq * q_len).reshape(nq, q_len, 128))


def maxsim_prefix(c: dict, m: int):
    return c["D"][: int(c["doc_ptr"][m])], c["doc_ptr"][: m + 1]


def maxsim_mixed_overflow(rng):
    """300 documents: 200 near-duplicates of one 40-token document (differing in the 4th decimal), interleaved with 100
    random ones of 30 .. 100 tokens; 16 queries: the even ones aimed at the cluster (20 noisy copies of its tokens + 12
    random tokens: the 200 duplicates tie inside the margin, far more than the candidate list holds), the odd ones random
    (the cluster scores like any 40-token document: below their cut).  An aimed and a random query share every pass-1 wave.
    Returns dict(D, doc_ptr, Q, aimed = query ids, cluster = document ids)."""
    base = unit_rows(rng, 40)
    docs, cluster = [], []
    for i in range(300):
        if i % 3 != 2:
            cluster.append(i)
            docs.append(base + 1e-4 * rng.standard_normal(base.shape).astype(np.float32))
        else:
            docs.append(unit_rows(rng, int(rng.integers(30, 101))))
    D = np.concatenate(docs).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    doc_ptr = np.concatenate([[0], np.cumsum([len(x) for x in docs])]).astype(np.int64)
    Q = unit_rows(rng, 16 * 32).reshape(16, 32, 128)
    aimed = np.arange(0, 16, 2)
    for b in aimed:
        Q[b, :20] = base[:20] + 0.05 * rng.standard_normal((20, 128)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=2, keepdims=True)
    return dict(D=D, doc_ptr=doc_ptr, Q=Q.astype(np.float32), aimed=aimed, cluster=np.array(cluster))


MS_SHARED_DOC = 100  # the planted document of maxsim_shared


def maxsim_shared(rng):
    """201 documents of 1 .. 12 random unit tokens, but document MS_SHARED_DOC: 70 tokens (3 tiles), noisy copies of the
    tokens of query 0 at norm 0.35 — the best document of query 0 by far (~10 against ~5), and for any other query a
    document of short tokens far below its cut (~2.5).  In a batch that holds query 0 c times, document MS_SHARED_DOC is a
    candidate of exactly c queries.  Returns dict(D, doc_ptr, pool [30, 32, 128]): pool[0] is query 0, the rest random."""
    c = maxsim_short_docs(rng, 201, 30)
    lens = np.diff(c["doc_ptr"])
    lens[MS_SHARED_DOC] = 70
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    D = unit_rows(rng, int(doc_ptr[-1]))
    q0 = c["Q"][0]
    v = q0[np.arange(70) % 32] + 0.3 * unit_rows(rng, 70)
    D[doc_ptr[MS_SHARED_DOC]: doc_ptr[MS_SHARED_DOC + 1]] = 0.35 * v / np.linalg.norm(v, axis=1, keepdims=True)
    return dict(D=D, doc_ptr=doc_ptr, pool=c["Q"])


def maxsim_shared_batch(pool: np.ndarray, copies: int, nq: int = 24) -> np.ndarray:
    """`copies` times query 0, then nq - copies others of the pool."""
    return np.concatenate([np.repeat(pool[:1], copies, axis=0), pool[1: 1 + nq - copies]]).astype(np.float32)


def candidate_status(approx_row: np.ndarray, eps: float, k: int, slack: float) -> np.ndarray:
    """+1: a candidate by more than `slack`, -1: none by more than `slack`, 0: too close to the threshold for a model
    whose sums are not the kernel's fp32 sums to say."""
    thr = np.sort(approx_row)[::-1][k - 1] - 2.0 * eps
    return np.where(approx_row >= thr + slack, 1, np.where(approx_row < thr - slack, -1, 0))


def oracle_rank_mask(es: np.ndarray, tol: float) -> np.ndarray:
    """Positions of a descending oracle score row whose neighbours are both more than 2 tol away: where ranks are compared."""
    ok = np.abs(np.diff(es)) > 2 * tol
    return np.concatenate([[True], ok]) & np.concatenate([ok, [True]])


# ---------------------------------------------------------------------------------------------------------------------
# the GPU tests' driver of the MaxSim forms (needs the native library: `nat` is legal_rag_amd._native, loaded)

# documents per block of pass 1: the default, one, and seven (blocks that end inside the store's groups)
MS_VARIANTS = [{}, {"AMDR_MAXSIM_DOCS": "1"}, {"AMDR_MAXSIM_DOCS": "7"}]


def ms_forms(nat, monkeypatch, D, doc_ptr, Q, k, variants, ref_ids=None, rows=None, two_pass=None):
    """(scores, ids) of the one-pass form (AMDR_MAXSIM_TWOPASS=0), which equal ref_ids where given; every variant of the
    two-pass form — asserted to BE the two-pass form — returns the same ids and the same score bits.  rows: the queries
    compared (default: all); two_pass: a list that receives every variant's (scores, ids)."""
    rows = slice(None) if rows is None else rows
    monkeypatch.setenv("AMDR_MAXSIM_TWOPASS", "0")
    idx = nat.MaxSimIndex(D, doc_ptr)
    s1, i1 = idx.search(Q, k)
    idx.close()
    monkeypatch.delenv("AMDR_MAXSIM_TWOPASS")
    if ref_ids is not None:
        assert np.array_equal(i1, ref_ids)
    n_docs, nq = len(doc_ptr) - 1, len(Q)
    for env in variants:
        for n_, v in env.items():
            monkeypatch.setenv(n_, v)
        idx = nat.MaxSimIndex(D, doc_ptr)
        assert "two-pass" in idx.plan_info(nq), idx.plan_info(nq)
        assert nat.maxsim_workspace_plan(n_docs, True, nq, k, nq, k)[1] > (nq * n_docs * 4 + 255) // 256 * 256, (n_docs, nq, k)
        s2, i2 = idx.search(Q, k)
        idx.close()
        for n_ in env:
            monkeypatch.delenv(n_)
        if two_pass is not None:
            two_pass.append((s2, i2))
        if ref_ids is not None:
            assert np.array_equal(i2, ref_ids), env
        assert np.array_equal(i2[rows], i1[rows]), env
        assert np.array_equal(s2[rows].view(np.uint32), s1[rows].view(np.uint32)), env
    return s1, i1


def ms_check(nat, monkeypatch, D, doc_ptr, Q, k, top, variants):
    """ms_forms against the fp64 oracle's ids (oracle/maxsim.py), which are `top` where the construction fixes them."""
    from oracle import maxsim as OM
    _, ref_ids = OM.maxsim_topk(Q, D, doc_ptr, k)
    if top is not None:
        assert np.array_equal(ref_ids, top)
    return ms_forms(nat, monkeypatch, D, doc_ptr, Q, k, variants, ref_ids)

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
    """2^-e with amax = f 2^e, f in [0.5, 1) (frexpf); 1 for amax == 0 — dense_fp16.hpp dense_fp16_exp / dense_fp16_scale."""
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
    """maxsim_select_kernel: 1.5 2^-10 sum_i |q_i| max_t |d_t| 1.0001 + q_len 256 2^-25 unscale_q unscale_d."""
    d_scale, q_scale = maxsim_scales(Q, D)
    q_len = Q.shape[1]
    nsum = np.linalg.norm(np.asarray(Q, np.float64), axis=2).sum(axis=1)
    dmax = float(np.linalg.norm(np.asarray(D, np.float64), axis=1).max())
    return 1.5 * 9.765625e-4 * nsum * dmax * 1.0001 + q_len * 256.0 * 2.98023224e-8 / (q_scale * d_scale)


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

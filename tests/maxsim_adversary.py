"""Inputs on which EVERY MaxSim form has one right answer (tests/test_maxsim_adversary*.py; numpy only).

The ColBERT channel (csrc/maxsim.hip, csrc/maxsim_core.hpp, the scoped form of csrc/scope.hip) scores with the fp32-input
pair and blocked kernels, the split-fp16 pair kernel, the LDS ring kernel, the two-pass route (hi-only first pass, select,
items, ring re-score or overflow kernel, final top-k) and the scoped kernel.  Every builder here returns a store, queries,
the expected fp32 score matrix of the split-fp16 forms and of the fp32-input forms, and asserts an exactness CERTIFICATE
in fp64 arithmetic (split_expected / f32_expected):

- the split is emulated as the code defines it: s = 2^-e of the largest |component| (pow2_exp), hi = fp16(x s),
  lo = fp16((x s - hi) 2048), and hi + lo / 2048 == x s exactly;
- for every query, all terms of the hi.hi accumulator are multiples of one unit u with sum |terms| < LIMIT u
  (LIMIT = 2^24), and so are the terms of the cross accumulator (ah x ql + al x qh) with a unit of its own;
- the fold fma(cross, 1/2048, main) is exact (families with fold_exact=False state the ONE rounding it makes instead);
- the sum over the query tokens of the unscaled maxima is exact in fp32 (multiples of one unit, sum |.| < LIMIT units).

Under it any accumulation order, with or without FMA, gives the same fp32 number, and oracle/maxsim.py's fp64 value is
that number.  The fp32-input forms need the same bound on the plain products.  A zero compares by value (scores() may
return either sign, top-k outputs +0.0); everything else as uint32 bits (same_scores).

Families (FAMILIES), all seeded:
  integers   components in [-15, 15], one at +-15 in token 0 of document 0 and in row 0 of every query; every document is
             followed by a twin (the same tokens, permuted): scores are integers below 2^20, at least half of the cuts
             fall inside a tie group.  `short` is the same with 1 .. 12 tokens per document from a pool of 40 base
             documents (ties in masses) for the corpus sizes around the select kernel's row selectors.
  position   one-hot tokens +- w e_c: 128 documents, document d holds component d at tile row d mod 32 (second 32-token
             block of a 64-token tile from document 96 on) with a weight of its own; query b < 4 holds component 4 i + b
             in row i, queries 4 .. 7 the same with the rows reversed.  A dropped, doubled or permuted K slot, fragment
             row or query row moves a document in some list.
  bait       per remainder R of BAIT_REMAINDERS a document of R tokens whose every similarity is a distinct negative
             integer, the least negative in its LAST token, followed by a bait of 64 tokens that score far higher; the
             document of one remainder once more as the store's last, against the zero padding.
  wide       a 22-bit store ((1024 + A) / 2048 + B / 2^22, lo non-zero and exact) against one-hot queries +- 2^p with two
             live rows of {0, 15, 16, 31} (the al x qh MFMA); wide_rev the reverse (one-hot store, four wide query rows:
             the ah x ql MFMA).  The fp32-input forms return the same bits.
  both_wide  one-hot on both sides, q_len = 1: the split forms return round_fp32(a_hi b_hi + (a_hi b_lo + a_lo b_hi) /
             2048) — the documented form minus its lo.lo term —, the fp32-input forms the rounded fp64 product, and the two
             differ for some pair.  rounded_lo is the same with 24-bit components, whose lo IS rounded (hi + lo / 2048 is
             then within 2^-24 of x s, asserted instead of equality): still one right answer, since every accumulator term is
             exact; it is the family that tells a truncated lo from a rounded one, which no exactly split input can.
  scaled     integers and wide times 2^sd (store) and 2^sq (queries) over RA.MAXSIM_SCALE_PAIRS: expected scores scale.
  twopass    200+ documents: 100 clones of one document that tie for every query, k + 4 planted documents per listed
             query, separated from the rest by more than 2 eps of the fp64 model of the candidate rule (RA.maxsim_eps,
             RA.ms_cand_cap); a query without planted documents has the 100 clones tie at its cut: its list overflows.

Wrong-kernel models (FAULTS; model_scores / model_topk restate the tile walk of ms_pair_doc_h with one fault each) and
the family that catches each:
  max0 (maximum starts at 0, not -FLT_MAX)                bait        mask_gt (mask > instead of >= on the last tile)  bait
  nomask (reads on into the next document)                 bait        early16 (second 16-row block skipped at 17)      bait
  dropk (one K chunk dropped)                              position    qrows (query rows >= q_len neither zeroed nor
  lo_trunc (lo truncated, not rounded)                     rounded_lo         left out of the sum)                        integers
  cross_al / cross_ah (one cross term missing)             wide / wide_rev
  inv1024 (1/2048 applied as 1/1024)                       wide        tie_high (ties to the higher id)                  integers
  cut_first (the cut taken before the tie break)           integers
(In the kernels a query row >= q_len is zeroed AND left out of the finishing sum; either guard alone hides the loss of
the other, so the model removes both.)

form_of restates ms_route of csrc/maxsim.hip; cases() lists what the GPU driver runs and coverage_table() shows that every
listed document length, corpus size, batch size, query length and depth kind occurs in every form that admits it."""
from __future__ import annotations

import functools

import numpy as np

import rounding_adversary as RA

FLT_MAX = float(np.finfo(np.float32).max)
LIMIT = 1 << 24
DIM = 128

# ---- the route ----------------------------------------------------------------------------------------------------------
PAIRF32, PAIRHALF, BLOCKED, RING, TWOPASS, SCOPED = "PairF32", "PairHalf", "Blocked", "Ring", "TwoPass", "Scoped"
FORMS = (PAIRF32, PAIRHALF, BLOCKED, RING, TWOPASS, SCOPED)
SPLIT_FORMS = (PAIRHALF, RING, TWOPASS, SCOPED)
K_MSQ, K_MS_DOCS, MAX_K, SELECT_ROWS_MAX = 8, 8, 256, 2048
PIN_NAMES = ("AMDR_MAXSIM_F16X3", "AMDR_MAXSIM_TWOPASS", "AMDR_MAXSIM_DOCS", "AMDR_SCOPE_SLAB")
P_DEF, P_F32, P_ONE = {}, {"AMDR_MAXSIM_F16X3": "0"}, {"AMDR_MAXSIM_TWOPASS": "0"}
DOCS7 = ({}, {"AMDR_MAXSIM_DOCS": "7"})


def _off(pins, name):
    return pins.get(name, "")[:1] == "0"


def form_of(n_docs, nq, k, want_topk, pins, finite=True):
    """ms_route: the form of a call of nq queries at depth k (want_topk: search / search_device; False: scores) on a
    store of n_docs documents under the environment `pins`; finite: the store holds no NaN / infinity (it has images)."""
    half = finite and not _off(pins, "AMDR_MAXSIM_F16X3")
    batch = nq >= K_MSQ
    if want_topk and half and batch and 4 * k <= n_docs and not _off(pins, "AMDR_MAXSIM_TWOPASS"):
        return TWOPASS
    if batch and half:
        return RING
    if batch and (n_docs + K_MS_DOCS - 1) // K_MS_DOCS <= 65535:
        return BLOCKED
    return PAIRHALF if half else PAIRF32


def form_from_plan(text):
    """The form amdr_maxsim_plan_info reports (it has no k: the route at depth 1)."""
    for mark, form in (("two-pass top-k", TWOPASS), ("maxsim_scores_ring_kernel split-fp16", RING),
                       ("maxsim_scores_h_kernel split-fp16", PAIRHALF), ("maxsim_scores_blocked_kernel fp32-input", BLOCKED),
                       ("maxsim_scores_kernel fp32-input", PAIRF32)):
        if mark in text:
            return form
    raise AssertionError(f"unknown plan: {text}")


def rows_bytes(n_docs, nq):
    """ms_rows_bytes: all a one-pass call uses; the two-pass layout is larger."""
    return (nq * n_docs * 4 + 255) // 256 * 256


# ---- the split and the certificate -------------------------------------------------------------------------------------
def split(x, s):
    """(hi, lo) of ms_split as fp64: v = x s, hi = fp16(v), lo = fp16((v - hi) 2048)."""
    v = (np.asarray(x, np.float32) * np.float32(s)).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), np.asarray(x, np.float64) * float(s))  # a power of two: exact
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def unit_exp(x):
    """e of the largest 2^e that divides every non-zero element (None: all zero)."""
    x = np.abs(np.asarray(x, np.float64))
    x = x[x != 0]
    if x.size == 0:
        return None
    m, e = np.frexp(x)
    mi = np.ldexp(m, 53).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    return int((e - 53 + np.log2(low).astype(np.int64)).min())


def assert_budget(absum, *units, limit=LIMIT):
    """Every term a multiple of 2^(sum of units), the largest sum of |terms| below limit of them."""
    if any(u is None for u in units) or absum == 0:
        return
    assert absum < limit * 2.0 ** sum(units), (absum, units, limit)


def _f32_exact(v):
    with np.errstate(over="ignore"):
        r = np.asarray(v, np.float64).astype(np.float32)
    return np.array_equal(r.astype(np.float64), v), r


def _finish(V, doc_ptr, unscale, limit):
    """max over a document's tokens, times the unscale, sum over the query rows — asserted exact in fp32."""
    M = np.maximum.reduceat(V, np.asarray(doc_ptr[:-1], np.int64), axis=1) * unscale
    ok, _ = _f32_exact(M)
    assert ok and np.all((M == 0) | (np.abs(M) >= 2.0 ** -126))
    if M.shape[0] > 1:  # (one query row: nothing is added)
        assert_budget(np.abs(M).sum(axis=0).max(), unit_exp(M), limit=limit)
    tot = M.sum(axis=0)
    ok, r = _f32_exact(tot)
    assert ok
    return r


def split_expected(D, doc_ptr, Q, fold_exact=True, split_exact=True, limit=LIMIT):
    """The fp32 score matrix of the split-fp16 forms, with the certificate asserted."""
    d_scale, q_scale = RA.maxsim_scales(Q, D)
    Dh, Dl = split(D, d_scale)
    Ds = np.asarray(D, np.float64) * d_scale
    if split_exact:
        assert np.array_equal(Dh + Dl / 2048.0, Ds)
    else:
        assert np.max(np.abs(Dh + Dl / 2048.0 - Ds)) <= 2.0 ** -24
    uDh, uDl = unit_exp(Dh), unit_exp(Dl)
    out = np.empty((len(Q), len(doc_ptr) - 1), np.float32)
    for b in range(len(Q)):
        Qh, Ql = split(Q[b], q_scale[b])
        Qs = np.asarray(Q[b], np.float64) * q_scale[b]
        assert np.array_equal(Qh + Ql / 2048.0, Qs) if split_exact else np.max(np.abs(Qh + Ql / 2048.0 - Qs)) <= 2.0 ** -24
        uQh, uQl = unit_exp(Qh), unit_exp(Ql)
        assert_budget((np.abs(Qh) @ np.abs(Dh).T).max(), uQh, uDh, limit=limit)
        cu = [a + c for a, c in ((uQl, uDh), (uQh, uDl)) if a is not None and c is not None]
        assert_budget((np.abs(Ql) @ np.abs(Dh).T + np.abs(Qh) @ np.abs(Dl).T).max(), min(cu) if cu else None, limit=limit)
        main, cross = Qh @ Dh.T, Ql @ Dh.T + Qh @ Dl.T
        V = main + cross / 2048.0
        assert np.array_equal((V - main) * 2048.0, cross)  # the fp64 fold itself lost nothing
        ok, r = _f32_exact(V)
        assert ok or not fold_exact
        out[b] = _finish(r.astype(np.float64), doc_ptr, 1.0 / (q_scale[b] * d_scale), limit)
    return out


def f32_expected(D, doc_ptr, Q, one_product=False, limit=LIMIT):
    """The fp32 score matrix of the fp32-input forms: every product sum exact (one_product: a single non-zero product
    per similarity, rounded once), then as above."""
    D64 = np.asarray(D, np.float64)
    uD = unit_exp(D64)
    out = np.empty((len(Q), len(doc_ptr) - 1), np.float32)
    for b in range(len(Q)):
        Q64 = np.asarray(Q[b], np.float64)
        V = Q64 @ D64.T
        if one_product:
            assert ((Q64 != 0).astype(np.int64) @ (D64 != 0).astype(np.int64).T).max() <= 1
            with np.errstate(under="ignore"):
                V = V.astype(np.float32).astype(np.float64)
        else:
            assert_budget((np.abs(Q64) @ np.abs(D64).T).max(), unit_exp(Q64), uD, limit=limit)
            assert _f32_exact(V)[0]
        out[b] = _finish(V, doc_ptr, 1.0, limit)
    return out


# ---- expected lists and comparisons ---------------------------------------------------------------------------------------
def order_of(row):
    row = np.asarray(row, np.float32) + np.float32(0.0)
    return np.lexsort((np.arange(row.size), -row.astype(np.float64)))


def topk_expected(S, k, rows=None):
    """(scores f32 [nq, k], ids i64 [nq, k]) of a score matrix: descending, ties -> lower id, -0.0 as +0.0, -FLT_MAX / -1
    behind the hits.  rows: per query the document ids ranked (a scope); default all."""
    nq = S.shape[0]
    s = np.full((nq, k), -FLT_MAX, np.float32)
    i = np.full((nq, k), -1, np.int64)
    for b in range(nq):
        r = np.arange(S.shape[1]) if rows is None else np.asarray(rows[b], np.int64)
        v = S[b, r] + np.float32(0.0)
        o = np.lexsort((r, -v.astype(np.float64)))[:k]
        s[b, :o.size], i[b, :o.size] = v[o], r[o]
    return s, i


def same_scores(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0))))


def tie_k(S, n):
    """The first depth 2 <= k < n whose cut falls inside a tie group of query 0 (None: no tie)."""
    v = np.sort(S[0].astype(np.float64))[::-1]
    hit = np.nonzero(v[1:n - 1] == v[2:n])[0]
    return int(hit[0]) + 2 if hit.size else None


def depths(S, n):
    """The depth kinds of a store of n documents: 1, one inside a tie group, n // 4 and n // 4 + 1 (the route boundary),
    n, and one beyond n (padding) — as {kind: k}, 1 <= k <= MAX_K."""
    out = {"one": 1, "tie": tie_k(S, n), "quarter": n // 4, "quarter+1": n // 4 + 1, "all": n, "over": n + 3}
    return {name: k for name, k in out.items() if k is not None and 1 <= k <= MAX_K}


def tie_share(S, ks):
    """The share of (query, k) cuts, k < n, that fall inside a tie group."""
    n = S.shape[1]
    inside = total = 0
    for row in S:
        v = np.sort(row.astype(np.float64))[::-1]
        for k in ks:
            if 1 <= k < n:
                total += 1
                inside += int(v[k - 1] == v[k])
    return inside / max(total, 1)


# ---- builders ---------------------------------------------------------------------------------------------------------------
DOC_LENS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 220, 513)
N_EDGES = (3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 23, 24, 25)
N_SELECT = (639, 640, 641, 1279, 1280, 1281, SELECT_ROWS_MAX - 1, SELECT_ROWS_MAX, SELECT_ROWS_MAX + 1)
NQS = (1, 7, 8, 9, 16, 17, 33)
Q_LENS = (1, 15, 16, 17, 31, 32)
BAIT_REMAINDERS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)
LIVE_ROWS = (0, 15, 16, 31)
_LENS_ORDER = (513, 1, 220, 15, 65, 16, 64, 17, 63, 31, 33, 32)


def _ptr(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _ints(rng, shape):
    return rng.integers(-15, 16, size=shape).astype(np.float32)


def _int_queries(rng, nq):
    Q = _ints(rng, (nq, 32, DIM))
    Q[:, 0, 5] = np.where(np.arange(nq) % 2 == 0, 15.0, -15.0)  # the scale of every query, whatever its q_len
    return Q


@functools.lru_cache(maxsize=None)
def integers_store():
    """25 documents: every length of DOC_LENS, each followed by its twin (the same tokens, permuted), and a third 513."""
    rng = np.random.default_rng(4101)
    docs = []
    for ln in _LENS_ORDER:
        t = _ints(rng, (ln, DIM))
        if not docs:
            t[0, 3] = 15.0  # the store's scale, in every prefix
        docs += [t, t[rng.permutation(ln)]]
    docs.append(docs[0][rng.permutation(513)])
    return dict(D=np.concatenate(docs), doc_ptr=_ptr([len(t) for t in docs]), Q=_int_queries(rng, 33))


@functools.lru_cache(maxsize=None)
def short_store():
    """SELECT_ROWS_MAX + 1 documents of RA.maxsim_short_docs' length profile (1 .. 12 tokens), each a permutation of one
    of 40 base documents: ties in masses at every cut, under 14 k tokens.  Document 0 holds the scale."""
    rng = np.random.default_rng(4102)
    base = [_ints(rng, (int(ln), DIM)) for ln in rng.integers(1, 13, size=40)]
    base[0][0, 3] = 15.0
    pick = rng.integers(0, 40, size=SELECT_ROWS_MAX + 1)
    pick[:4] = [0, 1, 2, 3]
    docs = [base[p][rng.permutation(len(base[p]))] for p in pick]
    return dict(D=np.concatenate(docs), doc_ptr=_ptr([len(t) for t in docs]), Q=_int_queries(rng, 8))


@functools.lru_cache(maxsize=None)
def position_store():
    D = np.zeros((64 * 32 + 64 * 64, DIM), np.float32)
    lens = [32] * 64 + [64] * 64
    ptr = _ptr(lens)
    sign = np.where(np.arange(DIM) % 3 == 0, -1.0, 1.0).astype(np.float32)
    for d in range(128):
        row = d % 32 + (32 if d >= 96 else 0)
        D[ptr[d] + row, d] = sign[d] * (1 + (d * 37) % 128)
    Q = np.zeros((8, 32, DIM), np.float32)
    for b in range(4):
        for i in range(32):
            c = 4 * i + b
            Q[b, i, c] = sign[c]
            Q[4 + b, 31 - i, c] = 2.0 * sign[c]
    return dict(D=D, doc_ptr=ptr, Q=Q)


def position_coverage(c):
    """(components, tile rows, query rows) that alone decide a positive score of the position store."""
    comps, rows, qrows = set(), set(), set()
    ptr = c["doc_ptr"]
    for d in range(len(ptr) - 1):
        t, col = np.nonzero(c["D"][ptr[d]:ptr[d + 1]])
        for b in range(len(c["Q"])):
            i = np.nonzero(c["Q"][b][:, col[0]])[0]
            if i.size:
                comps.add(int(col[0])), rows.add(int(t[0]) % 32), qrows.add(int(i[0]))
    return comps, rows, qrows


@functools.lru_cache(maxsize=None)
def bait_store(last):
    """[negative_R, bait] for every R of BAIT_REMAINDERS, then negative_last once more, at the very end of the store."""
    rng = np.random.default_rng(4103)
    docs = []

    def negative(R, base):
        t = np.zeros((R, DIM), np.float32)
        t[:, 0] = -(base + R - 1 - np.arange(R))  # distinct, the least negative (-base) in the LAST token
        return t
    for n, R in enumerate(BAIT_REMAINDERS):
        bait = np.zeros((64, DIM), np.float32)
        bait[:, 0] = 100.0
        docs += [negative(R, n + 1), bait]
    docs.append(negative(last, BAIT_REMAINDERS.index(last) + 1))
    Q = _ints(rng, (9, 32, DIM))
    Q[:, :, 0] = rng.integers(1, 16, size=(9, 32))  # positive on the one component the store uses
    Q[:, 0, 0] = 15.0
    return dict(D=np.concatenate(docs), doc_ptr=_ptr([len(t) for t in docs]), Q=Q)


def _wide(rng, shape, low_bits=22):
    """(1024 + A) / 2048 + B / 2^low_bits, 0 < |B| < 2^(low_bits - 12), random signs: for A >= 1 hi is the first term and
    lo the second (split() emulates the rest)."""
    A = rng.integers(0, 1024, size=shape)
    half = 1 << (low_bits - 12)
    B = rng.integers(-half + 1, half, size=shape)
    B = np.where(B == 0, 1, B)
    x = (1024 + A) / 2048.0 + B / float(1 << low_bits)
    x32 = (x * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)
    assert np.array_equal(np.abs(x32).astype(np.float64), x)
    return x32


@functools.lru_cache(maxsize=None)
def wide_store(reverse=False):
    """A 22-bit side against a one-hot side +- 2^p with live rows LIVE_ROWS (two per query; reverse: the store is the
    one-hot side — documents with two live tokens at tile rows of LIVE_ROWS, the rest all-zero — and the queries carry
    four wide rows)."""
    rng = np.random.default_rng(4104 + int(reverse))
    lens = list(DOC_LENS[:10]) + [32, 32]
    ptr = _ptr(lens)
    if not reverse:
        D = _wide(rng, (int(ptr[-1]), DIM))
        Q = np.zeros((9, 32, DIM), np.float32)
        for b in range(9):
            for j in range(2):
                row = LIVE_ROWS[(b + 1 + b // 4) % 4 if j else b % 4]  # two different rows, one p per query
                Q[b, row, rng.integers(0, DIM)] = rng.choice([-1.0, 1.0]) * 2.0 ** (b % 5 - 2)
        return dict(D=D, doc_ptr=ptr, Q=Q)
    D = np.zeros((int(ptr[-1]), DIM), np.float32)
    for d, ln in enumerate(lens):
        for r in {LIVE_ROWS[d % 4] % ln, LIVE_ROWS[(d + 1 + d // 4) % 4] % ln, ln - 1}:
            D[ptr[d] + r, rng.integers(0, DIM)] = rng.choice([-1.0, 1.0]) * 0.25
    Q = np.zeros((9, 32, DIM), np.float32)
    Q[:, LIVE_ROWS, :] = _wide(rng, (9, 4, DIM))
    return dict(D=D, doc_ptr=ptr, Q=Q)


@functools.lru_cache(maxsize=None)
def both_wide_store(low_bits=22):
    """One-hot wide tokens on 8 components against one-hot wide queries of one token."""
    rng = np.random.default_rng(4105 + low_bits)
    lens = list(DOC_LENS[:10])
    ptr = _ptr(lens)
    n = int(ptr[-1])
    D = np.zeros((n, DIM), np.float32)
    D[np.arange(n), rng.integers(0, 8, size=n) * 16 + 3] = _wide(rng, n, low_bits)
    Q = np.zeros((9, 1, DIM), np.float32)
    Q[np.arange(9), 0, (np.arange(9) % 8) * 16 + 3] = _wide(rng, 9, low_bits)
    return dict(D=D, doc_ptr=ptr, Q=Q)


TP_K, TP_CLONES = 5, 100


@functools.lru_cache(maxsize=None)
def twopass_store(kind):
    """kind: 'listed' (every query has TP_K + 4 planted documents), 'overflow' (none has: the TP_CLONES clones tie at
    every cut) or 'mixed' (even queries overflow, odd ones are listed — both in every pass-1 wave).  17 queries."""
    rng = np.random.default_rng(4106)
    nq = 17
    Q = _int_queries(rng, nq)
    listed = [b for b in range(nq) if kind == "listed" or (kind == "mixed" and b % 2 == 1)]
    clone = _ints(rng, (2 * nq, DIM))
    over = [b for b in range(nq) if b not in listed]
    for j, b in enumerate(over):  # the clones hold two rows of each overflowing query: its best documents by far
        clone[2 * j: 2 * j + 2] = Q[b, 1:3]
    docs = [_ints(rng, (int(rng.integers(1, 30)), DIM)) for _ in range(30)]
    docs[0][0, 3] = 15.0
    docs += [clone[rng.permutation(2 * nq)] for _ in range(TP_CLONES)]
    for b in listed:
        for j in range(TP_K + 4):  # copies of 32 - 2 j rows of the query: |q_i|^2 ~ 10^4 per row and step
            docs.append(np.concatenate([Q[b, : 32 - 2 * j], _ints(rng, (3, DIM))]))
    order = rng.permutation(len(docs))
    order = np.concatenate([[0], order[order != 0]])
    docs = [docs[i] for i in order]
    return dict(D=np.concatenate(docs), doc_ptr=_ptr([len(t) for t in docs]), Q=Q, listed=np.array(listed, np.int64))


def twopass_status(c, k, nq=None):
    """Per query: +1 listed (its k + 4 best are more than 2 eps above the rest: at most k + 4 candidates), -1 overflowed
    (more than ms_cand_cap(k) documents tie exactly at its cut), by the fp64 model of the candidate rule; 0: neither."""
    Q = c["Q"][:nq]
    S = c["exp_split"].astype(np.float64)
    approx, eps = RA.model_maxsim_hi(Q, c["D"], c["doc_ptr"]), RA.maxsim_eps(Q, c["D"])
    out = np.zeros(len(Q), np.int64)
    for b in range(len(Q)):
        v = np.sort(S[b])[::-1]
        n_cand = len(RA.candidates(approx[b], eps[b], k))
        if v[k + 3] - v[k + 4] > 2 * eps[b] and n_cand <= k + 4:
            out[b] = 1
        elif int(np.sum(S[b] == v[k - 1])) > RA.ms_cand_cap(k) and n_cand > RA.ms_cand_cap(k):
            out[b] = -1
    return out


FAMILIES = ("integers", "short", "position", "bait", "wide", "wide_rev", "both_wide", "rounded_lo", "twopass")
_STORES = {"integers": integers_store, "short": short_store, "position": position_store, "bait": bait_store,
           "wide": wide_store, "wide_rev": lambda: wide_store(True), "both_wide": both_wide_store,
           "rounded_lo": lambda: both_wide_store(24), "twopass": twopass_store}


@functools.lru_cache(maxsize=None)
def view(family, arg=None, n_docs=None, nq=None, q_len=None, sd=0, sq=0):
    """A case: the family's store (arg: bait_store's remainder / twopass_store's kind) cut to its first n_docs documents,
    nq queries and q_len query rows, times 2^sd / 2^sq, with exp_split and exp_f32 — certificates asserted."""
    c = _STORES[family](arg) if arg is not None else _STORES[family]()
    ptr = c["doc_ptr"] if n_docs is None else c["doc_ptr"][: n_docs + 1]
    out = dict(c, D=c["D"][: int(ptr[-1])], doc_ptr=ptr, Q=np.ascontiguousarray(c["Q"][:nq, :q_len]), family=family)
    if sd or sq:
        out = RA.maxsim_scaled(out, sd, sq)
    rounded = family in ("both_wide", "rounded_lo")
    d_scale, q_scale = RA.maxsim_scales(out["Q"], out["D"])
    assert np.all(1.0 / (q_scale * d_scale) >= 2.0 ** -126) and np.all(1.0 / (q_scale * d_scale) < 2.0 ** 128)
    out["exp_split"] = split_expected(out["D"], ptr, out["Q"], fold_exact=not rounded, split_exact=family != "rounded_lo")
    out["exp_f32"] = f32_expected(out["D"], ptr, out["Q"], one_product=rounded)
    if rounded:
        assert np.any(out["exp_split"].view(np.uint32) != out["exp_f32"].view(np.uint32))  # the test tells the forms apart
    else:
        assert same_scores(out["exp_split"], out["exp_f32"])
    for m in (out["exp_split"], out["exp_f32"]):
        assert np.all(np.isfinite(m)) and np.all((m == 0) | (np.abs(m) >= 2.0 ** -126))
    return out


def expected_of(c, form):
    return c["exp_split"] if form in SPLIT_FORMS else c["exp_f32"]


# ---- non-finite stores (section 5 of the header's rule) -----------------------------------------------------------------
NONFINITE_KINDS = ("nan-token", "nan-document", "inf-zero", "inf-nonzero", "neginf-zero", "neginf-nonzero")
NF_DOC, NF_ONE = 4, 2  # a 220-token document and a one-token document among the first 9 of the integers store


def nonfinite_case(kind, nq):
    """The first 9 documents of the integers store with one bad component, q_len = 17: (case, bad document, clean store —
    the bad token replaced by zeros).  Component 9 of every query row is zero for the '-zero' kinds (inf x 0 = NaN in
    every row) and +-3 for the '-nonzero' kinds."""
    c = view("integers", None, 9, nq, 17)
    D, Q = c["D"].copy(), c["Q"].copy()
    doc = NF_ONE if kind == "nan-document" else NF_DOC
    tok = int(c["doc_ptr"][doc]) + (0 if doc == NF_ONE else 40)
    clean = D.copy()
    clean[tok] = 0.0
    if kind.startswith("nan"):
        D[tok, 9] = np.nan
    else:
        Q[:, :, 9] = 0.0 if kind.endswith("-zero") else np.where(np.arange(17) % 2 == 0, 3.0, -3.0)[None, :]
        D[tok, 9] = -np.inf if kind.startswith("neginf") else np.inf
    return dict(c, D=D, Q=Q), doc, clean


def nonfinite_expected(D, doc_ptr, Q):
    """The rule of include/amdretrieval.h for the fp32-input forms: a similarity that is NaN or -inf never wins a
    maximum, which starts at -FLT_MAX; +inf does; the maxima are summed in fp32 (-FLT_MAX absorbs finite addends, two of
    them overflow to -inf).  Never NaN."""
    out = np.empty((len(Q), len(doc_ptr) - 1), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(len(Q)):
            V = np.asarray(Q[b], np.float64) @ np.asarray(D, np.float64).T
            V = np.where(np.isnan(V), -FLT_MAX, np.maximum(V, -FLT_MAX))
            out[b] = np.maximum.reduceat(V, np.asarray(doc_ptr[:-1], np.int64), axis=1).sum(axis=0).astype(np.float32)
    assert not np.any(np.isnan(out))
    return out


# ---- wrong-kernel models ------------------------------------------------------------------------------------------------------
FAULTS = ("max0", "mask_gt", "nomask", "early16", "dropk", "qrows", "lo_trunc", "cross_al", "cross_ah", "inv1024", "tie_high",
          "cut_first")
SCORE_FAULTS = FAULTS[:10]


def _f16_trunc(v):
    """fp16 toward zero."""
    h = np.asarray(v, np.float32).astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(v)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float16)


def model_scores(D, doc_ptr, Q, fault=None):
    """The split-fp16 pair form as ms_pair_doc_h walks it — 32-token tiles that read on into the next document's tokens
    and into one zero tile behind the store, rows >= remain masked on a document's last tile — in fp64 with the fold
    rounded to fp32 once; `fault`: one of SCORE_FAULTS (None: the kernel as written)."""
    d_scale, q_scale = RA.maxsim_scales(Q, D)
    nq, q_len = Q.shape[:2]
    flat = np.concatenate([np.asarray(Q, np.float32).reshape(-1, DIM), np.zeros((32, DIM), np.float32)])

    def sp(x, s):
        hi, lo = split(x, s)
        if fault == "lo_trunc":
            v = (np.asarray(x, np.float32) * np.float32(s)).astype(np.float32)
            lo = _f16_trunc((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float64)
        return hi, lo
    Dh, Dl = (np.concatenate([a, np.zeros((32, DIM))]) for a in sp(D, d_scale))
    live = np.ones(DIM, bool)
    if fault == "dropk":
        live[40:48] = False
    out = np.empty((nq, len(doc_ptr) - 1), np.float32)
    for b in range(nq):
        rows = 32 if fault == "qrows" else q_len
        Qh, Ql = sp(flat[b * q_len: b * q_len + rows], q_scale[b])
        Qh, Ql = Qh * live, Ql * live
        un = 1.0 / (q_scale[b] * d_scale)
        for d in range(len(doc_ptr) - 1):
            t_lo, ln = int(doc_ptr[d]), int(doc_ptr[d + 1] - doc_ptr[d])
            best = np.full(rows, 0.0 if fault == "max0" else -FLT_MAX)
            for tok0 in range(0, ln, 32):
                ah, al = Dh[t_lo + tok0: t_lo + tok0 + 32], Dl[t_lo + tok0: t_lo + tok0 + 32]
                cross = (0 if fault == "cross_ah" else Ql @ ah.T) + (0 if fault == "cross_al" else Qh @ al.T)
                V = (Qh @ ah.T + cross / (1024.0 if fault == "inv1024" else 2048.0)).astype(np.float32).astype(np.float64)
                remain = ln - tok0
                keep = remain + 1 if fault == "mask_gt" else 32 if fault == "nomask" else remain
                if fault == "early16" and remain <= 17:
                    keep = min(keep, 16)
                best = np.maximum(best, V[:, :min(keep, 32)].max(axis=1))
            out[b, d] = np.float32((best * un).sum())
    return out


def model_topk(S, k, fault=None):
    """The top-k of a score matrix; fault 'tie_high': ties to the higher id; 'cut_first': the k best are cut out by score
    alone (ties at the cut fall to the higher ids) and only then ordered with the tie rule."""
    if fault is None:
        return topk_expected(S, k)
    nq, n = S.shape
    s = np.full((nq, k), -FLT_MAX, np.float32)
    i = np.full((nq, k), -1, np.int64)
    for b in range(nq):
        v = (S[b] + np.float32(0.0)).astype(np.float64)
        o = np.lexsort((-np.arange(n), -v))[:k]
        if fault == "cut_first":
            o = o[np.lexsort((o, -v[o]))]
        s[b, :o.size], i[b, :o.size] = S[b, o] + np.float32(0.0), o
    return s, i


# ---- the cases of the GPU driver and their coverage ---------------------------------------------------------------------------
def _case(name, family, arg=None, n_docs=None, nq=8, q_len=32, pins=(P_DEF, P_F32, P_ONE), ks=None, sd=0, sq=0):
    return dict(name=name, family=family, arg=arg, n_docs=n_docs, nq=nq, q_len=q_len, pins=pins, ks=ks, sd=sd, sq=sq)


def scale_pairs():
    """RA.MAXSIM_SCALE_PAIRS whose product of unscales is a normal fp32 number: it is 2^(sd + sq + c), |c| <= 8 for the
    families scaled here (view() asserts it on the data)."""
    return [(sd, sq) for sd, sq in RA.MAXSIM_SCALE_PAIRS if abs(sd + sq) <= 110]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for j, nq in enumerate(NQS):  # every batch size, the query lengths in turn, all 25 documents = every length
        out.append(_case(f"lens-nq{nq}", "integers", nq=nq, q_len=Q_LENS[j % len(Q_LENS)]))
    for j, q_len in enumerate(Q_LENS):  # every query length in a pair batch and in a block batch
        out.append(_case(f"qlen{q_len}-nq7", "integers", n_docs=24, nq=7, q_len=q_len))
        out.append(_case(f"qlen{q_len}-nq9", "integers", n_docs=24, nq=9, q_len=q_len))
    for n in N_EDGES:  # corpus sizes on and across the documents per block of every kernel
        out.append(_case(f"docs{n}-nq7", "integers", n_docs=n, nq=7, q_len=17))
        out.append(_case(f"docs{n}-nq8", "integers", n_docs=n, nq=8, q_len=32))
    for n in N_SELECT:  # the select kernel's row selectors; k <= 64 takes them, 65 the staged sweep
        out.append(_case(f"select{n}", "short", n_docs=n, nq=8, pins=(P_DEF,), ks={"one": 1, "ten": 10, "k64": 64, "k65": 65}))
    out.append(_case("position-nq7", "position", nq=7, ks={"one": 1, "live": 32, "all": 128}))
    out.append(_case("position-nq8", "position", nq=8, ks={"one": 1, "live": 32, "all": 128}))
    for R in BAIT_REMAINDERS:
        out.append(_case(f"bait{R}-nq2", "bait", arg=R, nq=2, q_len=31))
        out.append(_case(f"bait{R}-nq9", "bait", arg=R, nq=9, q_len=32))
    for fam in ("wide", "wide_rev", "both_wide", "rounded_lo"):
        q_len = 1 if fam in ("both_wide", "rounded_lo") else 32
        out.append(_case(f"{fam}-nq7", fam, nq=7, q_len=q_len))
        out.append(_case(f"{fam}-nq9", fam, nq=9, q_len=q_len))
    for sd, sq in scale_pairs():
        if (sd, sq) != (0, 0):
            out.append(_case(f"scaled-int-{sd}-{sq}-nq7", "integers", n_docs=9, nq=7, q_len=17, sd=sd, sq=sq))
            out.append(_case(f"scaled-int-{sd}-{sq}-nq8", "integers", n_docs=9, nq=8, q_len=32, sd=sd, sq=sq))
            out.append(_case(f"scaled-wide-{sd}-{sq}-nq9", "wide", nq=9, sd=sd, sq=sq))
    for kind in ("listed", "overflow", "mixed"):
        for nq in (16, 17):
            out.append(_case(f"twopass-{kind}-nq{nq}", "twopass", arg=kind, nq=nq, pins=(P_DEF, P_ONE), ks={"tp": TP_K, "one": 1}))
    return tuple(out)


def case_view(case):
    return view(case["family"], case["arg"], case["n_docs"], case["nq"], case["q_len"], case["sd"], case["sq"])


def case_depths(case, c):
    return case["ks"] if case["ks"] is not None else depths(c["exp_split"], len(c["doc_ptr"]) - 1)


SCOPE_CASES = tuple(("integers", None, 25, nq, Q_LENS[j % len(Q_LENS)]) for j, nq in enumerate(NQS)) + (
    ("bait", 17, None, 2, 31), ("bait", 33, None, 9, 32), ("bait", 64, None, 9, 32), ("position", None, None, 8, 32),
    ("wide", None, None, 7, 32), ("wide_rev", None, None, 7, 32))


def scopes_of(n_docs):
    """Scopes of one document (the first, one inside, the last), a run, and every document."""
    return [np.arange(n_docs), np.array([0]), np.array([n_docs // 2]), np.array([n_docs - 1]),
            np.arange(n_docs // 3, min(n_docs, n_docs // 3 + 9))]


def coverage_table():
    """{form: {axis: set of values}} over cases(): document lengths, corpus sizes, batch sizes, query lengths and depth
    kinds that reach each form, by form_of (the scoped form: SCOPE_CASES)."""
    tab = {f: {"len": set(), "n_docs": set(), "nq": set(), "q_len": set(), "k": set(), "docs7": {False, True}} for f in FORMS}
    for case in cases():
        c = case_view(case)
        n = len(c["doc_ptr"]) - 1
        lens = set(np.diff(c["doc_ptr"]).tolist())
        for pins in case["pins"]:
            seen = {(form_of(n, case["nq"], 1, False, pins), None)}
            seen |= {(form_of(n, case["nq"], k, True, pins), kind) for kind, k in case_depths(case, c).items()}
            for form, kind in seen:
                t = tab[form]
                t["len"] |= lens
                t["n_docs"].add(n), t["nq"].add(case["nq"]), t["q_len"].add(case["q_len"])
                if kind:
                    t["k"].add(kind)
    for family, arg, n_docs, nq, q_len in SCOPE_CASES:
        c = view(family, arg, n_docs, nq, q_len)
        t = tab[SCOPED]
        t["len"] |= set(np.diff(c["doc_ptr"]).tolist())
        t["n_docs"].add(len(c["doc_ptr"]) - 1), t["nq"].add(nq), t["q_len"].add(q_len)
        t["k"] |= {"one", "tie", "all", "over"}
    return tab


def admitted(form):
    """The listed edges a form admits: the pair forms take batches below K_MSQ, the block forms from it on; the two-pass
    route needs 4 k <= n_docs (so n_docs >= 4 and no depth beyond n_docs // 4) and alone has the select kernel's corpus
    sizes; the scoped form ranks a scope, not a corpus: its depths are 1, a tie, the scope and beyond it."""
    pair = form in (PAIRF32, PAIRHALF)
    a = {"len": set(DOC_LENS), "q_len": set(Q_LENS),
         "nq": {q for q in NQS if (q < K_MSQ) == pair},
         "n_docs": set(N_EDGES), "k": {"one", "tie", "quarter", "quarter+1", "all", "over"}}
    if form == TWOPASS:
        a["n_docs"] = {n for n in N_EDGES if n >= 4} | set(N_SELECT)
        a["k"] = {"one", "tie", "quarter", "k64", "k65"}
    if form == RING:
        a["k"] = {"one", "tie", "quarter", "quarter+1", "all", "over"}  # (one .. quarter: pinned to one pass)
    if form == SCOPED:
        a["nq"], a["n_docs"], a["k"] = set(NQS), {25}, {"one", "tie", "all", "over"}  # (the scope is cut into slabs: AMDR_SCOPE_SLAB)
    return a

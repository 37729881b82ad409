"""Resident stores past the three address marks of `base + row * width` (tests/test_store_limit*.py).

The marks, for a store of 4-byte elements:
  byte offset 2^32    a 32-bit byte offset or buffer range wraps       element 2^30
  element    2^31    a signed int element index wraps
  element    2^32    an unsigned element index wraps
A zero-filled or periodic store hides such a wrap — the wrapped address holds the same data — so every store here is a
CLOSED FORM of its (row, column): f for the dense matrix, g for the ColBERT token rows, hash-like integer functions
computed modulo 2^32 in int64.  Any row can be produced anywhere (numpy on the host, torch on the device, whole chunks or
single rows) without holding the store, and the wrong-address certificates below evaluate, by formula only, what a kernel
with one of four address faults would read in place of each checked row.

Dense: d = 768, so every mark falls INSIDE a row; n = 5 596 619 rows (17.2 GB; n = 11 mod 32).  Values in {-3 .. 3} and
queries in {-3 .. 3}: max|Q| sum|x| <= 6 912 < 2^24, every fp32 score is an exact integer in any order.  Planted rows
3 sign(Q[j]) (the row's own background in the query's zero columns) around every mark: all planted rows of one query tie
exactly, on both sides of every mark, so the lower id must win across the marks.

ColBERT: 128 columns, T = 2^24 + 3 001 tokens (8.6 GB: D and img past byte 2^32 and element 2^31, img_hi past byte 2^32),
document lengths 1 .. 220 from a seeded generator with one document straddling token 2^23 and one straddling 2^24.
Values in {-7 .. 7} on both sides: every similarity and every sum is an integer below 2^24, fp16 holds every scaled
component, the lo halves are zero.

The references never call the library: torch fp64 GEMMs in row / token chunks on the device (exact on these integers),
numpy fp64 on rows produced by the formula for the row-addressed calls."""
from __future__ import annotations

import functools

import numpy as np

import dense_adversary as DA
import maxsim_adversary as MS

M32 = (1 << 32) - 1

# ---- shapes and marks ---------------------------------------------------------------------------------------------------
D_DENSE = 768
N_DENSE = 5_596_619
N_OWNED = 2_796_203 + 4_213
DIM_MS = 128
T_MS = (1 << 24) + 3001
MS_MAXLEN = 220
VAL_DENSE, VAL_MS = 3, 7


class Marks:
    """The marks of a store of `width` elements of `elem` bytes per row: {name: element index}."""

    def __init__(self, width, elem=4, byte_mark=1 << 32, int_mark=1 << 31, uint_mark=1 << 32):
        self.width, self.elem = int(width), int(elem)
        self.elements = {"byte2^32": byte_mark // elem, "elem2^31": int_mark, "elem2^32": uint_mark}
        self.byte_mark, self.int_mark, self.uint_mark = byte_mark, int_mark, uint_mark

    def row(self, name):
        """The row that holds the mark (the mark need not be at its start)."""
        return self.elements[name] // self.width

    def rows(self, n):
        """{name: row} of the marks that lie inside an n-row store."""
        return {m: self.row(m) for m in self.elements if self.row(m) < n}


DENSE_MARKS = Marks(D_DENSE)
MS_MARKS = Marks(DIM_MS)
assert DENSE_MARKS.rows(N_DENSE) == {"byte2^32": 1_398_101, "elem2^31": 2_796_202, "elem2^32": 5_592_405}
assert all(DENSE_MARKS.elements[m] % D_DENSE for m in DENSE_MARKS.elements)  # every mark inside a row
assert N_DENSE % 32 == 11
assert set(DENSE_MARKS.rows(N_OWNED)) == {"byte2^32", "elem2^31"} and N_OWNED - 1 > DENSE_MARKS.row("elem2^31")
# the ColBERT store: token 2^23 is the byte mark of D (128 x 4 B) and 2^24 its 2^31-element mark; the fp16 images
# (img: hi and lo, img_hi: hi only, 2 B elements) reach byte 2^32 at token 2^24
assert MS_MARKS.rows(T_MS) == {"byte2^32": 1 << 23, "elem2^31": 1 << 24}

# ---- the closed forms -----------------------------------------------------------------------------------------------------
_A, _B, _M1, _M2 = 0x9E3779B1, 0x85EBCA77, 0x7FEB352D, 0x446B2D2B  # odd; the multipliers of a hashed value stay below 2^31
SALT_F, SALT_G = 0x1234567, 0x7654321


def _hash_np(r, c, salt):
    """Modulo 2^32, carried in int64: r < 2^31 (r A < 2^63), c < 2^16, every product of a 32-bit value below 2^63."""
    h = (np.asarray(r, np.int64) * _A + np.asarray(c, np.int64) * _B + salt) & M32
    h = h ^ (h >> 15)
    h = (h * _M1) & M32
    h = h ^ (h >> 13)
    h = (h * _M2) & M32
    return h ^ (h >> 16)


def f_np(rows, cols=None):
    """Background dense rows [len(rows), 768] (or the given columns) as int64 in {-3 .. 3}."""
    rows = np.asarray(rows, np.int64).reshape(-1)
    cols = np.arange(D_DENSE, dtype=np.int64) if cols is None else np.asarray(cols, np.int64)
    return _hash_np(rows[:, None], cols[None, :], SALT_F) % (2 * VAL_DENSE + 1) - VAL_DENSE


def g_np(tokens):
    """ColBERT token rows [len(tokens), 128] as int64 in {-7 .. 7}."""
    tokens = np.asarray(tokens, np.int64).reshape(-1)
    return _hash_np(tokens[:, None], np.arange(DIM_MS, dtype=np.int64)[None, :], SALT_G) % (2 * VAL_MS + 1) - VAL_MS


def _hash_torch(torch, r, width, salt):
    """The same function written for torch: r an int64 tensor of rows on any device -> [len(r), width] int64, in place."""
    c = torch.arange(width, dtype=torch.int64, device=r.device)
    h = r.reshape(-1, 1).mul(_A).add(c.mul(_B).add_(salt).reshape(1, -1))
    h.bitwise_and_(M32)
    h.bitwise_xor_(h.bitwise_right_shift(15))
    h.mul_(_M1).bitwise_and_(M32)
    h.bitwise_xor_(h.bitwise_right_shift(13))
    h.mul_(_M2).bitwise_and_(M32)
    h.bitwise_xor_(h.bitwise_right_shift(16))
    return h


def f_torch(torch, rows):
    return _hash_torch(torch, rows, D_DENSE, SALT_F).remainder_(2 * VAL_DENSE + 1).sub_(VAL_DENSE)


def g_torch(torch, tokens):
    return _hash_torch(torch, tokens, DIM_MS, SALT_G).remainder_(2 * VAL_MS + 1).sub_(VAL_MS)


# ---- the dense case -------------------------------------------------------------------------------------------------------
NQ_ALL = 161
PLANT_QUERIES = (0, 1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 95, 96, 97, 159, 160)


@functools.lru_cache(maxsize=None)
def dense_queries():
    Q = np.random.default_rng(20_001).integers(-VAL_DENSE, VAL_DENSE + 1, size=(NQ_ALL, D_DENSE)).astype(np.float32)
    Q.setflags(write=False)
    return Q


def plant_offsets(j):
    """Offsets from a mark's row at which query PLANT_QUERIES[j] has planted rows: query 0 the mark's own row and both
    neighbours, query 1 the rows 33 away, the others a pair of their own."""
    return (-1, 0, 1) if j == 0 else (-33, 33) if j == 1 else (-(j + 1), j + 1)


@functools.lru_cache(maxsize=None)
def dense_plants(n=N_DENSE, marks=DENSE_MARKS):
    """{row: query} of the planted rows of an n-row store: around every mark inside it, plus row n - 1 (query 0) and
    row 0 (query 1)."""
    out = {}
    for m, row in marks.rows(n).items():
        for j, q in enumerate(PLANT_QUERIES):
            for o in plant_offsets(j):
                assert 0 < row + o < n - 1 and row + o not in out
                out[row + o] = q
    out[n - 1], out[0] = 0, 1
    return out


def plant_row(q, row):
    """The planted row of query q at `row`: 3 sign(Q[q]) where the query is non-zero — the largest score any row can have,
    3 sum|Q[q]| — and the background f(row, c) in the query's zero columns, so that no two planted rows are equal (the
    rows 2^32 elements = 4 194 304 rows apart would otherwise be: 3 x 2^30 is a multiple of 768)."""
    q_row = dense_queries()[q].astype(np.float64)
    return np.where(q_row != 0, 3.0 * np.sign(q_row), f_np([row])[0].astype(np.float64))


def dense_rows_np(rows, plants=None):
    """Rows of the planted dense store [len(rows), 768] fp64 (plants: dense_plants() by default)."""
    plants = dense_plants() if plants is None else plants
    rows = np.asarray(rows, np.int64).reshape(-1)
    X = f_np(rows).astype(np.float64)
    for i, r in enumerate(rows.tolist()):
        if r in plants:
            X[i] = plant_row(plants[r], r)
    return X


def dense_flat_np(elems, n=N_DENSE, plants=None):
    """The planted store at flat element indices (each inside the store)."""
    plants = dense_plants(n) if plants is None else plants
    elems = np.asarray(elems, np.int64)
    assert np.all((elems >= 0) & (elems < n * D_DENSE))
    r, c = elems // D_DENSE, elems % D_DENSE
    out = (_hash_np(r, c, SALT_F) % (2 * VAL_DENSE + 1) - VAL_DENSE).astype(np.float64)
    for row, q in plants.items():
        hit = r == row
        if hit.any():
            out[hit] = plant_row(q, row)[c[hit]]
    return out


def fill_dense_torch(torch, X, row0=0, chunk=1 << 18, plants=None, n_total=None):
    """X[i] = row row0 + i of the planted store, on X's device, in chunks."""
    n = X.shape[0]
    plants = dense_plants(n_total if n_total is not None else n) if plants is None else plants
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        X[s:e] = f_torch(torch, torch.arange(row0 + s, row0 + e, dtype=torch.int64, device=X.device)).to(X.dtype)
    rows = np.array(sorted(r for r in plants if row0 <= r < row0 + n), np.int64)
    if rows.size:
        P = np.stack([plant_row(plants[int(r)], int(r)) for r in rows]).astype(np.float32)
        X[torch.from_numpy(rows - row0).to(X.device)] = torch.from_numpy(P).to(X.device).to(X.dtype)


ID_BITS = 23  # ids below 2^23 ride in the low bits of an int64 key behind the integer score
assert N_DENSE < 1 << ID_BITS


def chunked_topk_torch(torch, rows_of, n, Q, k, chunk=1 << 18):
    """Top k of an n-row store by (score descending, id ascending), fp64 GEMM per row chunk: rows_of(lo, hi) -> the rows
    [hi - lo, d] as a tensor on the device.  Scores are integers (asserted), so (score, -id) packs exactly into one int64
    key.  -> (scores f32 [nq, k], ids i64 [nq, k]) as numpy."""
    dev = Q.device
    Qd = Q.double().t().contiguous()
    lim = (1 << ID_BITS) - 1
    best = None
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        S = (rows_of(lo, hi).double() @ Qd).t().contiguous()  # [nq, rows]
        Si = S.long()
        assert bool((Si.double() == S).all()) and int(Si.abs().max()) < DA.LIMIT
        key = Si * (1 << ID_BITS) + (lim - torch.arange(lo, hi, dtype=torch.int64, device=dev))[None, :]
        top = torch.topk(key, min(k, hi - lo), dim=1).values
        best = top if best is None else torch.topk(torch.cat([best, top], dim=1), min(k, best.shape[1] + top.shape[1]), dim=1).values
    best = torch.sort(best, dim=1, descending=True).values.cpu().numpy()
    ids = lim - (best & lim)
    scores = (best >> ID_BITS).astype(np.float32)
    out_s = np.full((Q.shape[0], k), -DA.FLT_MAX, np.float32)
    out_i = np.full((Q.shape[0], k), -1, np.int64)
    out_s[:, :best.shape[1]], out_i[:, :best.shape[1]] = scores, ids
    return out_s, out_i


# ---- certificates (formula only) ------------------------------------------------------------------------------------------
def sides_certificate(plants, marks, n):
    """For every mark inside the store some query has planted rows strictly before AND strictly behind the row that
    holds it.  -> {mark: [such queries]}"""
    out = {}
    for m, row in marks.rows(n).items():
        qs = sorted({q for r, q in plants.items() if 0 < row - r <= 64} & {q for r, q in plants.items() if 0 < r - row <= 64})
        assert qs, (m, "no query has planted rows on both sides")
        out[m] = qs
    return out


FAULT_MODELS = ("byte offset mod 2^32", "element index through int32", "element index through uint32",
                "row x width in 32 bits")
OUTSIDE = -1


def wrapped_elements(model, row, marks):
    """The flat element indices a kernel with the address fault `model` reads in place of row `row` (width elements;
    OUTSIDE where the wrapped index is negative: before the store)."""
    w = marks.width
    e = row * w + np.arange(w, dtype=np.int64)
    if model == FAULT_MODELS[0]:
        return (e * marks.elem % marks.byte_mark) // marks.elem
    if model == FAULT_MODELS[1]:
        v = (e + marks.int_mark) % (2 * marks.int_mark) - marks.int_mark
        return np.where(v < 0, OUTSIDE, v)
    if model == FAULT_MODELS[2]:
        return e % marks.uint_mark
    if model == FAULT_MODELS[3]:
        return (row * w) % marks.uint_mark + np.arange(w, dtype=np.int64)
    raise KeyError(model)


def wrong_address_certificate(model, rows, marks, flat_of, unit=4):
    """For every row of `rows` that the fault moves: what it reads (flat_of: flat elements -> values) differs from the
    right row in at least one 16-byte unit (`unit` elements), or lies before the store.  -> (rows the fault moves, rows
    that land before the store, the smallest number of differing units)."""
    w = marks.width
    moved, outside, least = [], [], w // unit
    for row in rows:
        right = row * w + np.arange(w, dtype=np.int64)
        got = wrapped_elements(model, row, marks)
        if np.array_equal(got, right):
            continue
        moved.append(row)
        if np.any(got == OUTSIDE):  # (nothing of the store lies there: no data of it can stand in for the row)
            outside.append(row)
            continue
        differs = (flat_of(got) != flat_of(right)).reshape(-1, unit).any(axis=1)
        assert differs.any(), (model, row, "the wrapped address holds the same data")
        least = min(least, int(differs.sum()))
    return moved, outside, least


def rows_past(marks, n):
    """Per model, the first row the fault moves in an n-row store (None: the store does not reach the fault)."""
    first = {FAULT_MODELS[0]: marks.row("byte2^32"), FAULT_MODELS[1]: marks.row("elem2^31"),
             FAULT_MODELS[2]: marks.row("elem2^32"), FAULT_MODELS[3]: -(-marks.uint_mark // marks.width)}
    return {m: (r if r < n else None) for m, r in first.items()}


def mark_window_rows(n, marks, reach=33):
    """The rows at, before and behind every mark inside the store (offsets 0, +-1, +-2, +-reach), row 0 and row n - 1."""
    out = {0, n - 1}
    for row in marks.rows(n).values():
        out |= {row + o for o in (-reach, -2, -1, 0, 1, 2, reach) if 0 <= row + o < n}
    return np.array(sorted(out), np.int64)


# ---- updates of the owned dense index: a model of where every row comes from --------------------------------------------
class RowSource:
    """The owned index as a list of sources: src[i] >= 0: row src[i] of f; src[i] < 0: extra row -1 - src[i]."""

    def __init__(self, n):
        self.src = np.arange(n, dtype=np.int64)
        self.extra = []

    @property
    def n(self):
        return self.src.size

    def rows(self, ids):
        s = self.src[np.asarray(ids, np.int64)]
        X = f_np(np.where(s >= 0, s, 0)).astype(np.float64)
        for i in np.nonzero(s < 0)[0]:
            X[i] = self.extra[-1 - int(s[i])]
        return X

    def remove(self, ids):
        """-> new id -> old id of the survivors (the rule: survivors keep their order)."""
        ids = np.asarray(ids, np.int64)
        new = np.arange(self.n - ids.size, dtype=np.int64)
        old = new + np.searchsorted(ids - np.arange(ids.size), new, side="right")
        self.src = self.src[old]
        return old

    def replace(self, ids, src=None, extra=None):
        """Row ids[i] becomes row src[i] of f, or the given extra vector."""
        for i, r in enumerate(np.asarray(ids, np.int64).tolist()):
            if extra is not None and extra[i] is not None:
                self.extra.append(np.asarray(extra[i], np.float64))
                self.src[r] = -len(self.extra)
            else:
                self.src[r] = src[i]

    def add(self, src):
        self.src = np.concatenate([self.src, np.asarray(src, np.int64)])


def sample_ids(n, positions, step=257, half=64):
    """About n / step + 128 per position row ids: every step-th, a window of 2 half around each position, the first and
    the last row."""
    parts = [np.arange(0, n, step), [0, n - 1]]
    for p in positions:
        parts.append(np.arange(max(0, p - half), min(n, p + half)))
    return np.unique(np.concatenate(parts).astype(np.int64))


def probe_queries(d=D_DENSE):
    """Unit vectors on the first, a middle and the last 16-byte unit of a row, and an all-ones query: [13, d]."""
    cols = [0, 1, 2, 3, d // 2, d // 2 + 1, d // 2 + 2, d // 2 + 3, d - 4, d - 3, d - 2, d - 1]
    Q = np.zeros((len(cols) + 1, d), np.float32)
    Q[np.arange(len(cols)), cols] = 1.0
    Q[-1] = 1.0
    return Q


# ---- the ColBERT case -------------------------------------------------------------------------------------------------------
MS_NQ, MS_QLEN = 8, 32


@functools.lru_cache(maxsize=None)
def ms_doc_ptr(T=T_MS, straddle=(1 << 23, 1 << 24), maxlen=MS_MAXLEN, seed=20_002):
    """Document lengths 1 .. maxlen from a seeded generator, cut to T tokens; a boundary that falls on a straddle token is
    moved one token on, so that one document holds tokens s - 1 and s for each s."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, maxlen + 1, size=2 * T // maxlen + 64)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert ptr[-1] > T
    ptr = ptr[: int(np.searchsorted(ptr, T, side="left")) + 1].copy()
    ptr[-1] = T
    for s in straddle:
        i = int(np.searchsorted(ptr, s))
        if ptr[i] == s:
            ptr[i] += 1
    lens = np.diff(ptr)
    assert np.all((lens >= 1) & (lens <= maxlen + 1)) and ptr[0] == 0 and ptr[-1] == T
    for s in straddle:
        d = ms_doc_of(ptr, s)
        assert ptr[d] < s < ptr[d + 1], (s, "no document straddles it")
    ptr.setflags(write=False)
    return ptr


def ms_doc_of(ptr, token):
    return int(np.searchsorted(ptr, token, side="right")) - 1


@functools.lru_cache(maxsize=None)
def ms_queries():
    Q = np.random.default_rng(20_003).integers(-VAL_MS, VAL_MS + 1, size=(MS_NQ, MS_QLEN, DIM_MS)).astype(np.float32)
    Q[:, 0, 5] = np.where(np.arange(MS_NQ) % 2 == 0, VAL_MS, -VAL_MS)  # the scale of every query
    Q.setflags(write=False)
    return Q


def ms_range_certificate(q_len=MS_QLEN):
    """The exact-representability conditions of maxsim_adversary on the VALUE RANGE of g and the queries: a worst-case
    store — one token of every magnitude, all of one sign, and tokens of +-7 throughout — against worst-case queries
    passes split_expected / f32_expected (the split is exact, lo is zero, every accumulator and the sum over the query
    rows stay below 2^24 units), and both forms give the same numbers.  Any store with values in the range has
    term sums no larger."""
    mags = np.arange(VAL_MS + 1, dtype=np.float32)
    D = np.concatenate([np.tile(mags[:, None], (1, DIM_MS)), -np.tile(mags[:, None], (1, DIM_MS)),
                        np.where(np.arange(DIM_MS) % 2 == 0, VAL_MS, -VAL_MS)[None, :].astype(np.float32)])
    ptr = np.arange(D.shape[0] + 1, dtype=np.int64)
    Q = np.stack([np.full((q_len, DIM_MS), VAL_MS, np.float32), np.full((q_len, DIM_MS), -VAL_MS, np.float32),
                  np.tile(np.where(np.arange(DIM_MS) % 2 == 0, VAL_MS, -VAL_MS).astype(np.float32), (q_len, 1))])
    a, b = MS.split_expected(D, ptr, Q), MS.f32_expected(D, ptr, Q)
    assert MS.same_scores(a, b)
    hi, lo = MS.split(D, 1.0 / 8.0)
    assert np.array_equal(hi * 8.0, D) and not lo.any()
    worst = float(np.abs(a).max())
    assert worst == q_len * DIM_MS * VAL_MS * VAL_MS < MS.LIMIT
    return worst


def ms_scores_np(tokens_of_doc, Q):
    """numpy fp64 MaxSim of a few documents: tokens_of_doc a list of token-id arrays -> [nq, n]."""
    out = np.empty((len(Q), len(tokens_of_doc)), np.float64)
    Qd = np.asarray(Q, np.float64)
    for j, t in enumerate(tokens_of_doc):
        V = Qd @ g_np(t).astype(np.float64).T  # [nq, q_len, tokens]
        out[:, j] = V.max(axis=2).sum(axis=1)
    return out


def ms_scores_torch(torch, tokens, seg, n_docs, Q, chunk=1 << 20):
    """torch fp64 MaxSim: tokens(lo, hi) -> token rows [hi - lo, 128] on the device for the token POSITIONS lo .. hi - 1,
    seg an int64 device tensor of each position's document (ascending), n_docs documents -> [nq, n_docs] fp64 on the
    device: a segment maximum per document and query row, summed over the query rows."""
    nq, q_len, dim = Q.shape
    Qf = Q.reshape(nq * q_len, dim).double().t().contiguous()
    M = torch.full((n_docs, nq * q_len), -float("inf"), dtype=torch.float64, device=Q.device)
    T = seg.shape[0]
    for lo in range(0, T, chunk):
        hi = min(T, lo + chunk)
        V = tokens(lo, hi).double() @ Qf
        M.index_reduce_(0, seg[lo:hi], V, "amax", include_self=True)
    return M.reshape(n_docs, nq, q_len).sum(dim=2).t().contiguous()


class DocSource:
    """The ColBERT store as a list of documents, each a run of g's tokens: start[d], length[d]."""

    def __init__(self, ptr):
        self.start = np.asarray(ptr[:-1], np.int64).copy()
        self.length = np.diff(ptr).astype(np.int64)

    @property
    def n(self):
        return self.start.size

    def ptr(self):
        return np.concatenate([[0], np.cumsum(self.length)]).astype(np.int64)

    def tokens(self, d):
        return self.start[d] + np.arange(self.length[d], dtype=np.int64)

    def all_tokens(self):
        """Source token of every position of the store, and the document of every position."""
        seg = np.repeat(np.arange(self.n, dtype=np.int64), self.length)
        p = self.ptr()
        return self.start[seg] + (np.arange(p[-1], dtype=np.int64) - p[seg]), seg

    def remove(self, ids):
        keep = np.ones(self.n, bool)
        keep[np.asarray(ids, np.int64)] = False
        self.start, self.length = self.start[keep], self.length[keep]

    def replace(self, ids, start, length):
        self.start[np.asarray(ids, np.int64)] = start
        self.length[np.asarray(ids, np.int64)] = length

    def add(self, start, length):
        self.start = np.concatenate([self.start, np.asarray(start, np.int64)])
        self.length = np.concatenate([self.length, np.asarray(length, np.int64)])


def ms_flat_np(elems):
    elems = np.asarray(elems, np.int64)
    return _hash_np(elems // DIM_MS, elems % DIM_MS, SALT_G) % (2 * VAL_MS + 1) - VAL_MS

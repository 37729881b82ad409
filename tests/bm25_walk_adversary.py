"""Hand-built indexes for the SCORING half of the BM25 channel: bm25_block_query (csrc/bm25_core.hpp) and its scoped twin
scope_bm25_piece (csrc/scope.hip).  Not a test module: tests/test_bm25_walk_adversary.py proves on the CPU that the data
is what it claims and that plausible wrong kernels would fail on it, tests/test_bm25_walk_adversary_gpu.py runs it.

The walk resolves a query's tokens 32 at a time (kBmTok), keeps those with postings in the slab (ballot + popcount), and
reads the kept lists as ONE sequence of 64-posting chunks, eight of them (kAhead) requested across token boundaries
before the first is applied.  A slab's range inside a list comes from two binary searches with shortcuts at lo == 0 and
hi >= n_docs; a slab no token touches skips scoring and ranking.  Every family below sits on one of those edges:

  W1  posting-list length: 1 ... 1025 around one chunk (64), one prefetch window (512) and nine chunks (576)
  W2  token boundaries at every position of the prefetch window, documents hit in neighbouring chunks, repeats
  W3  token groups: 0 ... 97 tokens, four kinds of unkept token, groups without a kept token
  W4  slab borders: postings at lo - 1, lo, hi - 1, hi; slabs no token touches; a slab of fewer than k documents
  W5  sums that cancel to zero

Values that make the order visible: idf is free (amdr_bm25_create takes any finite value), so it is spread over
2^-30 ... 2^40 with both signs, near-cancelling pairs (a, -a + tiny) and random 52-bit mantissas; post_tf and doc_len
vary, so the per-posting factor is an arbitrary fp64 number and fma(idf, w, s) != s + idf * w.  W5 alone keeps the
factor-1.0 construction of bm25_image_adversary (tf = 1, doc_len == avgdl): it needs exact cancellation.

About -0.0: the accumulator starts at +0.0 and IEEE round-to-nearest gives x + y = -0.0 only for x = y = -0.0, so NO
sequence of contributions leaves a raw score at -0.0: a - a is +0.0, and 0.0 + (-0.0) — a product of an idf of -0.0 —
is +0.0 too.  W5 holds both (exact cancellation, and terms whose every product is -0.0); the full-matrix comparison of
get_scores then pins the sign of every zero to +.  The wrong model "negative-zero-last" is therefore the pair of mistakes
that can make the sign visible at all: the first contribution STORED instead of added to +0.0, and -0.0 ranked below +0.0.

Expected values come from ref_scores / ref_topk of bm25_image_adversary (plain numpy fp64) and from nothing else;
model_scores restates the walk slab by slab only to show that a wrong order, a dropped token or a border off by one
changes the top k of the cases built to catch it."""
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from bm25_image_adversary import bm_plan, make_csr, nvt_bucket, plan_text, posting_factor, ref_scores, ref_topk  # noqa: F401

KTOK, CHUNK, AHEAD = 32, 64, 8  # kBmTok, postings per chunk, kAhead of bm25_block_query
DEPTHS = (1, 10, 16, 17, 64, 65, 96, 97, 256)
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 575, 576, 577, 1023, 1024, 1025)
TOKEN_COUNTS = (0, 1, 31, 32, 33, 63, 64, 65, 96, 97)
FAMILIES = ("W1", "W2", "W3", "W4", "W5")
MODELS = ("term-order", "fold-repeats", "fma", "pairwise", "drop-33rd", "stop-at-empty-group", "hi-counted", "lo-left-out",
          "negative-zero-last")
BORDER_MODELS = ("hi-counted", "lo-left-out")
SLAB_MODELS = BORDER_MODELS + ("stop-at-empty-group",)  # the models whose result depends on where the slabs are cut
LIMIT = 2.0 ** 100  # no partial sum gets near the -inf the arg-max rounds use as "no document"

W1_N, W2_N, W3_N, W5_N = 1100, 1024, (300, 1100, 2100), (300, 700, 2100)  # 300: the arg-max rounds rank k = 65 and 96 there
W4_N = (90, 2049, 4097, 4100)  # 90: one slab, not a multiple of 16, fewer documents than the depths 96, 97 and 256


@dataclass
class Case:
    family: str
    name: str
    n: int
    k: int
    csr: dict
    queries: list
    edge: str            # the edge the case sits on, in words
    reached: object      # predicate: reached(case) evaluates the edge on the arrays and returns what it found (or asserts)
    catches: tuple       # the wrong models this case is built to catch at its depth
    group: str = ""      # cases of one group share csr and queries and differ in k


# ---- values ------------------------------------------------------------------------------------------------------------
def _val(rng, e, sign=1):
    """sign * 1.m * 2^e with a random 52-bit mantissa."""
    return sign * math.ldexp(1.0 + int(rng.integers(0, 1 << 52)) / float(1 << 52), int(e))


def _spread(rng, count, lo=-30, hi=40):
    """`count` idf values: exponents spread evenly over [lo, hi] in random order, both signs, random mantissas."""
    es = np.round(np.linspace(lo, hi, count)).astype(int)
    rng.shuffle(es)
    return [_val(rng, e, 1 if rng.random() < 0.6 else -1) for e in es]


def _near_cancel(rng, e):
    """(a, -a + tiny): tiny is 2^-40 of a."""
    a = _val(rng, e)
    return a, -a + math.ldexp(a, -40)


def _vary(csr, rng):
    """Term frequencies 1-6 and document lengths 3-40 around an avgdl that is no round number: every per-posting factor
    is its own fp64 value."""
    n = csr["doc_len"].shape[0]
    csr["post_tf"] = rng.integers(1, 7, size=csr["post_doc"].shape[0]).astype(np.int32)
    csr["doc_len"] = rng.integers(3, 41, size=n).astype(np.int32)
    csr["avgdl"] = float(csr["doc_len"].sum()) / n
    return csr


def slabs_of(n, k):
    """[(lo, hi)] of the slabs bm_plan cuts n documents into at depth k."""
    slab, nslabs, _ = bm_plan(n, k)
    return [(s * slab, min((s + 1) * slab, n)) for s in range(nslabs)]


def borders_of(n, depths=DEPTHS):
    """Every slab border (the hi of one slab, the lo of the next) of every plan the depths take."""
    return sorted({lo for k in depths for lo, _ in slabs_of(n, k) if lo > 0})


def term_range(csr, t, lo, hi):
    """[a, b) of term t's postings inside documents [lo, hi); (0, 0) for an id outside the table."""
    if not 0 <= t < csr["idf"].shape[0]:
        return 0, 0
    p0, p1 = int(csr["term_ptr"][t]), int(csr["term_ptr"][t + 1])
    docs = csr["post_doc"][p0:p1]
    return p0 + int(np.searchsorted(docs, lo, "left")), p0 + int(np.searchsorted(docs, hi, "left"))


def kept_mask(csr, q, lo, hi):
    """Per token of q: has it a posting in [lo, hi)?  (what the ballot of a group sees)"""
    return [b > a for a, b in (term_range(csr, t, lo, hi) for t in q)]


def chunks(length):
    return (length + CHUNK - 1) // CHUNK


def boundary_positions(csr, q, lo, hi):
    """Positions inside the prefetch window (0 = exactly on a window's end) at which the kept tokens of each group end.
    The chunk sequence starts anew with every group of 32 tokens."""
    out = []
    for g in range(0, len(q), KTOK):
        at = 0
        for t in q[g:g + KTOK]:
            a, b = term_range(csr, t, lo, hi)
            if b > a:
                at += chunks(b - a)
                out.append(at % AHEAD)
    return out


# ---- the walk, restated with one mistake at a time ---------------------------------------------------------------------
_W = {}


def _factor(csr):
    key = id(csr)
    if key not in _W:
        _W[key] = (csr, posting_factor(csr))
    return _W[key][1]


def _fma(s, x, y):
    """fma(x, y, s): the exact product added exactly, one rounding."""
    return float(Fraction(float(s)) + Fraction(float(x)) * Fraction(float(y)))


def model_scores(csr, q, slabs, model=None):
    """fp64 scores [n] of query q (raw, not yet folded), walked slab by slab as bm25_block_query does, with ONE mistake:
      term-order           kept tokens applied in ascending term-id order
      fold-repeats         a repeated token applied once, as (count * idf) * w
      fma                  s = fma(idf, w, s)
      pairwise             a document's per-token contributions added as a balanced tree, not left to right
      drop-33rd            the token at position 32 (lane 0 of the second group) dropped
      stop-at-empty-group  a group without a kept token ends the query
      hi-counted           the upper bound of a slab's range inclusive: the posting at document hi is applied by this slab
                           as well (it lands on document hi, which the next slab scores again)
      lo-left-out          the lower bound exclusive: the posting at document lo is skipped
      negative-zero-last   the first contribution of a document stored, not added to +0.0 (model_topk then ranks -0.0
                           below +0.0)
    model=None: the walk as it should be (equals ref_scores; the CPU test checks that)."""
    n = csr["doc_len"].shape[0]
    w, pd, idf = _factor(csr), csr["post_doc"], csr["idf"]
    out = np.zeros(n, dtype=np.float64)
    stray = np.zeros(n, dtype=np.float64)
    for lo, hi in slabs:
        toks = []
        for pos, t in enumerate(q):
            a, b = term_range(csr, t, lo, hi)
            if 0 <= t < idf.shape[0]:
                p0, p1 = int(csr["term_ptr"][t]), int(csr["term_ptr"][t + 1])
                if model == "hi-counted" and hi < n:
                    b = p0 + int(np.searchsorted(pd[p0:p1], hi, "right"))
                if model == "lo-left-out" and lo > 0:
                    a = p0 + int(np.searchsorted(pd[p0:p1], lo, "right"))
            toks.append((pos, t, a, b))
        if model == "drop-33rd":
            toks = [x for x in toks if x[0] != KTOK]
        if model == "stop-at-empty-group":
            for g in range(0, len(q), KTOK):
                if not any(b > a for pos, t, a, b in toks if g <= pos < g + KTOK):
                    toks = [x for x in toks if x[0] < g]
                    break
        kept = [(t, a, b, 1) for pos, t, a, b in toks if b > a]
        if model == "term-order":
            kept.sort(key=lambda x: x[0])
        if model == "fold-repeats":
            first = {}
            for t, a, b, c in kept:
                first[t] = (t, a, b, first[t][3] + 1) if t in first else (t, a, b, 1)
            kept = list(first.values())
        acc = np.zeros(n, dtype=np.float64)
        if model == "pairwise":
            if kept:
                C = np.zeros((len(kept), n), dtype=np.float64)
                for j, (t, a, b, c) in enumerate(kept):
                    C[j, pd[a:b]] = idf[t] * w[a:b]
                while C.shape[0] > 1:
                    even = C[0:C.shape[0] - C.shape[0] % 2:2] + C[1::2]
                    C = np.concatenate([even, C[-1:]]) if C.shape[0] % 2 else even
                acc = acc + C[0]
        else:
            touched = np.zeros(n, dtype=bool)
            for t, a, b, c in kept:
                docs = pd[a:b]
                x = idf[t] * c if model == "fold-repeats" else idf[t]
                p = x * w[a:b]
                if model == "fma":
                    old = acc[docs]
                    new = old + p
                    for j in np.nonzero(old != 0.0)[0]:
                        new[j] = _fma(old[j], x, w[a + j])
                    acc[docs] = new
                elif model == "negative-zero-last":
                    acc[docs] = np.where(touched[docs], acc[docs] + p, p)
                    touched[docs] = True
                else:
                    acc[docs] += p
        out[lo:hi] = acc[lo:hi]
        if model == "hi-counted" and hi < n:
            stray[hi] = acc[hi]
    return out + stray if model == "hi-counted" else out


def model_topk(row, k, model=None):
    """ref_topk, but for "negative-zero-last" -0.0 ranks below +0.0."""
    if model != "negative-zero-last":
        return ref_topk(row, k)
    x = row + 0.0
    order = np.lexsort((np.arange(x.shape[0]), np.signbit(row) & (row == 0.0), -x))[:k]
    ids = np.full(k, -1, dtype=np.int64)
    sc = np.full(k, -float(np.finfo(np.float64).max), dtype=np.float64)
    ids[:order.shape[0]] = order
    sc[:order.shape[0]] = x[order]
    return ids, sc


_ROWS = {}


def model_row(case, qi, model):
    """Cached model_scores of query qi of the case (models that do not depend on the slabs are computed once per query)."""
    slabs = tuple(slabs_of(case.n, case.k)) if model in SLAB_MODELS else ((0, case.n),)
    key = (id(case.csr), tuple(case.queries[qi]), model, slabs)
    if key not in _ROWS:
        _ROWS[key] = (case.csr, model_scores(case.csr, case.queries[qi], slabs, model))
    return _ROWS[key][1]


def caught(case, model):
    """The first query of the case whose top k under the wrong model differs from the reference in an id or in a score
    bit, or None."""
    for qi in range(len(case.queries)):
        ei, es = ref_topk(model_row(case, qi, None), case.k)
        mi, ms = model_topk(model_row(case, qi, model), case.k, model)
        if not (np.array_equal(ei, mi) and np.array_equal(es.view(np.uint64), ms.view(np.uint64))):
            return qi
    return None


def applicable(case, model):
    """A border model needs a border: a plan of one slab has none."""
    return model not in BORDER_MODELS or bm_plan(case.n, case.k)[1] > 1


# ---- building ----------------------------------------------------------------------------------------------------------
class _Terms:
    """Term table under construction: add(name, docs, idf) -> term id; ids are handed out in a shuffled order so that
    query order and term-id order differ."""

    def __init__(self, rng, count):
        self.free = [int(i) for i in rng.permutation(count)]
        self.docs, self.idf, self.id = {}, {}, {}

    def add(self, name, docs, idf):
        t = self.free.pop()
        self.id[name], self.docs[t], self.idf[t] = t, np.asarray(sorted({int(d) for d in docs}), dtype=np.int32), float(idf)
        return t

    def csr(self, n, rng=None):
        V = len(self.docs)
        assert not self.free and sorted(self.docs) == list(range(V))
        csr = make_csr(n, [self.docs[t] for t in range(V)], [self.idf[t] for t in range(V)])
        return _vary(csr, rng) if rng is not None else csr


def _expand(family, group, n, csr, queries, edge, reached, catches, depths=DEPTHS):
    out = []
    for k in depths:
        c = Case(family, f"{family} {group} n={n} k={k}", n, k, csr, queries, edge, reached, (), group)
        c.catches = tuple(m for m in catches if applicable(c, m))
        out.append(c)
    return out


def _mixes(rng, core, everywhere, count=8):
    """`count` queries: the core terms and the all-document terms in a random order, one all-document term twice (not one
    of the near-cancelling pair everywhere[:2], so that the pair still cancels and the rounding of the large partial sums
    shows in the small total).  Every
    document sums at least len(everywhere) + 1 contributions, so each wrong order has `count` chances at every depth."""
    out = []
    for j in range(count):  # every other query without the core: no list of a few documents decides the first ranks there
        q = (list(core) if j % 2 == 0 else []) + list(everywhere) + [everywhere[int(rng.integers(2, len(everywhere)))]]
        out.append([int(q[j]) for j in rng.permutation(len(q))])
    return out


def _len_of(csr, t):
    return int(csr["term_ptr"][t + 1] - csr["term_ptr"][t])


# ---- W1: posting-list length -------------------------------------------------------------------------------------------
def alternating(n, L):
    """L documents, every other one: 0, 2, 4, ...; a list longer than n / 2 cannot skip throughout, so it skips the odd
    documents 1, 3, ... 2 (n - L) - 1 and holds every document behind them."""
    if 2 * L - 1 <= n:
        return list(range(0, 2 * L, 2))
    return sorted(set(range(n)) - set(range(1, 2 * (n - L), 2)))


def w1():
    rng = np.random.default_rng(101)
    n = W1_N
    T = _Terms(rng, 3 * len(LENGTHS) + 4)
    vals = _spread(rng, 3 * len(LENGTHS))
    for i, L in enumerate(LENGTHS):
        T.add(("first", L), range(L), vals[3 * i])
        T.add(("last", L), range(n - L, n), vals[3 * i + 1])
        T.add(("alt", L), alternating(n, L), vals[3 * i + 2])
    # four lists of every document (a near-cancelling pair among them): with them in a query EVERY document sums four
    # and more contributions, so a wrong order shows at every depth, not only where the short lists happen to rank first
    a, b = _near_cancel(rng, 21)
    bga, bgb = T.add("bga", range(n), a), T.add("bgb", range(n), b)
    bgc, bgd = T.add("bgc", range(n), _val(rng, -3)), T.add("bgd", range(n), _val(rng, 9, -1))
    csr = T.csr(n, rng)
    out = []
    for L in LENGTHS:
        f, l, x = T.id[("first", L)], T.id[("last", L)], T.id[("alt", L)]
        queries = [[f], [l], [x], [f, l], [x, f], [bga, x, bgc, f, bgb, bgd, l], [l, bgb, f, f, bgd, x, bga, bgc],
                   [bga, x, bgc, bga, x, f, bgb, bgb], [bgd, l, bga, bgc, x, bgb]] + _mixes(rng, [f, l, x], [bga, bgb, bgc, bgd])

        def reached(case, L=L, f=f, l=l, x=x):
            c = case.csr
            docs = lambda t: c["post_doc"][c["term_ptr"][t]:c["term_ptr"][t + 1]]
            assert _len_of(c, f) == _len_of(c, l) == _len_of(c, x) == L
            assert np.array_equal(docs(f), np.arange(L)) and np.array_equal(docs(l), np.arange(case.n - L, case.n))
            skip = min(L, case.n - L + 1) - 1  # the leading part of the list that takes every other document
            assert docs(x)[0] == 0 and np.all(np.diff(docs(x))[:skip] == 2) and np.all(np.diff(docs(x))[skip:] == 1)
            assert all(any(t in q for q in case.queries) for t in (f, l, x)) and [f] in case.queries
            assert len(slabs_of(case.n, case.k)) == 1
            return f"length {L} = {chunks(L)} chunks ({L % CHUNK} in the last), first / last / every other document"
        out += _expand("W1", f"L={L}", n, csr, queries, f"lists of {L} postings at the front, at the end and on every other document",
                       reached, ("term-order", "fold-repeats", "fma", "pairwise"))
    return out


# ---- W2: the prefetch window -------------------------------------------------------------------------------------------
def w2():
    rng = np.random.default_rng(202)
    n = W2_N
    lens = sorted({CHUNK * a + r for a in range(10) for r in (0, 1, 63)} - {0})
    strided = [L for L in lens if 2 * L <= n and L <= 7 * CHUNK + 63]
    T = _Terms(rng, len(lens) + len(strided) + 3 + 4)
    vals = _spread(rng, len(lens) + len(strided))
    for i, L in enumerate(lens):
        T.add(("P", L), range(L), vals[i])
    for i, L in enumerate(strided):
        T.add(("S", L), range(0, 2 * L, 2), vals[len(lens) + i])
    big, nbig = _near_cancel(rng, 38)
    T.add("BIG", range(200), big), T.add("NBIG", range(200), nbig), T.add("SMALL", range(200), _val(rng, -20))
    # four lists of every document (16 chunks = two whole windows: they move no boundary): every document sums three
    # and more contributions in the queries that hold them
    xa, xb = _near_cancel(rng, 17)
    ALLA, ALLB, ALLC = T.add("ALLA", range(n), xa), T.add("ALLB", range(n), xb), T.add("ALLC", range(n), _val(rng, -6, -1))
    EVERY = [ALLA, ALLB, ALLC, T.add("ALLD", range(n), _val(rng, 6))]
    csr = T.csr(n, rng)
    P, S = (lambda L: T.id[("P", L)]), (lambda L: T.id[("S", L)])
    BIG, NBIG, SMALL = T.id["BIG"], T.id["NBIG"], T.id["SMALL"]
    out = []

    # a token boundary at every position of the window, and exactly on its end (c = 8)
    queries = []
    for c in range(1, AHEAD + 1):
        for head in (P(CHUNK * (c - 1) + 1), P(CHUNK * c)):
            queries.append([ALLA, head, P(1), ALLC, P(577), S(65), ALLB, P(63)])

    nb = len(queries)
    queries += _mixes(rng, [P(65), P(449), S(63)], EVERY)

    def reached_b(case, nb=nb):
        got = [boundary_positions(case.csr, q, 0, case.n) for q in case.queries[:nb]]
        assert {g[1] for g in got} == set(range(AHEAD)) and {p for g in got for p in g} == set(range(AHEAD)), got
        assert all(_len_of(case.csr, q[0]) == AHEAD * CHUNK * 2 and g[0] == 0 for q, g in zip(case.queries, got))
        for q in case.queries[:nb]:  # consecutive tokens share documents: document 0 is in every list
            assert all(case.csr["post_doc"][case.csr["term_ptr"][t]] == 0 for t in q)
        return "the token behind two whole windows ends at window positions " + str(sorted({g[1] for g in got})) + " (0: on the window's end)"
    out += _expand("W2", "boundary", n, csr, queries, "a token boundary at each of the eight window positions and on the window's end",
                   reached_b, ("term-order", "fma", "pairwise"))

    # one document in chunk u and u + 1 of one window and again in the next one: ten one-chunk lists, all hold documents 0 ...
    one = [P(1), P(63), P(64), S(1), S(63), S(64), P(1), P(64), S(63), P(63), S(64), P(63)]
    queries = [one[:10], one[2:], one[::-1], [P(128), S(64), P(65), P(128), S(65), P(64), P(129)]]
    queries += _mixes(rng, one[:10], EVERY)

    def reached_s(case):
        c = case.csr
        for q in case.queries[:3]:
            assert len(q) >= 10 and all(_len_of(c, t) <= CHUNK and c["post_doc"][c["term_ptr"][t]] == 0 for t in q)
        return "document 0 is hit by ten and more consecutive one-chunk tokens: every window position, two windows"
    out += _expand("W2", "same-document", n, csr, queries, "one document in chunk u, u + 1 and in the next window", reached_s,
                   ("term-order", "fold-repeats", "fma", "pairwise"))

    queries = [[P(65), P(65)], [P(129), S(63), P(129)], [P(512), P(512)], [S(65), P(577), S(65), S(65)], [P(1), P(1), P(1), P(1), P(1)]]
    queries += _mixes(rng, [P(65), P(65), P(512), S(63), P(512)], EVERY)

    def reached_r(case):
        assert all(len(set(q)) < len(q) for q in case.queries)
        assert any(q[0] == q[1] for q in case.queries) and any(len(q) > 2 and q[0] == q[2] != q[1] for q in case.queries)
        return "repeats t, t and t, u, t"
    out += _expand("W2", "repeats", n, csr, queries, "a token repeated next to itself and with another between", reached_r,
                   ("fold-repeats", "fma"))

    queries = [[BIG, NBIG, SMALL], [BIG, SMALL, NBIG], [SMALL, BIG, NBIG, P(64)], [BIG, P(1), NBIG, SMALL, P(63), BIG],
               [NBIG, SMALL, P(65), BIG, SMALL]]
    queries += [q[:6] for q in _mixes(rng, [BIG, NBIG, SMALL], EVERY)[:2]] + _mixes(rng, [BIG, NBIG], EVERY)

    def reached_o(case):
        idf = case.csr["idf"]
        assert idf[BIG] > 2.0 ** 38 and idf[NBIG] < 0 and 0 < idf[BIG] + idf[NBIG] < idf[BIG] * 2.0 ** -39
        assert abs(idf[SMALL]) < 2.0 ** -19 and all(3 <= len(q) <= 6 for q in case.queries[:7])
        return "big, -big + tiny, small in three to six tokens"
    out += _expand("W2", "order", n, csr, queries, "sums whose value depends on the order: big, -big + tiny, small", reached_o,
                   ("term-order", "fma", "pairwise"))
    return out


# ---- W3: token groups --------------------------------------------------------------------------------------------------
def _w3_index(n, seed):
    rng = np.random.default_rng(seed)
    slab0 = slabs_of(n, 10)[0][1]
    two = len(slabs_of(n, 10)) > 1
    T = _Terms(rng, 40 + 3 + 4 + 4 + 4)
    vals = _spread(rng, 40)
    for j in range(40):
        T.add(("A", j), rng.choice(n, size=n // 6, replace=False), vals[j])
    ga, gb = _near_cancel(rng, 19)
    for j, v in enumerate((ga, gb, _val(rng, -7), _val(rng, 5, -1))):
        T.add(("G", j), range(n), v)  # every document; G0 and G1 nearly cancel
    for j in range(3):
        T.add(("E", j), [], _val(rng, 5))
    for j in range(4):  # postings in the first slab only / behind it only (one slab: two halves of it)
        T.add(("S0", j), rng.choice(slab0 - 100 if two else n // 2 - 50, size=60, replace=False), _val(rng, 8 + j, -1 if j % 2 else 1))
        base = slab0 + 50 if two else n // 2 + 50
        T.add(("S1", j), base + rng.choice(n - base, size=60, replace=False), _val(rng, 9 + j, 1 if j % 2 else -1))
    csr = T.csr(n, rng)
    return T, csr, two


def _w3_fill(T, pattern, rng, two, V):
    """Token ids for a keep pattern (as slab 0 sees it): kept -> the A terms in turn, unkept -> the four kinds in turn
    (id -1, id >= n_terms, an empty list, and - where there is a second slab - postings in the other slab only).  The
    kept token at position 32 is G0, a list of every document; its near-cancelling partner G1 and G2, G3 are the second
    to fourth kept tokens: every document's total depends on the order, and on the 33rd token."""
    kinds = [lambda j: -1, lambda j: V + 7 + j, lambda j: T.id[("E", j % 3)]] + ([lambda j: T.id[("S1", j % 4)]] if two else [])
    order = [int(j) for j in rng.permutation(40)]
    q, nk, nu = [], 0, 0
    for keep in pattern:
        if keep:
            g = 0 if len(q) == KTOK else nk if 1 <= nk <= 3 else None
            q.append(T.id[("G", g)] if g is not None else T.id[("A", order[nk % 40])])
            nk += 1
        else:
            q.append(kinds[nu % len(kinds)](nu))
            nu += 1
    return q


def w3():
    out = []
    for n, seed in zip(W3_N, (305, 303, 304)):
        T, csr, two = _w3_index(n, seed)
        V = csr["idf"].shape[0]
        rng = np.random.default_rng(seed + 10)
        G = KTOK
        groups = {
            "all-kept": [[True] * t for t in TOKEN_COUNTS],
            "alternating": [[(i + ph) % 2 == 0 for i in range(t)] for t in TOKEN_COUNTS[1:] for ph in (0, 1, 0)],
            "empty-groups": [[False] * G + [True] * 64, [True] * G + [False] * G + [True] * G, [True] * 64 + [False] * G,
                             [False] * G + [True] * 65, [True] * G + [False] * G + [True] * 33, [False] * 64 + [True],
                             [False] * 96 + [True], [False] * G + [True] * G, [True, False] * 16 + [False] * G + [False, True] * 16,
                             [False] * 33, [False] * 97],
            "lane-0-and-31": [[True] + [False] * 31, [False] * 31 + [True], [True] + [False] * 31 + [False] * 31 + [True],
                              [False] * 31 + [True] + [True] + [False] * 31 + [True] * G, [False] * 31 + [True, True],
                              [True] + [False] * 31 + [True] * G + [False] * 31 + [True] + [True],
                              [True] * G + [True] + [False] * 31 + [False] * 31 + [True], [False] * 31 + [True] + [True] * 65,
                              [True] * G + [False] * 31 + [True] + [True] * 33],
        }
        catches = {"all-kept": ("term-order", "fold-repeats", "fma", "pairwise", "drop-33rd"),
                   "alternating": ("term-order", "fma", "pairwise", "drop-33rd"),
                   "empty-groups": ("stop-at-empty-group", "fma", "pairwise"),
                   "lane-0-and-31": ("drop-33rd", "term-order", "fma")}
        edges = {"all-kept": "0 ... 97 tokens, all kept: groups of 32 kept tokens and a last group of 1, 31, 32",
                 "alternating": "kept and unkept tokens alternating, from lane 0 and from lane 1",
                 "empty-groups": "a first, a middle and a last group without a kept token; queries with no kept token at all",
                 "lane-0-and-31": "groups whose only kept token sits at lane 0 or at lane 31"}
        for name, patterns in groups.items():
            queries = [_w3_fill(T, p, rng, two, V) for p in patterns]
            if two and name == "empty-groups":  # once more without the other-slab kind: these groups stay empty in a plan of one slab
                patterns = patterns + patterns
                queries += [_w3_fill(T, p, rng, False, V) for p in patterns[:len(queries)]]

            def reached(case, patterns=patterns, name=name, two=two, V=V):
                lo, hi = slabs_of(case.n, 10)[0]
                kinds = set()
                for q, p in zip(case.queries, patterns):
                    assert kept_mask(case.csr, q, lo, hi) == list(p), (name, p)
                    for t, keep in zip(q, p):
                        if not keep:
                            kinds.add("id -1" if t == -1 else "id >= n_terms" if t >= V else "empty list" if _len_of(case.csr, t) == 0
                                      else "other slab")
                counts = sorted({len(q) for q in case.queries})
                if name in ("all-kept", "alternating"):
                    assert set(counts) | {0} == set(TOKEN_COUNTS)
                if name == "all-kept":
                    assert kinds == set()
                else:
                    assert kinds == {"id -1", "id >= n_terms", "empty list"} | ({"other slab"} if two else set()), kinds
                per_group = [[sum(p[g:g + KTOK]) for g in range(0, len(p), KTOK)] for p in patterns]
                if name == "empty-groups":
                    assert any(c[0] == 0 and sum(c) for c in per_group) and any(len(c) == 3 and c[1] == 0 and c[0] and c[2] for c in per_group)
                    assert any(c[-1] == 0 and sum(c) for c in per_group) and any(sum(c) == 0 for c in per_group)
                if name == "lane-0-and-31":
                    solo = [(p[g:g + KTOK].index(True)) for p in patterns for g in range(0, len(p), KTOK) if sum(p[g:g + KTOK]) == 1 and len(p[g:g + KTOK]) == KTOK]
                    assert {0, 31} <= set(solo)
                return f"token counts {counts}, kept per group {per_group[:4]} ..., unkept kinds {sorted(kinds)}"
            out += _expand("W3", name, n, csr, queries, edges[name], reached, catches[name])
    return out


# ---- W4: slab borders --------------------------------------------------------------------------------------------------
def _w4_index(n, seed):
    rng = np.random.default_rng(seed)
    B = borders_of(n)
    plans = sorted({tuple(slabs_of(n, k)) for k in DEPTHS}, key=len, reverse=True)  # the shallow plan first
    pieces = sorted({iv for plan in plans for iv in plan})  # every slab of every plan
    T = _Terms(rng, 5 * len(B) + 1 + 5 * len(pieces) + 1 + 3 + 4)
    for b in B:
        T.add(("both", b), [b - 1, b], _val(rng, 40))
        T.add(("lo", b), [b], _val(rng, 39))
        T.add(("hi-1", b), [b - 1], _val(rng, 39))
        T.add(("wide", b), range(b - 40, min(b + 40, n)), _val(rng, 12, -1))
        T.add(("at-hi", b), list(range(max(b - 300, 0), b - 200)) + [b], _val(rng, 37))  # its last posting is the slab's hi
    T.add("span", set(range(0, n, 7)) | {d for b in B for d in (b - 1, b)}, _val(rng, -3))
    for lo, hi in pieces:
        m = hi - lo
        inner = lo + (m // 8) + rng.choice(m - m // 4, size=min(50, m - m // 4), replace=False)
        T.add(("in+", lo, hi), inner, _val(rng, 6))
        T.add(("in-", lo, hi), inner[::2], _val(rng, 7, -1))
        up, down = _near_cancel(rng, 10)  # larger than in+ / in-: the slab's small totals keep the rounding of large partial sums
        T.add(("all+", lo, hi), range(lo, hi), up)
        T.add(("all-", lo, hi), range(lo, hi), down)
        T.add(("all~", lo, hi), range(lo, hi), _val(rng, -9))
    first, last = plans[0][0], plans[0][-1]
    T.add("skip", list(range(first[0] + 5, first[0] + 40)) + list(range(last[1] - 40, last[1] - 5)), _val(rng, 3))
    T.add("first", [0], _val(rng, 40))
    T.add("last", [n - 1], _val(rng, 30, -1))
    T.add("ends", [0, n - 1], _val(rng, 29))
    ga, gb = _near_cancel(rng, 15)
    for name, v in (("bga", ga), ("bgb", gb), ("bgc", _val(rng, -8)), ("bgd", _val(rng, 4, -1))):
        T.add(name, range(n), v)  # every document: a list that crosses every border
    return T, T.csr(n, rng), B, plans


def w4():
    out = []
    for n, seed in zip(W4_N, (401, 402, 403, 404)):
        T, csr, B, plans = _w4_index(n, seed)
        I = T.id
        s0, s9 = plans[0][0], plans[0][-1]  # the first and the last slab of the shallow plan
        ends = [[I["first"]], [I["last"]], [I["ends"]], [I["ends"], I["span"], I["first"], I[("all+",) + s0], I["last"], I["ends"]],
                [I[("all-",) + s9], I["last"], I["span"], I[("all+",) + s9], I["ends"], I["last"]]]
        bg = [I["bga"], I["bgb"], I["bgc"], I["bgd"]]
        mix_rng = np.random.default_rng(seed + 60)
        queries = list(ends) + _mixes(mix_rng, [I["first"], I["ends"], I["last"]], bg, 14)
        for b in B:
            queries += _mixes(mix_rng, [I["both", b], I["lo", b], I["hi-1", b], I["at-hi", b]], bg, 3)
        for b in B:
            queries += [[I["both", b]], [I["lo", b]], [I["hi-1", b]], [I["at-hi", b]], [I["wide", b], I["both", b], I["span"]],
                        [I["span"], I["wide", b], I["lo", b], I["hi-1", b], I["both", b], I["at-hi", b], I["lo", b]]]

        def reached_b(case, B=B, I=I):
            c = case.csr
            mine = [lo for lo, _ in slabs_of(case.n, case.k) if lo > 0]
            assert set(mine) <= set(B)
            for b in mine:  # every border of THIS plan: queried lists with postings at lo - 1 = hi - 1 and at lo = hi
                here = {(int(d) - b) for q in case.queries for t in q if 0 <= t < c["idf"].shape[0]
                        for d in c["post_doc"][c["term_ptr"][t]:c["term_ptr"][t + 1]] if b - 1 <= d <= b}
                assert here == {-1, 0}
                for name in ("both", "lo", "hi-1", "at-hi"):
                    assert [I[name, b]] in case.queries
            docs = lambda t: c["post_doc"][c["term_ptr"][t]:c["term_ptr"][t + 1]]
            assert docs(I["first"]).tolist() == [0] and docs(I["last"]).tolist() == [case.n - 1]
            small = case.n < case.k
            return (f"borders {mine}: postings at lo - 1, lo (= hi - 1, hi of the slab before); documents 0 and n - 1"
                    + ("; the slab holds fewer than k documents" if small else ""))
        out += _expand("W4", "borders", n, csr, queries, "postings exactly at lo - 1, lo, hi - 1 and hi of every border",
                       reached_b, ("hi-counted", "lo-left-out", "fma", "pairwise", "term-order"))

        queries = []
        for plan in plans:  # the slabs of the shallow plan and of the deep one: each depth finds its own among them
            for iv in plan:
                queries += [[I[("in+",) + iv]], [I[("in-",) + iv]],
                            [I[("all-",) + iv], I[("in+",) + iv], I[("in-",) + iv], I[("all-",) + iv], I[("all+",) + iv]]]
            queries += [[I[("all-",) + iv] for iv in plan if iv != z] for z in plan]   # the zero slab outranks the others
            queries += [[I[("all+",) + iv] for iv in plan if iv != z] for z in plan]   # ... and here it does not
        queries += [[I["skip"]], [I["skip"], I[("in-",) + s0], I["span"], I["skip"]], [I[("in+",) + s0], I[("in-",) + s9]]]
        for plan in plans:  # one slab scored by six tokens (its documents sum four and more: a near-cancelling pair around a small term), every other slab untouched
            for iv in plan:
                core = [I[(x,) + iv] for x in ("all-", "all~", "in+", "all+", "in-", "all~")]
                queries += [[core[j] for j in mix_rng.permutation(6)] for _ in range(7)]
        queries = [q for i, q in enumerate(queries) if q and q not in queries[:i]]

        def reached_z(case):
            c = case.csr
            slabs = slabs_of(case.n, case.k)
            zero = neg = pos = inside = skipped = 0
            for q in case.queries:
                touched = [any(kept_mask(c, q, lo, hi)) for lo, hi in slabs]
                row = ref_scores(c, [q])[0]
                if len(slabs) > 1 and not all(touched) and any(touched):
                    zero += 1
                    tot = [row[lo:hi] for (lo, hi), t in zip(slabs, touched) if t]
                    neg += all(np.all(x < 0) for x in tot)
                    pos += all(np.all(x > 0) for x in tot)
                if len(q) == 1:
                    d = c["post_doc"][c["term_ptr"][q[0]]:c["term_ptr"][q[0] + 1]]
                    at = [bool(np.any((d >= lo) & (d < hi))) for lo, hi in slabs]
                    inside += sum(at) == 1
                    skipped += len(slabs) > 2 and at[0] and at[-1] and not all(at)
            if len(slabs) > 1:
                assert zero and neg and pos and inside, (zero, neg, pos, inside)
                assert skipped or len(slabs) < 3
            return (f"{len(slabs)} slabs: {zero} queries leave a slab untouched ({neg} with only negative totals elsewhere, "
                    f"{pos} with only positive ones), {inside} lists inside one slab, {skipped} skip a slab")
        out += _expand("W4", "zero-slabs", n, csr, queries, "queries that miss a slab with every token; lists inside one slab; lists that skip one",
                       reached_z, ("term-order", "fold-repeats", "fma", "pairwise"))
    return out


# ---- W5: zero sums -----------------------------------------------------------------------------------------------------
def w5():
    out = []
    for n, seed in zip(W5_N, (503, 501, 502)):
        rng = np.random.default_rng(seed)
        T = _Terms(rng, 13)
        D1 = rng.choice(n, size=40, replace=False)
        D2 = np.concatenate([D1[:15], rng.choice(np.setdiff1d(np.arange(n), D1), size=25, replace=False)])
        a, b, s = _val(rng, 30), _val(rng, 12), _val(rng, -20)
        for name, docs, v in (("P1", D1, a), ("N1", D1, -a), ("P2", D2, b), ("N2", D2, -b), ("SM", D1, s), ("SM2", D2, -s),
                              ("Z", range(6), -0.0), ("ZP", D2, 0.0), ("PALL", range(n), b), ("NALL", range(n), -b),
                              ("ZALL", range(n), -0.0), ("PH", range(n // 2), a), ("NH", range(n // 2), -a)):
            T.add(name, docs, v)
        csr = T.csr(n)  # tf = 1, doc_len == avgdl: every factor is 1.0 and a - a is exactly zero
        I = T.id
        zero = [[I["P1"], I["N1"]], [I["N1"], I["P1"]], [I["P1"], I["P1"], I["N1"], I["N1"]], [I["PALL"], I["NALL"]],
                [I["NALL"], I["PALL"], I["P2"], I["N2"]], [I["Z"]], [I["Z"], I["Z"]], [I["ZALL"]], [I["ZP"], I["Z"]],
                [I["P1"], I["N1"], I["Z"]], [I["PH"], I["NH"], I["ZALL"]], [I["N2"], I["ZP"], I["P2"]]]

        def reached_0(case, zero=zero):
            assert np.all(posting_factor(case.csr) == 1.0)
            rows = ref_scores(case.csr, case.queries)
            assert np.all(rows == 0.0) and not np.any(np.signbit(rows))  # every sum is +0.0: -0.0 cannot be reached
            idf = case.csr["idf"]
            prod_neg = sum(all(np.signbit(idf[t]) and idf[t] == 0.0 for t in q) for q in case.queries)
            cancel = sum(any(idf[t] != 0.0 for t in q) for q in case.queries)
            for q in case.queries:  # all tokens kept in some slab, yet nothing scores
                assert all(_len_of(case.csr, t) > 0 for t in q)
            full = sum(any(_len_of(case.csr, t) == case.n for t in q) for q in case.queries)
            assert prod_neg >= 3 and cancel >= 6 and full >= 3
            return (f"{cancel} queries cancel to +0.0, {prod_neg} add only products of -0.0; {full} touch every document: "
                    "all tokens kept, every score zero")
        out += _expand("W5", "all-zero", n, csr, zero, "every token kept, every score exactly zero: the first k ids", reached_0,
                       ("negative-zero-last",))

        ties = [[I["P1"], I["SM"], I["N1"]], [I["P1"], I["N1"], I["P2"]], [I["P1"], I["N1"], I["N2"]], [I["SM"], I["P1"], I["SM"], I["N1"]],
                [I["P1"], I["SM"], I["N1"], I["SM"]], [I["P2"], I["SM2"], I["P1"], I["N2"], I["SM"], I["N1"]],
                [I["NALL"], I["P2"], I["PALL"], I["N2"], I["Z"]], [I["Z"], I["P1"], I["SM"], I["N1"], I["SM"]]]

        def reached_t(case):
            rows = ref_scores(case.csr, case.queries)
            tied = lost = 0
            for q, row in zip(case.queries, rows):
                touched = np.zeros(case.n, dtype=bool)
                for t in q:
                    touched[case.csr["post_doc"][case.csr["term_ptr"][t]:case.csr["term_ptr"][t + 1]]] = True
                tied += bool(np.any(touched & (row == 0.0)) and np.any(~touched))
                lost += bool(np.any((row != 0.0) & (np.abs(row) < 2.0 ** -10)))
            assert tied >= 3 and lost >= 3 and not np.any(np.signbit(rows) & (rows == 0.0))
            return f"{tied} queries leave touched documents at +0.0 beside untouched ones; {lost} keep only the rounding residue of a small term"
        out += _expand("W5", "ties-and-residues", n, csr, ties, "touched documents tie with untouched ones at +0.0; big + small - big",
                       reached_t, ("term-order", "fold-repeats", "pairwise"))
    return out


def all_cases():
    return w1() + w2() + w3() + w4() + w5()


# ---- scopes of the scoped twin -----------------------------------------------------------------------------------------
def scope_lists(n, borders):
    """Row lists (ascending document ids) for scope_bm25_piece: every document, every other one, the 8 documents on
    each side of every BM25 slab border, the empty scope, and scopes of 1, 64, 65, 1024 and 1025 documents."""
    rng = np.random.default_rng(n)
    lists = [np.arange(n), np.arange(0, n, 2),
             np.asarray(sorted({d for b in borders for d in range(b - 8, b + 8) if 0 <= d < n}), dtype=np.int64),
             np.zeros(0, dtype=np.int64)]
    for m in (1, 64, 65, 1024, 1025):
        if m <= n:
            lists.append(np.sort(rng.choice(n, size=m, replace=False)))
    return [np.asarray(r, dtype=np.int64) for r in lists]


def ref_scoped_topk(row, rows, k):
    """ref_scores restricted to the scope, then ref_topk: (ids, scores) with document ids of the corpus."""
    ids, sc = ref_topk(row[rows], k)
    out = np.full(k, -1, dtype=np.int64)
    out[ids >= 0] = rows[ids[ids >= 0]]  # rows ascend: a tie by position is a tie by document id
    return out, sc

"""Batches for the fusion, rerank-blend and compaction kernels (csrc/fuse.hip, csrc/fuse_core.hpp) and what the oracle
(oracle/fusion.py) says they must write, laid out as the kernels write it.  numpy + oracle.fusion only.

launch_fuse picks one of four differently written forms from max_out = kd + kb + kc (and, inside fuse_kernel, from the size
U of the union of ids): fuse_packed_kernel<16> (4 queries per wave), fuse_packed_kernel<32> (2 per wave), fuse_kernel with
U <= 64 (values in registers) and with U > 64 (two evaluations, rank loop over LDS).  The builders here put DIFFERENT kinds
of queries side by side in one batch — and therefore in one wave of the packed forms — so that a slip in a per-segment
ballot, in the wave-wide loop bound of the union search or in the wave-wide choice between the descending-list shortcut and
the reductions changes some query's answer.

Contract of a channel list: a valid prefix, then -1 ids; ids unique inside a channel; a list that is not
descending is accepted, rank = list position.  Scores under the padding are random garbage here, not 0, so a kernel that
reads past the prefix shows.  Dense and ColBERT scores are float32 values (held in float64 arrays), so the float32 call
(amdr_fuse_device) and the float64 call (amdr_fuse) see the same numbers.  NaN and +-inf channel scores are undefined."""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import fusion as F

# AMDR_FV_* (include/amdretrieval.h), in order
FV = ("score", "rrf_norm", "weighted_sum", "dense_norm", "bm25_norm", "colbert_norm", "contrib_dense", "contrib_bm25",
      "contrib_colbert")
NVALS = len(FV)
METHODS = ("rrf_norm_blend", "rrf", "wrrf", "weighted_sum")
P16, P32, LONG_REG, LONG_LDS = "fuse_packed_kernel<16>", "fuse_packed_kernel<32>", "fuse_kernel U<=64", "fuse_kernel U>64"

# (kd, kb, kc) of part a: every route, each boundary of launch_fuse and of fuse_kernel's U <= 64 test
SHAPES = ((5, 5, 5), (8, 8, 0), (10, 0, 0), (10, 7, 0), (10, 10, 10), (16, 16, 0), (11, 11, 11), (32, 32, 0), (22, 22, 21),
          (256, 256, 256))
NQS = (1, 2, 3, 4, 5, 7, 67)  # every remainder of 4 and of 2, several waves
NQ_MAX = max(NQS)
# the edge cases run on these: <16>, <32>, fuse_kernel in registers, fuse_kernel over LDS
ROUTE_SHAPES = ((5, 5, 5), (10, 10, 10), (11, 11, 11), (22, 22, 21))
MIN_FINAL = 0.2  # the filter of part a; the rerank inputs come from it, so count < U occurs
SCORE_RANGE = ((-1.0, 1.0), (0.0, 40.0), (0.0, 30.0))
KINDS = ("disjoint", "overlap", "no_middle", "empty", "ragged")


def route(max_out: int, union: int) -> str:
    """launch_fuse + the branch inside fuse_kernel, restated."""
    if max_out <= 16:
        return P16
    if max_out <= 32:
        return P32
    return LONG_REG if union <= 64 else LONG_LDS


def knobs(method="rrf_norm_blend", rrf_k=60, alpha=0.5, w=(0.6, 0.4, 0.35)) -> dict:
    return {"fusion_method": method, "rrf_k": int(rrf_k), "rrf_alpha": float(alpha), "dense_weight": float(w[0]),
            "bm25_weight": float(w[1]), "colbert_weight": float(w[2])}


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def pack(lists, shape, seed):
    """Per-query channel lists -> ids i64 [nq, k] and scores f64 [nq, k] per channel: -1 ids and garbage scores past the
    valid prefix."""
    rng = np.random.default_rng([int(seed), 0xFA])
    nq = len(lists)
    ids = [np.full((nq, k), -1, dtype=np.int64) for k in shape]
    scores = []
    for c, k in enumerate(shape):
        g = rng.standard_normal((nq, k)) * 100.0
        scores.append(g.astype(np.float32).astype(np.float64) if c != 1 else g)
    for q, chans in enumerate(lists):
        for c, pairs in enumerate(chans):
            assert len(pairs) <= shape[c], (q, c, len(pairs), shape)
            assert len({i for i, _ in pairs}) == len(pairs), "ids are unique inside a channel"
            for j, (i, s) in enumerate(pairs):
                assert i >= 0 and math.isfinite(s) and (c == 1 or float(np.float32(s)) == s), (q, c, j, i, s)
                ids[c][q, j] = i
                scores[c][q, j] = s
    return ids, scores


class Batch:
    """lists[q] = (dense, bm25, colbert), each [(id, score), ...]; ids[c] / scores[c] the same lists packed."""

    def __init__(self, lists, shape, seed=0, kinds=None):
        self.lists = [tuple(list(ch) for ch in q) for q in lists]
        self.shape = tuple(int(k) for k in shape)
        self.kinds = list(kinds) if kinds is not None else [None] * len(lists)
        self.ids, self.scores = pack(self.lists, self.shape, seed)
        frozen(*self.ids, *self.scores)

    @property
    def nq(self):
        return len(self.lists)

    @property
    def max_out(self):
        return sum(self.shape)

    def head(self, nq):
        """The first nq queries (the same arrays: a batch of 67 is built once, its prefixes are the smaller batches)."""
        b = object.__new__(Batch)
        b.lists, b.shape, b.kinds = self.lists[:nq], self.shape, self.kinds[:nq]
        b.ids, b.scores = [a[:nq] for a in self.ids], [a[:nq] for a in self.scores]
        return b

    def host_args(self):
        """(ids, scores f64) per channel as _native.fuse takes them; None for a channel of depth 0."""
        return [(self.ids[c], self.scores[c]) if k else None for c, k in enumerate(self.shape)]

    def widened(self, kc, seed=0):
        """The same lists with an all -1 ColBERT block of width kc (route independence)."""
        assert self.shape[2] == 0 and all(not q[2] for q in self.lists)
        return Batch(self.lists, (self.shape[0], self.shape[1], kc), seed, self.kinds)

    def unions(self):
        return [len({i for ch in q for i, _ in ch}) for q in self.lists]

    def routes(self):
        return {route(self.max_out, u) for u in self.unions()}


def _desc(rng, c, n, lo=None, hi=None):
    lo, hi = SCORE_RANGE[c] if lo is None else (lo, hi)
    s = np.sort(rng.uniform(lo, hi, size=n))[::-1]
    if c != 1:
        s = s.astype(np.float32)
    return [float(x) for x in s]


def _query(kind, shape, rng, off):
    kmax = max(shape)
    if kind == "disjoint":  # U = max_out
        idl = [off + c * 4096 + rng.permutation(4096)[:k] for c, k in enumerate(shape)]
    elif kind == "overlap":  # small U: every channel draws from a pool barely larger than one list
        pool = off + rng.permutation(kmax + 2)
        idl = [rng.permutation(pool)[:int(rng.integers(1, k + 1))] if k else [] for k in shape]
    elif kind == "no_middle":  # the middle channel is all -1
        pool = off + rng.permutation(2 * kmax)
        idl = [rng.permutation(pool)[:int(rng.integers(1, k + 1))] if k and c != 1 else [] for c, k in enumerate(shape)]
    elif kind == "empty":  # union 0, count 0, all padding
        idl = [[] for _ in shape]
    else:  # ragged
        pool = off + rng.permutation(3 * kmax)
        idl = [rng.permutation(pool)[:int(rng.integers(0, k + 1))] if k else [] for k in shape]
    return tuple([(int(i), s) for i, s in zip(ids, _desc(rng, c, len(ids)))] for c, ids in enumerate(idl))


def _offset(q):  # ids differ between queries (a neighbour's entry never matches by accident); odd queries need 64 bits
    return q * 100000 + ((1 << 40) if q % 2 else 0)


@functools.lru_cache(maxsize=None)
def mixed_batch(shape, seed=1):
    """NQ_MAX queries, kinds in KINDS order: 5 is coprime to 4 and 2, so every kind meets every segment of a wave."""
    rng = np.random.default_rng([int(seed), *shape])
    kinds = [KINDS[q % len(KINDS)] for q in range(NQ_MAX)]
    return Batch([_query(k, shape, rng, _offset(q)) for q, k in enumerate(kinds)], shape, seed, kinds)


def expected_arrays(lists, kn, min_final, max_out, keep_order=False):
    """oracle.fusion.fuse per query, as the kernels write it: ids [nq, max_out], vals [nq, max_out, 9] in AMDR_FV_* order,
    mask (bit c: the id is in channel c), count (hits with score >= min_final: a prefix, the rows are sorted).  Rows past the
    union hold -1 / 0 / 0.0."""
    nq = len(lists)
    ids = np.full((nq, max_out), -1, dtype=np.int64)
    vals = np.zeros((nq, max_out, NVALS), dtype=np.float64)
    mask = np.zeros((nq, max_out), dtype=np.int32)
    count = np.zeros((nq,), dtype=np.int32)
    for q, (d, b, c) in enumerate(lists):
        hits = F.fuse(d, b, c, kn, keep_order=keep_order)
        assert len(hits) <= max_out
        for r, h in enumerate(hits):
            sb = h["breakdown"]
            con = sb["channel_contrib"]
            ids[q, r] = h["id"]
            vals[q, r] = (h["score"], sb["rrf_norm"], sb["weighted_sum"], sb["dense_norm"], sb["bm25_norm"],
                          sb["colbert_norm"], con["dense"], con["bm25"], con["colbert"])
            mask[q, r] = sum(1 << F.CHANNELS.index(ch) for ch in sb["channel"])
        count[q] = sum(1 for h in hits if h["score"] >= min_final)
    return ids, vals, mask, count


@functools.lru_cache(maxsize=None)
def expected_mixed(shape, method):
    """Part a's reference: computed once per (shape, method) for the 67 queries; smaller batches are its first rows."""
    return frozen(*expected_arrays(mixed_batch(shape).lists, knobs(method), MIN_FINAL, sum(shape)))


def head(arrays, nq):
    return tuple(a[:nq] for a in arrays)


# ---- c. knob edges (on mixed_batch(shape).head(5): one query of every kind) ----------------------------------------------
KNOB_EDGES = (
    ("alpha=0", knobs(alpha=0.0)), ("alpha=1", knobs(alpha=1.0)),
    ("wrrf w=(0,.4,.35)", knobs("wrrf", w=(0.0, 0.4, 0.35))), ("wrrf w=(0,0,.35)", knobs("wrrf", w=(0.0, 0.0, 0.35))),
    ("wrrf w=(.6,0,0)", knobs("wrrf", w=(0.6, 0.0, 0.0))), ("wrrf w=(0,0,0)", knobs("wrrf", w=(0.0, 0.0, 0.0))),
    ("blend w=(0,.4,.35)", knobs(w=(0.0, 0.4, 0.35))), ("blend w=(0,0,.35)", knobs(w=(0.0, 0.0, 0.35))),
    ("blend w=(0,0,0)", knobs(w=(0.0, 0.0, 0.0))), ("wsum w=(.6,0,.35)", knobs("weighted_sum", w=(0.6, 0.0, 0.35))),
    # an RRF total of exactly 0 that is NOT the smallest (mass > 0, t <= 1e-18: the empty allocation) needs a negative weight
    ("wrrf w=(-.5,0,.35)", knobs("wrrf", w=(-0.5, 0.0, 0.35))),
    ("rrf k=0", knobs("rrf", rrf_k=0)), ("rrf k=1", knobs("rrf", rrf_k=1)), ("rrf k=1000", knobs("rrf", rrf_k=1000)),
    ("blend k=0", knobs(rrf_k=0)), ("blend k=1000", knobs(rrf_k=1000)), ("wrrf k=0", knobs("wrrf", rrf_k=0)),
)


def min_final_edges(lists, kn):
    """A candidate's own score (>= keeps it), the next double above it (drops it), +inf (count 0), -inf.  The candidate is
    the middle hit of query 0, whose score no other hit of that query shares."""
    hits = F.fuse(*lists[0], kn)
    s = hits[len(hits) // 2]["score"]
    assert sum(1 for h in hits if h["score"] == s) == 1
    return (s, math.nextafter(s, math.inf), math.inf, -math.inf)


# ---- c. value edges ---------------------------------------------------------------------------------------------------------
SPAN_BELOW, SPAN_ABOVE = 2.0 ** -40, 2.0 ** -39  # on either side of _minmax's 1e-12
VALUE_KINDS = ("span_below", "span_above", "one_entry", "negative", "flat")


def _span_scores(n, span, base=2.0 ** -30):
    """n >= 2 non-increasing float32 values from base + span down to base: hi - lo is exactly `span`."""
    assert n >= 2
    out = [base + span * (((n - 1 - j) * 4 // (n - 1)) / 4.0) for j in range(n)]
    assert out[0] - out[-1] == span and all(float(np.float32(x)) == x for x in out)
    return out


def value_edge_batch(shape, seed=2):
    """One query per VALUE_KINDS entry (nq = 5).  span_below: dense and ColBERT span 2^-40 (norms all 0), BM25 2^-39;
    span_above the reverse; one_entry: every channel holds one id; negative: all scores < 0; flat: every channel constant."""
    rng = np.random.default_rng([int(seed), *shape])
    lists = []
    for q, kind in enumerate(VALUE_KINDS):
        off = _offset(q)
        pool = off + rng.permutation(max(shape) + 3)
        n = [1 if kind == "one_entry" else k for k in shape]
        idl = [rng.permutation(pool)[:nc] if k else [] for nc, k in zip(n, shape)]
        chans = []
        for c, ids in enumerate(idl):
            if kind in ("span_below", "span_above") and len(ids) >= 2:
                low = (kind == "span_below") == (c != 1)
                sc = _span_scores(len(ids), SPAN_BELOW if low else SPAN_ABOVE)
            elif kind == "negative":
                sc = _desc(rng, c, len(ids), -50.0, -1.0)
            elif kind == "flat":
                sc = [float(np.float32(3.25 + c))] * len(ids)
            else:
                sc = _desc(rng, c, len(ids))
            chans.append([(int(i), s) for i, s in zip(ids, sc)])
        lists.append(tuple(chans))
    return Batch(lists, shape, seed, VALUE_KINDS)


# ---- d. exact ties in the fused score -------------------------------------------------------------------------------------
TIE_KINDS = ("disjoint", "mirrored", "flat")


def tie_batch(shape, nq=7, seed=3):
    """disjoint: under rrf, rank r of every channel has the same total (in the U > 64 route the tied candidates sit in
    different 64-chunks of the union).  mirrored: BM25 holds the dense ids with adjacent pairs swapped — A first / second,
    B second / first: equal totals, A appeared first.  flat: every channel constant, so weighted_sum is 0.0 for every
    candidate.  Kinds cycle, so segments 1..3 of a packed wave hold ties."""
    rng = np.random.default_rng([int(seed), *shape])
    lists, kinds = [], []
    for q in range(nq):
        kind = TIE_KINDS[q % len(TIE_KINDS)]
        off = _offset(q)
        if kind == "disjoint":
            chans = _query("disjoint", shape, rng, off)
        elif kind == "mirrored":
            kd, kb, kc = shape
            a = [int(x) for x in off + rng.permutation(4096)[:kd]]
            m = min(kd, kb) // 2 * 2
            b = [a[j ^ 1] for j in range(m)] + [off + 5000 + j for j in range(kb - m)]
            c = [off + 6000 + j for j in range(kc)]
            chans = tuple([(i, s) for i, s in zip(ids, _desc(rng, ch, len(ids)))] for ch, ids in enumerate((a, b, c)))
        else:
            pool = off + rng.permutation(max(shape) + 2)
            chans = tuple([(int(i), float(np.float32(1.5 + c))) for i in rng.permutation(pool)[:k]] for c, k in enumerate(shape))
        lists.append(chans)
        kinds.append(kind)
    return Batch(lists, shape, seed, kinds)


def tie_groups(hits):
    """Runs of exactly equal fused scores in an oracle result: lists of ids."""
    groups, run = [], []
    for h in hits:
        if run and h["score"] != run[-1]["score"]:
            groups.append([x["id"] for x in run])
            run = []
        run.append(h)
    if run:
        groups.append([x["id"] for x in run])
    return [g for g in groups if len(g) > 1]


def union_positions(chans):
    """id -> position in the union (first-appearance order over dense, bm25, colbert)."""
    pos = {}
    for ch in chans:
        for i, _ in ch:
            pos.setdefault(i, len(pos))
    return pos


# ---- e. lists that are not descending ---------------------------------------------------------------------------------------
def shuffled(batch, queries, seed=4):
    """The batch with every channel list of the given queries permuted so that its first entry is not its maximum (lists of
    two or more distinct scores).  The reference for such a batch is expected_arrays(..., keep_order=True)."""
    rng = np.random.default_rng([int(seed), *batch.shape])
    lists = [tuple(list(ch) for ch in q) for q in batch.lists]
    for q in queries:
        for ch in lists[q]:
            if len(ch) < 2:
                continue
            ch[:] = [ch[j] for j in rng.permutation(len(ch))]
            top = max(range(len(ch)), key=lambda j: ch[j][1])
            if top == 0:
                ch[0], ch[-1] = ch[-1], ch[0]
    return Batch(lists, batch.shape, seed, batch.kinds)


def is_descending(ch):
    return all(ch[j][1] >= ch[j + 1][1] for j in range(len(ch) - 1))


# ---- b. row2uid maps ----------------------------------------------------------------------------------------------------------
def map_batch(shape, nq=5, seed=5):
    """Lists of ROWS in [0, R) and one injective row -> uid map per channel onto the same uid range [0, R): different rows of
    different channels meet at one uid, the same row number means different uids, and a channel left without a map (its rows
    are its uids) still collides with the mapped ones.  Query 0 is full depth, the others ragged."""
    rng = np.random.default_rng([int(seed), *shape])
    R = 2 * max(shape) + 8
    maps = frozen(*[rng.permutation(R).astype(np.int64) for _ in shape])
    lists = []
    for q in range(nq):
        n = [k if q == 0 else int(rng.integers(0, k + 1)) for k in shape]
        lists.append(tuple([(int(i), s) for i, s in zip(rng.permutation(R)[:nc], _desc(rng, c, nc))] for c, nc in enumerate(n)))
    return Batch(lists, shape, seed), maps


def mapped_lists(lists, maps):
    return [tuple([(int(m[i]) if m is not None else i, s) for i, s in ch] for ch, m in zip(q, maps)) for q in lists]


# ---- the packed forms' wave-wide loop bound -------------------------------------------------------------------------------
def union_search_depth(chans):
    """Per channel c: (U0 = union size before the channel, deepest union position one of its entries matches, or -1)."""
    pos, out = {}, []
    for ch in chans:
        u0 = len(pos)
        deepest = max([pos[i] for i, _ in ch if i in pos], default=-1)
        out.append((u0, deepest))
        for i, _ in ch:
            pos.setdefault(i, len(pos))
    return out


def needs_the_longest_union(lists, per_wave):
    """Waves (groups of per_wave consecutive queries) in which a query of segment >= 1 finds a match at a union position
    that segment 0's own union (rounded up to the search's step of 4) does not reach: taking the loop bound from segment 0
    alone loses that match."""
    found = []
    for w0 in range(0, len(lists), per_wave):
        depth = [union_search_depth(q) for q in lists[w0:w0 + per_wave]]
        for seg in range(1, len(depth)):
            for c in range(3):
                if depth[seg][c][1] >= (depth[0][c][0] + 3) // 4 * 4:
                    found.append((w0, seg, c))
    return found


# ---- g. rerank blend ------------------------------------------------------------------------------------------------------------
RERANK_SHAPES = ((1, 0, 0), (10, 10, 0), (32, 32, 0), (22, 22, 21), (256, 256, 256))  # max_out 1, 20, 64, 65, 768
RERANK_NQS = (1, 5, 67)
BETAS = (0.0, 0.35, 1.0)
CE_KINDS = ("random", "equal", "span_below", "span_above", "duplicates")


@functools.lru_cache(maxsize=None)
def rerank_input(shape, method):
    """Part a's fused record of the 67 mixed queries (min_final 0.2).  The count is the filter's, except that every other
    'disjoint' query keeps all of its max_out candidates (as under min_final = -inf) so that count runs from 0 ('empty'
    queries) to max_out inside one batch."""
    ids, vals, mask, count = expected_mixed(shape, method)
    count = count.copy()
    b = mixed_batch(shape)
    for q in range(0, b.nq, 2 * len(KINDS)):
        assert b.kinds[q] == "disjoint"
        count[q] = b.max_out
    return ids, vals, mask, frozen(count)


@functools.lru_cache(maxsize=None)
def ce_scores(nq, top_n, seed=6):
    """Cross-encoder raw scores [nq, top_n], kind by query in CE_KINDS order: random; all equal (norm 0); three values
    spanning 2^-40 / 2^-39 around 1.0 (norm 0 / not); draws from four values (exact duplicates: the stable order decides)."""
    rng = np.random.default_rng([int(seed), nq, top_n])
    out = np.empty((nq, top_n), dtype=np.float64)
    for q in range(nq):
        kind = CE_KINDS[q % len(CE_KINDS)]
        if kind == "random":
            out[q] = rng.normal(0.0, 4.0, size=top_n)
        elif kind == "equal":
            out[q] = -2.5
        elif kind in ("span_below", "span_above"):
            span = SPAN_BELOW if kind == "span_below" else SPAN_ABOVE
            out[q] = 1.0 + span * (np.arange(top_n) % 3) / 2.0
        else:
            out[q] = rng.choice(np.array([-1.0, 0.25, 0.5, 3.0]), size=top_n)
    return frozen(out)


def top_ns(count, max_out):
    """1, a count of the batch that lies strictly inside (0, max_out) where there is one, max_out, and above max_out: below,
    at and above counts of the batch."""
    inner = sorted({int(c) for c in count if 0 < c < max_out})
    return sorted({1, inner[len(inner) // 2] if inner else 1, max_out, max_out + 3})


def expected_rerank(ids, vals, mask, count, ce_raw, top_n, beta):
    """oracle.fusion.rerank_blend on the first count[q] hits of every query with raw = ce_raw[q, :min(top_n, count[q])].
    Returns new ids, vals (the score replaced, the other eight values travelling with their id), mask and out_rerank
    [nq, max_out, 2] (raw, norm; NaN where the hit's source is not "rerank").  Rows [count, max_out) equal the input."""
    nq, max_out = ids.shape
    oi, ov, om = ids.copy(), vals.copy(), mask.copy()
    rer = np.full((nq, max_out, 2), np.nan, dtype=np.float64)
    for q in range(nq):
        cnt = int(count[q])
        n = min(int(top_n), cnt)
        if n <= 0:
            continue
        fused = [{"id": j, "score": float(vals[q, j, 0]), "rank": j + 1, "source": "retriever", "breakdown": {}}
                 for j in range(cnt)]
        out = F.rerank_blend(fused, [float(x) for x in ce_raw[q, :n]], float(beta))
        assert len(out) == cnt
        src = np.array([h["id"] for h in out], dtype=np.int64)
        oi[q, :cnt], ov[q, :cnt], om[q, :cnt] = ids[q, src], vals[q, src], mask[q, src]
        ov[q, :cnt, 0] = [h["score"] for h in out]
        for r, h in enumerate(out):
            if h["source"] == "rerank":
                rer[q, r] = (h["breakdown"]["rerank_raw"], h["breakdown"]["rerank_norm"])
    assert all((oi[q, count[q]:] == ids[q, count[q]:]).all() for q in range(nq))
    return oi, ov, om, rer


# ---- h. compaction ----------------------------------------------------------------------------------------------------------------
COMPACT_MAX_OUT = 4
# (nq, w): nq * w below, at and above 256 and 512 (fuse_compact_kernel's blocks of 256 threads), w = 1, 3, max_out
COMPACT_CASES = tuple((nq, 1) for nq in (1, 255, 256, 257, 511, 512, 513)) + \
    tuple((nq, 3) for nq in (5, 85, 86, 170, 171)) + tuple((nq, COMPACT_MAX_OUT) for nq in (63, 64, 65, 127, 128, 129))


def compact_record(nq, max_out=COMPACT_MAX_OUT, seed=7):
    """A synthetic fused record; counts cycle through 0 .. max_out (0, below w, above w for every w)."""
    rng = np.random.default_rng([int(seed), nq])
    ids = rng.integers(0, 1 << 40, size=(nq, max_out), dtype=np.int64)
    vals = rng.standard_normal((nq, max_out, NVALS))
    mask = rng.integers(1, 8, size=(nq, max_out), dtype=np.int32)
    count = (np.arange(nq) % (max_out + 1)).astype(np.int32)
    return ids, vals, mask, count


# ---- comparison -------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def first_difference(got, exp):
    d = np.argwhere(np.asarray(got) != np.asarray(exp))
    return tuple(int(x) for x in d[0]) if len(d) else None


def assert_record(got, exp, what):
    """ids, vals (bit patterns of all nine values), mask, count: whole arrays, ==."""
    for name, g, e in zip(("ids", "vals", "mask", "count"), got, exp):
        g, e = np.asarray(g), np.asarray(e)
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape, g.dtype, e.dtype)
        gb, eb = (bits(g), bits(e)) if name == "vals" else (g, e)
        at = first_difference(gb, eb)
        assert at is None, (what, name, "first difference at", at, "got", g[at], "expected", e[at])

"""Per-rank top-k lists for the shard exchange (csrc/shard.hip: shard_pack_kernel, shard_merge_kernel) at the edges of its
values, depths and shard sizes, and the reference of their merge.

The merge ranks the world * k candidates of a (query, channel) by (score descending, global id ascending) on one of three
paths: a register bitonic sort over 64 lanes (world * k <= 64), a second sorted half folded in (64 < world * k <= 128,
k <= 64), and the staged WaveTopK selector (world * k > 128 or k > 64).  A launch that holds one deep channel is the staged
kernel for all of them, and runs its shallow channels through the register path.  A wrong merge does not fault: it returns
a plausible list with a hit missing or two swapped, the same on every rank.

A case is `world` ranks x channels (k, dtype) x `nq` queries plus one id offset per rank.  Every list has the form a
channel search hands over: sorted by (score descending, id ascending) with a NaN behind every number and -0.0 == +0.0,
LOCAL ids, padding only at the tail (id -1, score -FLT_MAX / -DBL_MAX).  The ROGUE variant of a case keeps that shape but
writes a large score (9e9) and ids -1, -2 or -(2^40) on the padded entries: the ids decide what is padding, never the
scores, and a negative id passes the pack unchanged whatever the offset.

The reference is oracle/dense.py merge_topk per channel on the GLOBAL ids, in fp64 throughout (an fp32 score widens
exactly, which is also what the wire format does).  The kernel differs from it in three documented ways, applied by
kernel_view():
  * the oracle pads with -inf, the kernel with -FLT_MAX (fp32 channel) / -DBL_MAX (fp64 channel), id -1;
  * a -0.0 hit comes back as +0.0 (ord64 adds +0.0 so that the two zeros tie and the id decides);
  * any NaN comes back as a NaN (key 1: behind -inf, ahead of padding; the payload is not kept).

Not a test module (no test_ prefix): tests/test_shard_adversary.py checks on the CPU that the EXPECTED OUTPUTS hold every
edge, tests/test_shard_adversary_gpu.py runs the cases on the device.  numpy only.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

F32, F64 = np.float32, np.float64
FLT_MAX = np.float32(np.finfo(np.float32).max)
DBL_MAX = np.float64(np.finfo(np.float64).max)
# the NaN the selectors of topk.hpp give back (unord32 / unord64 of key 1), and a NaN of another payload
NAN32 = np.array([0xFFFFFFFE], dtype=np.uint32).view(np.float32)[0]
NAN64 = np.array([0xFFFFFFFFFFFFFFFE], dtype=np.uint64).view(np.float64)[0]
OTHER_NAN32 = np.array([0x7FC00001], dtype=np.uint32).view(np.float32)[0]
OTHER_NAN64 = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]
FIVE = (-0.5, -0.25, 0.0, 0.25, 1.0)  # "most candidates tie"
ROGUE_SCORE = 9e9
ROGUE_IDS = (-1, -2, -(1 << 40))
N_ROWS = 400  # rows of a rank's block unless a list is deeper

# the borders of the kernel's own conditions
TOTALS = (1, 63, 64, 65, 127, 128, 129)
KS = (1, 63, 64, 65, 255, 256)
BORDER_PAIRS = ((1, 64), (2, 64), (1, 65), (2, 65), (64, 1), (65, 1), (128, 1), (129, 1), (3, 43), (16, 8), (1, 256),
                (8, 256))
DEPTH_BORDERS = ((1, 1), (1, 63), (63, 1), (1, 64), (2, 32), (2, 64), (64, 1), (1, 65), (2, 65), (65, 1), (5, 13),
                 (127, 1), (128, 1), (129, 1), (3, 43), (16, 8), (1, 255), (1, 256), (8, 256))

FAMILIES = ("depth", "short", "values", "wide", "layouts")


def path_of(world: int, k: int) -> str:
    """The branch of shard_merge_kernel a channel takes (shard.hip), whichever launch holds it: the staged launch still
    ranks a channel with world * k <= 128 and k <= 64 in registers."""
    total = world * k
    if total > 128 or k > 64:
        return "staged"
    return "two_halves" if total > 64 else "one_sort"


def fmax(dtype):
    return FLT_MAX if dtype == F32 else DBL_MAX


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def ord64(x) -> np.ndarray:
    """topk.hpp ord64: order-preserving key of an fp64 score; -0.0 == +0.0, NaN -> 1, nothing maps to 0 (padding)."""
    x = np.asarray(x, np.float64) + 0.0
    u = np.ascontiguousarray(x).view(np.uint64)
    key = np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))
    return np.where(np.isnan(x), np.uint64(1), key)


def channel_order(s, i):
    """(score descending, id ascending), NaN last, the two zeros equal: the order every channel returns."""
    return np.lexsort((i, -np.asarray(s, np.float64)))


@dataclass
class Case:
    name: str
    family: str
    world: int
    nq: int
    chans: List[Tuple[int, type]]        # (k, dtype) per channel
    offsets: List[int]                    # id offset per rank
    lists: list                           # lists[r][c] = (scores [nq, k] dtype, LOCAL ids [nq, k] int64)
    rogue: bool = False

    @property
    def ks(self):
        return [k for k, _ in self.chans]

    @property
    def staged_launch(self) -> bool:
        return any(path_of(self.world, k) == "staged" for k in self.ks)

    def global_ids(self, r: int, c: int) -> np.ndarray:
        i = self.lists[r][c][1]
        return np.where(i >= 0, i + np.int64(self.offsets[r]), i)

    def n_valid(self, c: int) -> np.ndarray:
        """valid candidates per query over all ranks"""
        return sum((self.lists[r][c][1] >= 0).sum(axis=1) for r in range(self.world))


def reference(case: Case, c: int):
    """(scores fp64 [nq, k], global ids [nq, k]) of channel c: oracle.dense.merge_topk in fp64; -inf / -1 padding."""
    from oracle import dense as OD
    k = case.chans[c][0]
    sp = [case.lists[r][c][0].astype(np.float64) for r in range(case.world)]
    ip = [case.global_ids(r, c) for r in range(case.world)]
    return OD.merge_topk(sp, ip, k)


def kernel_view(es64, ei, dtype):
    """The reference as the kernel returns it (the three documented differences): (scores of `dtype`, NaN mask).  Score
    bits are compared wherever the mask is False; where it is True the kernel's score must be a NaN."""
    hit = ei >= 0
    with np.errstate(over="ignore"):
        s = es64.astype(dtype)  # exact: every score of an fp32 channel was an fp32
    s = np.where(s == 0, dtype(0.0), s)
    s = np.where(hit, s, -fmax(dtype)).astype(dtype)
    return s, np.isnan(es64) & hit


def edge_counts(case: Case, c: int, es64, got_s, got_i) -> dict:
    """What a RESULT (got_s, got_i) of channel c holds of the edges; es64 = the reference's scores, for the sign of a zero
    (the kernel returns +0.0 for both)."""
    k, dtype = case.chans[c]
    hit = got_i >= 0
    adj = hit[:, :-1] & hit[:, 1:]
    lo, hi = got_i[:, :-1], got_i[:, 1:]
    same = adj & ((got_s[:, :-1] == got_s[:, 1:]) | (np.isnan(got_s[:, :-1]) & np.isnan(got_s[:, 1:])))
    zero2 = adj & (es64[:, :-1] == 0) & (es64[:, 1:] == 0) & (np.signbit(es64[:, :-1]) != np.signbit(es64[:, 1:]))
    low = np.int64(0xFFFFFFFF)
    nhit = hit.sum(axis=1)
    with np.errstate(invalid="ignore"):
        sub = hit & (got_s != 0) & (np.abs(got_s) < np.finfo(dtype).tiny)
    return {
        "nan_hit": int((np.isnan(got_s) & hit).sum()),
        "zero_pair_in_id_order": int((zero2 & (lo < hi)).sum()),
        "pad_valued_hit": int((hit & (got_s == -fmax(dtype))).sum()),
        "inf_hit": int((hit & np.isinf(got_s)).sum()),
        "subnormal_hit": int(sub.sum()),
        "id_ge_2_32": int((got_i >= (1 << 32)).sum()),
        "tie_high_word_only": int((same & ((lo & low) == (hi & low)) & (lo < hi)).sum()),
        "tie_low_words_reversed": int((same & ((lo & low) > (hi & low)) & (lo < hi)).sum()),
        "tie": int(same.sum()),
        "row_short": int(((nhit > 0) & (nhit < k)).sum()),
        "row_empty": int((nhit == 0).sum()),
        "row_exactly_k": int(((nhit == k) & (case.n_valid(c) == k)).sum()),
        "row_k_plus_1": int((case.n_valid(c) == k + 1).sum()),
    }


def add_counts(total: dict, more: dict) -> dict:
    for key, v in more.items():
        total[key] = total.get(key, 0) + v
    return total


def lists_are_channel_shaped(case: Case) -> bool:
    """Every list: valid entries first, sorted by (ord64 key descending, id ascending); ids < 0 behind them only."""
    for r in range(case.world):
        for c, (k, dtype) in enumerate(case.chans):
            s, i = case.lists[r][c]
            if s.shape != (case.nq, k) or i.shape != (case.nq, k) or s.dtype != dtype or i.dtype != np.int64:
                return False
            for q in range(case.nq):
                n = int((i[q] >= 0).sum())
                if np.any(i[q, :n] < 0):
                    return False
                key = ord64(s[q, :n])
                for j in range(n - 1):
                    if key[j] < key[j + 1] or (key[j] == key[j + 1] and i[q, j] >= i[q, j + 1]):
                        return False
    return True


# ---------------------------------------------------------------------------------------------------------------------
# building blocks

class _Draft:
    """One channel of a case while it is put together: s / i [world, nq, k] in any order, cnt [world, nq] valid entries."""

    def __init__(self, world, nq, k, dtype, n_rows=N_ROWS):
        self.world, self.nq, self.k, self.dtype = world, nq, k, dtype
        self.n_rows = max(n_rows, 2 * k)
        self.s = np.zeros((world, nq, k), dtype=dtype)
        self.i = np.zeros((world, nq, k), dtype=np.int64)
        self.cnt = np.zeros((world, nq), dtype=np.int64)

    def fill(self, rng, q, cnt, ties=False):
        """cnt[r] entries on rank r for query q: distinct local ids, scores normal or from FIVE"""
        for r in range(self.world):
            c = int(cnt[r])
            self.cnt[r, q] = c
            self.i[r, q, :c] = rng.choice(self.n_rows, size=c, replace=False)
            self.s[r, q, :c] = (rng.choice(np.asarray(FIVE, self.dtype), size=c) if ties
                                else rng.standard_normal(c).astype(self.dtype))

    def put(self, rng, q, entries):
        """entries: (rank, score) appended to query q with a fresh local id"""
        for r, v in entries:
            c = int(self.cnt[r, q])
            assert c < self.k
            free = np.setdiff1d(np.arange(self.n_rows), self.i[r, q, :c])
            self.i[r, q, c] = rng.choice(free)
            self.s[r, q, c] = v
            self.cnt[r, q] = c + 1

    def copy_base(self, rng, q, cnt, ties):
        """the SAME sorted list (local ids and scores) on every rank, rank r keeping its first cnt[r] entries"""
        i = rng.choice(self.n_rows, size=self.k, replace=False).astype(np.int64)
        s = (rng.choice(np.asarray(FIVE, self.dtype), size=self.k) if ties
             else np.round(rng.standard_normal(self.k), 1).astype(self.dtype))
        o = channel_order(s, i)
        for r in range(self.world):
            self.cnt[r, q] = int(cnt[r])
            self.i[r, q], self.s[r, q] = i[o], s[o]

    def finish(self, rng, rogue):
        out = []
        for r in range(self.world):
            s, i = self.s[r].copy(), self.i[r].copy()
            for q in range(self.nq):
                c = int(self.cnt[r, q])
                o = channel_order(s[q, :c], i[q, :c])
                s[q, :c], i[q, :c] = s[q, :c][o], i[q, :c][o]
                s[q, c:] = ROGUE_SCORE if rogue else -fmax(self.dtype)
                i[q, c:] = rng.choice(ROGUE_IDS, size=self.k - c) if rogue else -1
            out.append((s, i))
        return out


def _case(name, family, world, nq, chans, offsets, drafts, rng, rogue):
    per_chan = [d.finish(rng, rogue) for d in drafts]
    lists = [[per_chan[c][r] for c in range(len(chans))] for r in range(world)]
    return Case(name, family, world, nq, list(chans), [int(o) for o in offsets], lists, rogue)


def _random_counts(rng, world, k):
    return np.where(rng.random(world) < 0.5, k, rng.integers(0, k + 1, size=world))


def _spread_long(total, world, k, start):
    """as few ranks as possible: full lists rank after rank from `start`"""
    cnt = np.zeros(world, dtype=np.int64)
    r = start % world
    while total > 0:
        cnt[r] = min(k, total)
        total -= cnt[r]
        r = (r + 1) % world
    return cnt


def _spread_thin(total, world, k):
    """as many ranks as possible: one entry each, then a second"""
    assert total <= min(2, k) * world, (total, world, k)
    cnt = np.zeros(world, dtype=np.int64)
    for j in range(total):
        cnt[j % world] += 1
    return cnt


def _spread_even(total, world):
    cnt = np.full(world, total // world, dtype=np.int64)
    cnt[:total % world] += 1
    return cnt


def _plain_offsets(world, n_rows):
    return [r * n_rows for r in range(world)]


# ---------------------------------------------------------------------------------------------------------------------
# the families

def depth_cases():
    """world * k and k at the borders of the kernel's conditions; an fp32 and an fp64 channel of the same depth."""
    out = []
    for n, (world, k) in enumerate(DEPTH_BORDERS):
        rng = np.random.default_rng(10_000 + 1000 * world + k)
        nq, ties, rogue = 5, n % 2 == 1, n % 3 == 0
        drafts = []
        for dtype in (F32, F64):
            d = _Draft(world, nq, k, dtype)
            d.fill(rng, 0, np.full(world, k), ties)          # every lane / slot holds a candidate
            d.fill(rng, 1, _random_counts(rng, world, k), ties)
            d.fill(rng, 2, _random_counts(rng, world, k), not ties)
            d.fill(rng, 3, _spread_long(k, world, k, n), ties)  # exactly k, from one rank
            d.fill(rng, 4, np.full(world, k), True)
            drafts.append(d)
        out.append(_case(f"depth-w{world}-k{k}", "depth", world, nq, [(k, F32), (k, F64)],
                         _plain_offsets(world, drafts[0].n_rows), drafts, rng, rogue))
    return out


SHORT_CONFIGS = ((6, 10), (12, 10), (16, 8), (40, 10), (40, 70))


def short_totals(world, k):
    t = [0, 1, k - 1, k, k + 1]
    if path_of(world, k) == "staged":
        t += [63, 64, 65]  # either side of one push of 64 lanes
    return t


def short_cases():
    """per query the valid candidates over all ranks number 0, 1, k-1, k, k+1 (staged: also 63, 64, 65): once from as few
    ranks as possible, once from ranks that hold one or two entries each."""
    out = []
    for n, (world, k) in enumerate(SHORT_CONFIGS):
        rng = np.random.default_rng(20_000 + 1000 * world + k)
        totals = short_totals(world, k)
        nq = 2 * len(totals)
        drafts = []
        for dtype in (F32, F64):
            d = _Draft(world, nq, k, dtype)
            for j, t in enumerate(totals):
                d.fill(rng, 2 * j, _spread_long(t, world, k, 3 * j + 1), ties=False)
                d.fill(rng, 2 * j + 1, _spread_thin(t, world, k), ties=n % 2 == 1)
            drafts.append(d)
        out.append(_case(f"short-w{world}-k{k}", "short", world, nq, [(k, F32), (k, F64)],
                         _plain_offsets(world, drafts[0].n_rows), drafts, rng, rogue=n % 2 == 0))
    return out


VALUE_CONFIGS = ((4, 10), (8, 12), (20, 10), (8, 80))


def _deal(rng, world, n, skip=()):
    """n ranks, round robin from a random start, never one of `skip`"""
    ranks = [r for r in range(world) if r not in skip] or list(range(world))
    start = int(rng.integers(len(ranks)))
    return [ranks[(start + j) % len(ranks)] for j in range(n)]


def value_cases():
    """Eight queries, one value edge each (pairs on DIFFERENT ranks), with so few candidates that the edge is in the
    result:  0 two NaNs (the canonical payload, another) | 1 -0.0 on the lower id, +0.0 on the higher | 2 the reverse |
    3 +inf and -inf | 4 a valid hit scoring the padding value | 5 subnormals of both signs around a zero | 6 five values,
    every rank full | 7 exactly k candidates: five values, a NaN, a zero pair, the padding value."""
    out = []
    for n, (world, k) in enumerate(VALUE_CONFIGS):
        rng = np.random.default_rng(30_000 + 1000 * world + k)
        nq, last = 8, world - 1
        drafts = []
        for dtype in (F32, F64):
            nan, other = (NAN32, OTHER_NAN32) if dtype == F32 else (NAN64, OTHER_NAN64)
            tiny = np.finfo(dtype).smallest_subnormal
            big = np.finfo(dtype).tiny * dtype(0.25)  # a subnormal with several mantissa bits left
            d = _Draft(world, nq, k, dtype)

            def normals(q, count, sign=0, skip=()):
                v = np.abs(rng.standard_normal(count)).astype(dtype) + dtype(0.5)
                if sign == 0:
                    v = v * rng.choice(np.asarray([-1, 1], dtype), size=count)
                d.put(rng, q, list(zip(_deal(rng, world, count, skip), v * dtype(sign or 1))))

            normals(0, k - 3)
            d.put(rng, 0, [(0, nan), (1 % world, other)])
            for q, (a, b) in ((1, (-0.0, 0.0)), (2, (0.0, -0.0))):
                normals(q, k // 2 - 1, +1)
                normals(q, k - k // 2 + 2, -1)
                d.put(rng, q, [(0, dtype(a)), (last, dtype(b))])
            normals(3, k - 3)
            d.put(rng, 3, [(0, dtype(np.inf)), (last, dtype(-np.inf))])
            normals(4, k - 3)
            d.put(rng, 4, [(last, -fmax(dtype))])
            normals(5, 2, +1)
            normals(5, k - 5, -1)
            d.put(rng, 5, list(zip(_deal(rng, world, 5), [tiny, -tiny, big, -big, dtype(0.0)])))
            d.fill(rng, 6, np.full(world, k), ties=True)
            d.fill(rng, 7, _spread_even(k - 4, world), ties=True)
            d.put(rng, 7, [(0, dtype(-0.0)), (last, dtype(0.0)), (1 % world, nan), (last, -fmax(dtype))])
            drafts.append(d)
        out.append(_case(f"values-w{world}-k{k}", "values", world, nq, [(k, F32), (k, F64)],
                         _plain_offsets(world, drafts[0].n_rows), drafts, rng, rogue=n % 2 == 1))
    return out


WIDE_CONFIGS = ((4, 10), (8, 12), (3, 43), (8, 80))


def wide_offsets(variant, world, n_rows, rng):
    if variant == "high":        # only the high word differs between the copies of a candidate
        return [r << 32 for r in range(world)]
    if variant == "high_rev":    # ... and the low words order them the other way round
        return [(r << 32) + (world - 1 - r) * 1000 for r in range(world)]
    if variant == "high_perm":   # ranks not in id order
        return [(int(p) << 32) + 7 for p in rng.permutation(world) + 1]
    if variant == "at_2_40":
        return [(1 << 40) + r * n_rows for r in range(world)]
    if variant == "across_2_32":  # a block that straddles the word boundary: the carry of local id + offset
        return [(1 << 32) - n_rows // 2 + r * n_rows for r in range(world)]
    raise ValueError(variant)


WIDE_VARIANTS = ("high", "high_rev", "high_perm", "at_2_40", "across_2_32")


def wide_cases():
    """Offsets above 2^32.  Queries 0 and 1 carry the SAME local list (ids and scores) on every rank — in full, and cut to
    a different length per rank — so that each candidate meets world - 1 others of its score and its low id word; 2 and 3
    are independent lists."""
    out = []
    for n, (world, k) in enumerate(WIDE_CONFIGS):
        for m, variant in enumerate(WIDE_VARIANTS):
            rng = np.random.default_rng(40_000 + 1000 * world + 10 * k + m)
            nq = 4
            drafts = []
            for dtype in (F32, F64):
                d = _Draft(world, nq, k, dtype)
                d.copy_base(rng, 0, np.full(world, k), ties=True)
                d.copy_base(rng, 1, rng.integers(1, k + 1, size=world), ties=False)
                d.fill(rng, 2, _random_counts(rng, world, k), ties=True)
                d.fill(rng, 3, _spread_thin(min(k + 1, world), world, k), ties=False)
                drafts.append(d)
            out.append(_case(f"wide-{variant}-w{world}-k{k}", "wide", world, nq, [(k, F32), (k, F64)],
                             wide_offsets(variant, world, drafts[0].n_rows, rng), drafts, rng, rogue=(n + m) % 4 == 0))
    return out


LAYOUTS = (
    (4, ((10, F32),)),
    (4, ((10, F32), (80, F64))),                     # register path inside the staged launch, shallow first
    (4, ((80, F64), (10, F32))),                     # ... deep first
    (3, ((7, F64), (64, F32), (40, F64))),           # one_sort, staged (192), two_halves (120)
    (3, ((3, F32), (65, F64), (16, F32), (256, F64))),
)
LAYOUT_NQ = (1, 2, 3, 5, 53)


def layout_cases():
    """1-4 channels of mixed dtype and depth x nq: nq * channels leaves 1, 2, 3 and 0 waves in the last block of four."""
    out = []
    for n, (world, chans) in enumerate(LAYOUTS):
        for nq in LAYOUT_NQ:
            rng = np.random.default_rng(50_000 + 100 * n + nq)
            drafts = []
            for k, dtype in chans:
                d = _Draft(world, nq, k, dtype)
                for q in range(nq):
                    d.fill(rng, q, _random_counts(rng, world, k), ties=(q + n) % 2 == 0)
                drafts.append(d)
            n_rows = max(d.n_rows for d in drafts)
            out.append(_case(f"layout{n}-nq{nq}", "layouts", world, nq, chans, _plain_offsets(world, n_rows), drafts, rng,
                             rogue=(n + nq) % 3 == 0))
    return out


_BUILDERS = {"depth": depth_cases, "short": short_cases, "values": value_cases, "wide": wide_cases,
             "layouts": layout_cases}
_CACHE = {}


def cases(family: str) -> List[Case]:
    """The cases of a family, built once per process and never changed."""
    if family not in _CACHE:
        _CACHE[family] = _BUILDERS[family]()
    return _CACHE[family]


def all_cases() -> List[Case]:
    return [c for f in FAMILIES for c in cases(f)]


_REF = {}


def reference_cached(case: Case, c: int):
    key = (case.name, c)
    if key not in _REF:
        es, ei = reference(case, c)
        es.setflags(write=False)
        ei.setflags(write=False)
        _REF[key] = (es, ei)
    return _REF[key]

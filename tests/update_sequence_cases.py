"""Long mixed add / remove / replace sequences on the resident stores (tests/test_update_sequence*.py; numpy only).

Every update has a module of its own that starts from a fresh handle and applies one operation.  A handle that is edited
for days is a state machine: capacity against rows, the fp16 image's rows and scale, statistics that an add folds into
and a remove or replace takes again from zero, a lazily made short-corpus image, what the fp16 first pass learnt.  Here a
plain host MODEL of each store runs a seeded SCRIPT of updates; the GPU tests apply the same script to one live handle and
compare it, after every step, with the model's bytes, with an exact reference computed from the model alone, and with a
fresh handle of the model's bytes.  Nothing in this module calls the library.

Kinds of steps: A-in (add inside the capacity), A-grow (add that reallocates), Rm, Rp, X (an update the host refuses
before anything is enqueued; every check of the previous state must still hold), B (build_image: no update; dense).

Dense data (exact by construction): background rows in {-1, 0, 1}, queries in {-3 .. 3} with no zero in query 0 and none
in column 0 of any query, so max|Q| sum|x| <= 3 * 24 * d < 2^24 even for the "large" rows of components +-24 (which raise
the power-of-two scale by three steps): every fp32 score is an exact integer in any order.  Planted rows:
  ties    3 sign(Q[t]) for a query t >= 1: all planted rows of one query tie exactly, so the lower id must win across
          every seam an update makes;
  ladder  for query 0 a family of rows with strictly increasing scores, all above every background score: 3 sign(Q[0])
          on the first m columns (d = 128: m = 64 .. 128), the rows of {-3 .. 3}^4 by score (d = 4).  Every add plants the
          next ladder row above query 0's current best, every remove takes query 0's best row out, every replace
          overwrites it with a background row: query 0's top-1 — hence the expected list of EVERY checked (nq, k), which
          all hold query 0 — changes at every update (certificate: every_step_matters).
A NaN row (one NaN component) never enters a list: the kernels' maxima drop it, the reference ranks its scores as -inf
and the scripts keep k below the finite rows.  An infinite component sits in column 0, where no query is zero: the row
scores +inf or -inf, never NaN, in the reference as on the device.

The dense model also predicts what amdr_dense_image_info shows (csrc/dense.hip amdr_dense_add / _remove / _replace):
  build_image   present (needs rows and finite statistics);
  add           the statistics FOLD the new rows in; a present image follows (rows = n, the scale of the folded
                maximum) while they are finite, else it is dropped;
  remove        the statistics from zero; a present image is made again unless no row is left or they are not finite;
  replace       the statistics from zero; a present image follows while they are finite, else it is dropped;
  nothing but build_image brings a dropped image back.
Finite: the largest |component| (NaN components dropped) <= FLT_MAX.  The scale exponent is frexp's of that maximum.
The capacity: create n; a growing add max(2 cap, n); remove n.  (So Rm -> A-in cannot occur on a dense handle.)"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import dense_adversary as DA

FLT_MAX = DA.FLT_MAX
KINDS = ("A-in", "A-grow", "Rm", "Rp")
NQ_ALL = 64
DENSE_NQS = (1, 4, 9, 33, 64)
DENSE_KS = (1, 10, 32)
HI_K = 10
HI_NQS = (9, 33, 64)
HI_KC0 = HI_K + 22 + 1           # hi_kc(10, 0): tiles re-scored per query at width level 0 (kHiExtra[0] = 22)
HI_KC_MAX = HI_K + 96 + 1        # hi_kc_max(10)
HI_MIN_ROWS = (2 * HI_KC_MAX - 1) * 32 + 1  # 214 tiles: the first n with tiles >= 2 kc_max under AMDR_DENSE_HI=1
HI_PINS = {"AMDR_DENSE_HI": "1", "AMDR_DENSE_TWO_LEVEL": "1"}
SHORT_PINS = {"AMDR_DENSE_SMALL_HI": "1", "AMDR_DENSE_TWO_LEVEL": "0", "AMDR_DENSE_SMALL_HI_MIN": "64"}
SHORT_MAX, ROW_WAVES_MAX = 1024, DA.ROW_WAVES_MAX
X_KINDS = ("remove id == n", "replace duplicate id", "remove negative id", "replace descending ids")


# ---- the dense model --------------------------------------------------------------------------------------------------
def amax_of(X):
    """The largest |component|, NaN components dropped (dense_stats_kernel's word 0)."""
    if X.size == 0:
        return 0.0
    a = np.abs(X.astype(np.float64))
    a = a[~np.isnan(a)]
    return float(a.max()) if a.size else 0.0


def finite_amax(amax):
    e = int(np.frexp(np.float32(amax))[1]) if 0.0 < amax <= FLT_MAX else 0
    return amax <= FLT_MAX and -100 < e < 100


def scale_exp(amax):
    return int(np.frexp(np.float32(amax))[1]) if 0.0 < amax <= FLT_MAX else 0


class DenseModel:
    """A float32 matrix with add / remove / replace, and the visible derived state of the handle."""

    def __init__(self, X):
        self.X = np.ascontiguousarray(X, dtype=np.float32).copy()
        self.d = self.X.shape[1]
        self.cap = self.n
        self.amax = amax_of(self.X)  # the statistics word as the handle holds it (folded by adds)
        self.image = False

    @property
    def n(self):
        return self.X.shape[0]

    def will_grow(self, n_add):
        return self.n + n_add > self.cap

    def add(self, R):
        R = np.asarray(R, np.float32).reshape(-1, self.d)
        n_new = self.n + R.shape[0]
        if n_new > self.cap:
            self.cap = max(2 * self.cap, n_new)
        self.amax = max(self.amax, amax_of(R)) if self.n else amax_of(R)
        self.X = np.concatenate([self.X, R])
        if self.image and not finite_amax(self.amax):
            self.image = False

    def remove(self, ids):
        keep = np.ones(self.n, bool)
        keep[np.asarray(ids, np.int64)] = False
        self.X = np.ascontiguousarray(self.X[keep])
        self.cap = self.n
        self.amax = amax_of(self.X)
        if self.image and (self.n == 0 or not finite_amax(self.amax)):
            self.image = False

    def replace(self, ids, R):
        self.X[np.asarray(ids, np.int64)] = np.asarray(R, np.float32).reshape(-1, self.d)
        self.amax = amax_of(self.X)
        if self.image and not finite_amax(self.amax):
            self.image = False

    def build_image(self):
        assert self.n > 0 and finite_amax(self.amax) and self.d % 128 == 0
        self.image = True

    def image_state(self):
        """(present, rows covered, e of the scale 2^-e): amdr_dense_image_info words 0, 2, 3."""
        return (True, self.n, scale_exp(self.amax)) if self.image else (False, 0, 0)

    def stats_finite(self):
        return finite_amax(self.amax)


class State:
    """The model after one step.  op: what the live handle is given — ('create', X) | ('build',) | ('add', R) |
    ('remove', ids) | ('replace', ids, R) | ('refused', call, args...)."""

    def __init__(self, step, kind, op, m, seam, note, planted):
        self.step, self.kind, self.op, self.note = step, kind, op, note
        self.X = m.X.copy()
        self.n, self.d, self.cap = m.n, m.d, m.cap
        self.image = m.image_state()
        self.finite = m.stats_finite()
        self.seam = [int(r) for r in seam]
        self.planted = dict(planted)  # {query: new / replaced-in planted row ids of this step}

    @property
    def finite_rows(self):
        return np.nonzero(np.all(np.isfinite(self.X), axis=1))[0]

    @property
    def nan_rows(self):
        return np.nonzero(np.any(np.isnan(self.X), axis=1))[0]


def rank_scores(X, Q):
    """fp64 scores [nq, n] for ranking: a NaN score (a row that holds a NaN) ranks as -inf; it never enters a list."""
    with np.errstate(invalid="ignore"):
        S = DA.exact_scores(X, Q)
    return np.where(np.isnan(S), -np.inf, S)


@functools.lru_cache(maxsize=None)
def _expected(profile, step, k):
    st = dense_states(profile)[step]
    return DA.oracle_topk(rank_scores(st.X, dense_queries(profile)), k)


def expected_topk(profile, step, nq, k, k_max=max(DENSE_KS)):
    """(scores f32, ids) of the first nq queries at depth k <= k_max: the prefix of the one list computed per state."""
    es, ei = _expected(profile, step, k_max)
    return es[:nq, :k], ei[:nq, :k]


def scoped_expected(X, Q, rows, k):
    """Top-k of each query over `rows` alone, with their own ids."""
    rows = np.asarray(rows, np.int64)
    es, ei = DA.oracle_topk(rank_scores(X[rows], Q), k)
    return es, np.where(ei >= 0, rows[np.maximum(ei, 0)], -1)


# ---- data -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_queries(profile):
    d = PROFILES[profile]["d"]
    rng = np.random.default_rng(PROFILES[profile]["seed"])
    Q = rng.integers(-3, 4, size=(NQ_ALL, d)).astype(np.float32)
    Q[:, 0] = np.where(Q[:, 0] == 0, 2, Q[:, 0])  # an infinite component (column 0) never meets a zero
    nz = rng.integers(1, 4, size=d) * rng.choice([-1, 1], size=d)
    Q[0] = np.where(Q[0] == 0, nz, Q[0])
    Q[0, 0] = -abs(Q[0, 0])  # the infinite row (+inf in column 0) scores -inf for query 0: the ladder still decides it
    if d == 4:
        Q[0], Q[1], Q[2] = (3, -2, 1, -3), (-1, 3, -2, 2), (2, 1, -3, 1)
        Q[0, 0] = -3
    return Q


@functools.lru_cache(maxsize=None)
def ladder(profile):
    """Rows with strictly increasing scores for query 0, the lowest above the largest score a background row can reach
    (sum |Q[0]|): [L, d] float32."""
    q = dense_queries(profile)[0].astype(np.float64)
    d = q.size
    bg_max = float(np.abs(q).sum())
    if d == 4:
        allr = np.array(list(itertools.product(range(-3, 4), repeat=4)), dtype=np.float32)
        s = allr.astype(np.float64) @ q
        rows, seen = [], set()
        for i in np.argsort(s, kind="stable"):
            if s[i] > bg_max and s[i] not in seen:
                seen.add(float(s[i]))
                rows.append(allr[i])
        return np.array(rows, dtype=np.float32)
    rows = []
    for m in range(d // 2, d + 1):
        r = np.zeros(d, np.float32)
        r[:m] = 3 * np.sign(q[:m])
        rows.append(r)
    L = np.array(rows, dtype=np.float32)
    s = L.astype(np.float64) @ q
    assert s[0] > bg_max and np.all(np.diff(s) > 0)
    return L


def tie_row(Q, t):
    return (3 * np.sign(Q[t])).astype(np.float32)


class _Builder:
    def __init__(self, profile):
        p = PROFILES[profile]
        self.profile, self.p = profile, p
        self.rng = np.random.default_rng(p["seed"] + 1)
        self.Q = dense_queries(profile)
        self.lad = ladder(profile)
        self.lad_s = self.lad.astype(np.float64) @ self.Q[0].astype(np.float64)
        d, n0 = p["d"], p["n0"]
        X = self.background(n0)
        # the initial planting: per query t >= 1 `ties0` tie rows, for query 0 the first `ladder0` ladder rows
        spots = self.rng.permutation(n0)
        at = 0
        for lv in range(p["ladder0"]):
            X[spots[at]] = self.lad[lv]
            at += 1
        # queries that take tie rows: those whose tie row stays below query 0's ladder (all of them at d = 128)
        q0 = self.Q[0].astype(np.float64)
        self.tq_ok = [t for t in range(1, NQ_ALL) if float(tie_row(self.Q, t) @ q0) <= float(np.abs(q0).sum())]
        assert len(self.tq_ok) >= 2
        for t in self.tq_ok:
            for _ in range(p["ties0"]):
                X[spots[at]] = tie_row(self.Q, t)
                at += 1
        assert at <= n0
        self.m = DenseModel(X)
        self.states = [State(0, "create", ("create", X.copy()), self.m, [0, n0 - 1], "create", {})]
        self.turn = 0

    def background(self, n):
        return self.rng.integers(-1, 2, size=(n, self.p["d"])).astype(np.float32)

    def best0(self):
        """(row id, score) of query 0's best finite-score row."""
        s = rank_scores(self.m.X, self.Q[:1])[0]
        s = np.where(np.isposinf(s), -np.inf, s)
        i = int(np.lexsort((np.arange(s.size), -s))[0])
        return i, float(s[i])

    def next_ladder(self, large=False):
        top = self.best0()[1] if self.m.n else -np.inf
        f = 8.0 if large else 1.0
        ok = np.nonzero(self.lad_s * f > top)[0]
        assert ok.size, "the ladder is used up: the script needs a remove or a replace of query 0's best rows first"
        return (self.lad[ok[0]] * np.float32(f)).astype(np.float32)

    def tie_queries(self, count):
        out = [self.tq_ok[(self.turn * count + j) % len(self.tq_ok)] for j in range(count)]
        self.turn += 1
        return out

    def push(self, kind, op, seam, note, planted=()):
        n = self.m.n
        seam = sorted({min(max(int(r), 0), n - 1) for r in seam}) if n else []
        self.states.append(State(len(self.states), kind, op, self.m, seam, note, planted))

    # -- the steps
    def build(self):
        self.m.build_image()
        self.push("B", ("build",), [0, self.m.n - 1], "build_image")

    def add(self, count, large=False, nan=False, inf=False, ties=2):
        ties = min(ties, count - 1 - int(nan) - int(inf))
        assert ties >= 0
        R = self.background(count)
        slots = list(self.rng.permutation(count))
        row0 = self.m.n
        if self.p["hi"]:
            # the ladder row goes into a tile that holds no row above the background for query 0 yet, so that an image of
            # the OLD matrix ranks that tile below the candidate cut (test_update_sequence's stale-maxima certificate)
            T = tile_maxima(self.m.X, self.Q[:1])[0]
            cold = [j for j in slots if (row0 + j) // 32 >= T.size or T[(row0 + j) // 32] <= float(np.abs(self.Q[0]).sum())]
            assert cold, "every tile this add reaches holds a ladder row already"
            slots.remove(min(cold))
            slots.insert(0, min(cold))
        planted = {0: [row0 + int(slots[0])]}
        R[slots.pop(0)] = self.next_ladder(large)
        for t in self.tie_queries(ties):
            planted.setdefault(t, []).append(row0 + int(slots[0]))
            R[slots.pop(0)] = tie_row(self.Q, t)
        if nan:
            R[slots.pop(0), 5 % self.p["d"]] = np.nan
        if inf:
            R[slots.pop(0), 0] = np.inf
        kind = "A-grow" if self.m.will_grow(count) else "A-in"
        self.m.add(R)
        note = f"add {count}" + (" large" if large else "") + (" NaN" if nan else "") + (" inf" if inf else "")
        self.push(kind, ("add", R), [row0 - 2, row0 - 1, row0, row0 + 1, self.m.n - 1, 0], note, planted)

    def remove(self, to=None, every=None, large=False, everything=False):
        n = self.m.n
        if everything:
            ids = np.arange(n)
        else:
            must = {self.best0()[0]}
            if large:
                must |= set(np.nonzero(np.nanmax(np.abs(self.m.X), axis=1) > 3)[0].tolist())
            if every:
                must |= set(range(every - 1, n, every))
            more = max(0, (n - to) - len(must)) if to is not None else 0
            pool = np.setdiff1d(np.arange(n), np.fromiter(must, np.int64))
            ids = np.sort(np.concatenate([np.fromiter(must, np.int64), self.rng.choice(pool, size=more, replace=False)]))
            assert to is None or n - ids.size == to, (n, ids.size, to)
        first = int(ids[0])
        self.m.remove(ids)
        note = "remove everything" if everything else f"remove {ids.size}" + (" large" if large else "")
        self.push("Rm", ("remove", ids.astype(np.int64)), [first - 2, first - 1, first, first + 1, 0, self.m.n - 1], note)

    def replace(self, at=(), large=False, unlarge=False, clean=False, ties=2):
        """at: row ids (negative: from the end) that take tie rows; query 0's best row always takes a background row."""
        n = self.m.n
        best = self.best0()[0]
        new = {best: self.background(1)[0]}
        planted = {}
        if unlarge:
            for r in np.nonzero(np.nanmax(np.abs(self.m.X), axis=1) > 3)[0]:
                new[int(r)] = self.background(1)[0]
        if clean:
            for r in np.nonzero(~np.all(np.isfinite(self.m.X), axis=1))[0]:
                new[int(r)] = self.background(1)[0]
        tq = self.tie_queries(max(ties, 1))
        for j, r in enumerate(at):
            r = int(r) % n
            if r == best:
                r = (r - 1) % n
            if j == 0 and not large:
                # the first listed row takes query 0's next ladder row (above what is left without the old best): the new
                # best row of a query enters from the listed tile, whatever an image of the old matrix says about it
                self.m.X[best] = new[best]
                new[r] = self.next_ladder()
                planted[0] = [r]
                continue
            t = tq[j % len(tq)]
            new[r] = tie_row(self.Q, t)
            planted.setdefault(t, []).append(r)
        ids = np.array(sorted(new), dtype=np.int64)
        R = np.array([new[int(i)] for i in ids], dtype=np.float32)
        if large:  # the row that takes the large ladder row: not query 0's old best, so both changes are in one call
            r = next(int(i) for i in ids[::-1] if int(i) != best)
            self.m.X[best] = new[best]  # (the ladder is taken against the matrix without the old best)
            R[list(ids).index(r)] = self.next_ladder(True)
            planted = {t: [i for i in rows if i != r] for t, rows in planted.items()}
            planted[0] = [r]
        self.m.replace(ids, R)
        note = f"replace {ids.size} from row {int(ids[0])}" + (" large" if large else "") + (" large out" if unlarge else "") + \
               (" non-finite out" if clean else "")
        self.push("Rp", ("replace", ids, R), [ids[0] - 1, ids[0], ids[0] + 1, ids[-1] - 1, ids[-1], ids[-1] + 1, 0, n - 1],
                  note, planted)

    def refused(self, which):
        n, d = self.m.n, self.p["d"]
        R2 = self.background(2)
        op = {"remove id == n": ("refused", "remove", np.array([0, n], np.int64)),
              "replace duplicate id": ("refused", "replace", np.array([3, 3], np.int64), R2),
              "remove negative id": ("refused", "remove", np.array([-1, 2], np.int64)),
              "replace descending ids": ("refused", "replace", np.array([5, 2], np.int64), R2)}[which]
        prev = self.states[-1]
        self.states.append(State(len(self.states), "X", op, self.m, prev.seam, f"refused: {which}", {}))


def _script_tiles(b):
    b.build()                                   # 70 / 70, image
    b.add(1)                                    # A-grow 71 / 140
    b.refused(X_KINDS[0])
    b.add(70)                                   # A-grow 141 / 280 (A-grow -> A-grow; across 96 and 128)
    b.add(19)                                   # A-in 160: img_rows on a tile edge
    b.refused(X_KINDS[1])
    b.add(3)                                    # A-in 163: img_rows mid-tile (A-in -> A-in; across 160)
    b.replace(at=(45, 131, 159))                # first id mid-tile, right after an A-in that left img_rows mid-tile
    b.refused(X_KINDS[2])
    b.add(5, large=True)                        # A-in 168: the scale rises by three steps
    b.remove(to=159, large=True)                # the scale falls; across 160 from above; cap == n
    b.refused(X_KINDS[3])
    b.add(3)                                    # A-grow 162 / 318 (Rm -> A-grow; across 160)
    b.replace(at=(0, 100, -1), large=True)      # A-grow -> Rp; the scale rises by a replace
    b.replace(at=(31, 32), unlarge=True)        # Rp -> Rp; the scale falls by a replace
    b.remove(to=127)                            # Rp -> Rm; across 128 from above
    b.remove(to=95)                             # Rm -> Rm; across 96 from above
    b.add(3)                                    # A-grow 98 / 190; across 96
    b.add(3)                                    # A-in 101 (A-grow -> A-in)
    b.remove(to=63)                             # A-in -> Rm; across 64 from above
    b.replace(at=(0, 31, 32, 62))               # Rm -> Rp
    b.add(3)                                    # A-grow 66 / 126 (Rp -> A-grow); across 64
    b.add(3)                                    # A-in 69
    b.replace(at=(64, 68))                      # A-in -> Rp
    b.add(3)                                    # A-in 72 (Rp -> A-in)
    b.add(60)                                   # A-grow 132 / 252 (A-in -> A-grow); across 96 and 128
    b.remove(to=33)                             # A-grow -> Rm; across 128, 96, 64
    b.refused(X_KINDS[0])
    b.remove(everything=True)                   # the empty index: the image is gone for good
    b.add(40)                                   # A-grow 40 / 40
    b.build()
    b.add(10)                                   # A-grow 50 / 80
    b.add(5, nan=True)                          # A-in 55: a NaN row; the statistics stay finite, the image follows
    b.replace(at=(20,), clean=True)             # the NaN row out by a replace
    b.add(4, inf=True)                          # A-in 59: an infinite row: the image is dropped
    b.replace(at=(54,), clean=True)             # the infinite row out: the image stays gone
    b.build()
    b.add(4)                                    # A-in 63
    b.remove(to=60)


def _script_short(b):
    b.add(30)                                   # A-grow 1 030 / 2 000: beyond the short-corpus form
    b.remove(to=1020)                           # back inside it
    b.replace(at=(0, 500, -1))                  # the short-corpus image of the old matrix exists (the checks searched)
    b.add(4)                                    # A-grow 1 024 / 2 040: the last short corpus
    b.add(1)                                    # A-in 1 025: the exact form
    b.refused(X_KINDS[1])
    b.replace(at=(1023, 1024))
    b.remove(to=1023)
    b.add(3, ties=1)                            # A-grow 1 026
    b.remove(to=1024)
    b.refused(X_KINDS[0])


def _script_rowwaves(b):
    b.add(10)                                   # A-grow 16 390 / 32 760: Scan
    b.remove(to=16384)                          # RowWaves, the last
    b.add(3, ties=1)                            # A-grow 16 387: Scan
    b.replace(at=(16383, 16384, 16386))
    b.remove(to=16385)
    b.remove(to=16383)
    b.refused(X_KINDS[2])
    b.replace(at=(0, 16382))
    b.add(3, ties=1)                            # A-grow 16 386
    b.add(3, ties=1)                            # A-in 16 389
    b.remove(to=16384)


def _script_hi(b):
    b.build()
    b.replace(at=(3, 17))                       # the first tile
    b.replace(at=(3401, 3430))                  # a middle tile
    b.replace(at=(-2, -1))                      # the last tile (the tiles: test_update_sequence's stale-maxima certificate)
    b.refused(X_KINDS[3])
    b.add(20)                                   # A-grow
    b.add(30)                                   # A-in: img_rows mid-tile
    b.replace(at=(6000, 6001))                  # A-in -> Rp at the same scale: the image is refreshed from row 5 984 on only
    b.remove(every=97)                          # every tile's content shifts
    b.add(40, large=True)                       # A-grow: the scale rises
    b.remove(large=True, every=1000)            # the scale falls (rows of every part of the matrix go with the large one)
    b.add(40)                                   # A-grow
    b.add(35)                                   # A-in
    b.replace(at=(3000, 5000), large=True)      # the scale rises by a replace whose first row is deep in the matrix
    b.replace(at=(3300,), unlarge=True)         # and falls by one
    b.remove(to=HI_MIN_ROWS - 17)               # below the admitting count: the route leaves the fp16 first pass
    b.replace(at=(100, 6000))
    b.add(40)                                   # A-grow: the route returns
    b.add(35)                                   # A-in
    b.refused(X_KINDS[0])


PROFILES = {
    "dense-tiles": dict(d=128, n0=70, seed=7101, ladder0=2, ties0=0, script=_script_tiles, hi=False),
    "dense-short": dict(d=128, n0=1000, seed=7102, ladder0=3, ties0=4, script=_script_short, hi=False),
    "dense-rowwaves": dict(d=4, n0=16380, seed=7103, ladder0=2, ties0=3, script=_script_rowwaves, hi=False),
    "dense-hi": dict(d=128, n0=HI_MIN_ROWS + 83, seed=7104, ladder0=14, ties0=14, script=_script_hi, hi=True),
}
DENSE_PROFILES = tuple(PROFILES)


@functools.lru_cache(maxsize=None)
def dense_states(profile):
    b = _Builder(profile)
    PROFILES[profile]["script"](b)
    return tuple(b.states)


def updates(states):
    """The states that an update (not a build, not a refusal, not the creation) made, each with its predecessor."""
    return [(states[i - 1], s) for i, s in enumerate(states) if s.kind in KINDS]


# ---- the route at a state ---------------------------------------------------------------------------------------------
def form_at(st, nq, k, pins):
    return DA.form_of(st.n, st.d, nq, k, pins, st.finite)


# ---- certificates -----------------------------------------------------------------------------------------------------
def transitions(states):
    """(ordered pairs of update kinds with only refusals / builds between them, kinds a refusal follows)."""
    pairs, refused_after, last = set(), set(), None
    for s in states:
        if s.kind in KINDS:
            if last:
                pairs.add((last, s.kind))
            last = s.kind
        elif s.kind == "X" and last:
            refused_after.add(last)
    return pairs, refused_after


def crossings(states, mark):
    """('up', 'down') directions in which n crosses `mark` (n <= mark on one side, n > mark on the other)."""
    out = set()
    for a, b in zip(states, states[1:]):
        if a.n <= mark < b.n:
            out.add("up")
        if b.n <= mark < a.n:
            out.add("down")
    return out


def events(states):
    """Named events of a dense script -> the steps where they occur."""
    ev = {}

    def hit(name, s):
        ev.setdefault(name, []).append(s.step)
    for a, b in zip(states, states[1:]):
        ea, eb = scale_exp(amax_of(a.X)), scale_exp(amax_of(b.X))
        if b.kind in KINDS:
            if eb >= ea + 3:
                hit(f"scale up by {b.kind}", b)
            if eb <= ea - 3 and b.n:
                hit(f"scale down by {b.kind}", b)
            if b.cap > a.cap and b.kind == "A-grow":
                hit("capacity grows", b)
            if b.kind == "A-grow" and a.cap == a.n:
                hit("add at cap == n", b)
            if b.kind == "Rp" and a.kind == "A-in" and a.n % 32 and int(b.op[1][0]) % 32:
                hit("replace from mid-tile after an A-in that left img_rows mid-tile", b)
            if b.nan_rows.size > a.nan_rows.size:
                hit(f"NaN row in by {b.kind}", b)
            if b.nan_rows.size < a.nan_rows.size:
                hit(f"NaN row out by {b.kind}", b)
            inf_a, inf_b = int(np.isinf(a.X).any(axis=1).sum()), int(np.isinf(b.X).any(axis=1).sum())
            if inf_b > inf_a:
                hit(f"infinite row in by {b.kind}", b)
            if inf_b < inf_a:
                hit(f"infinite row out by {b.kind}", b)
            if a.image[0] and not b.image[0]:
                hit("image dropped", b)
            if b.n == 0:
                hit("emptied", b)
            if a.n == 0:
                hit("add to the empty index", b)
        if b.kind == "B" and not a.image[0]:
            hit("image built", b)
    return ev


def coverage_table(profile):
    states = dense_states(profile)
    lines = [f"{profile}: {len(states) - 1} steps"]
    for s in states:
        lines.append(f"  {s.step:>2} {s.kind:<6} n={s.n:<6} cap={s.cap:<6} image={s.image}  {s.note}")
    pairs, ref = transitions(states)
    lines.append("  pairs: " + ", ".join(f"{a}->{b}" for a, b in sorted(pairs)))
    lines.append("  refused after: " + ", ".join(sorted(ref)))
    for name, steps in sorted(events(states).items()):
        lines.append(f"  {name}: steps {steps}")
    return "\n".join(lines)


# ---- wrong handles, restated in numpy -----------------------------------------------------------------------------------
def tile_maxima(X, Q):
    """[nq, tiles] the largest exact score of each 32-row tile (-inf for NaN scores)."""
    S = rank_scores(X, Q)
    n = X.shape[0]
    pad = (-n) % 32
    S = np.concatenate([S, np.full((S.shape[0], pad), -np.inf)], axis=1)
    return S.reshape(S.shape[0], -1, 32).max(axis=2)


def stale_image_topk(X_prev, X, Q, k, kc=HI_KC0):
    """A handle whose first pass reads an image of the PREVIOUS matrix: the kc best tiles by the stale maxima (tiles
    the old matrix did not have rank last), re-scored exactly on the current matrix."""
    T_old = tile_maxima(X_prev, Q)
    tiles = (X.shape[0] + 31) // 32
    T = np.full((Q.shape[0], tiles), -np.inf)
    w = min(tiles, T_old.shape[1])
    T[:, :w] = T_old[:, :w]
    ids = np.full((Q.shape[0], k), -1, np.int64)
    for q in range(Q.shape[0]):
        best = np.lexsort((np.arange(tiles), -T[q]))[:kc]
        rows = np.concatenate([np.arange(t * 32, min(t * 32 + 32, X.shape[0])) for t in best])
        ids[q] = scoped_expected(X, Q[q:q + 1], np.sort(rows), k)[1][0]
    return ids


def wrong_add_at_capacity(prev, st):
    """An in-place add that writes at cap_rows instead of n: rows [n_old, n_new) keep what the allocation held — the
    zeros of a fresh allocation here."""
    X = st.X.copy()
    X[prev.n:] = 0.0
    return X


def wrong_remove_keeps_positions(prev, st):
    """A remove that leaves the survivors at their old positions: the first n_new rows of the old matrix."""
    return prev.X[: st.n].copy()


def wrong_partial_image(prev, st):
    """A replace that converts the image again only from the first replaced row's tile on although the scale changed:
    the tiles before it hold the old rows at the old scale, i.e. scores off by the ratio of the scales."""
    ids = st.op[1]
    t0 = int(ids[0]) // 32 * 32
    ratio = 2.0 ** (scale_exp(amax_of(prev.X)) - scale_exp(amax_of(st.X)))
    X = st.X.astype(np.float64).copy()
    X[:t0] = prev.X[:t0].astype(np.float64) * ratio
    return X


# =========================================================================================================================
# BM25: a list of token lists.  After every step oracle.bm25.BM25Okapi is fitted from nothing on the model's documents and
# oracle.bm25.to_csr gives the expected resident arrays; the operands of the native call come from the product's own path
# (legal_rag_amd.bm25_model.BM25Okapi.{add,remove,replace}_documents with the resident index attached) in the GPU test.
# The handle has no capacity: the kinds are A, Rm, Rp (nine ordered pairs) and X.
# =========================================================================================================================
BM25_TILE = 2048      # postings per tile of the update kernels (amdr_bm25_info word 4; the GPU test asserts it)
BM25_KINDS = ("A", "Rm", "Rp")
BM25_N0 = 300
BM25_X = ("remove id == n", "replace an id twice", "remove every document")
BM25_PROBE = ["all", "z0", "z1"]  # the query whose best document every remove takes out


def postings_of(docs):
    return sum(len(set(d)) for d in docs)


def filler(count):
    """A document of exactly `count` distinct tokens, 1 <= count <= 401: "all" and the Zipfian terms z399, z398, ..."""
    assert 1 <= count <= 401, count
    return ["all"] + [f"z{399 - j}" for j in range(count - 1)]


def fillers(total, n_docs):
    """n_docs filler documents whose distinct-token counts sum to `total`."""
    assert n_docs <= total <= 401 * n_docs, (total, n_docs)
    base, extra = divmod(total, n_docs)
    return [filler(base + (1 if j < extra else 0)) for j in range(n_docs)]


def first_seen(docs):
    """The vocabulary in first-seen order: the re-fit's term ids."""
    return {w: t for t, w in enumerate(dict.fromkeys(w for d in docs for w in d))}


class BM25State:
    def __init__(self, step, kind, op, docs, at, note, counts):
        self.step, self.kind, self.op, self.note, self.at = step, kind, op, note, int(at)
        self.docs = [list(d) for d in docs]
        self.n = len(docs)
        self.postings = postings_of(docs)
        self.vocab = first_seen(docs)
        self.adds, self.removes, self.replaces = counts

    @property
    def residue(self):
        r = self.postings % BM25_TILE
        return {0: "tile", 1: "tile+1", BM25_TILE - 1: "tile-1"}.get(r)

    def info(self):
        """amdr_bm25_info words 0, 1, 2, 3, 5 and amdr_bm25_replaces."""
        return (self.n, len(self.vocab), self.postings, self.adds, self.removes, self.replaces)


class _BM25Builder:
    def __init__(self):
        from bm25_update_cases import make_docs
        self.make_docs = make_docs
        self.rng = np.random.default_rng(7201)
        # terms that live in one document each (they vanish with it), one in every 40th
        self.docs = make_docs(self.rng, BM25_N0, lambda i: ([f"only{i}"] if i % 7 == 0 else []) + (["forty"] if i % 40 == 0 else []))
        self.counts = [0, 0, 0]
        self.states = [BM25State(0, "create", ("create",), self.docs, 0, "create", self.counts)]
        self.serial = 0

    def push(self, kind, op, at, note):
        self.states.append(BM25State(len(self.states), kind, op, self.docs, at, note, self.counts))

    def target(self, residue, lo):
        """The smallest postings total >= lo on the residue: -1, 0, +1 around a multiple of the tile."""
        t = (lo - residue + BM25_TILE - 1) // BM25_TILE * BM25_TILE + residue
        return t

    def best(self):
        from oracle import bm25 as OB
        return OB.search(OB.BM25Okapi(self.docs), BM25_PROBE, 1)[0][0]

    def new_docs(self, count):
        self.serial += 1
        s = self.serial
        return self.make_docs(self.rng, count, lambda i: [f"new{s}_{i % 3}"] if i % 2 == 0 else [])

    def add(self, count, residue=None, bulk=0, skip=0):
        new = self.new_docs(count)
        if bulk:  # short documents: the list of "all" grows across tiles
            new += [["all", f"b{i % 50}"] for i in range(bulk)]
        if residue is not None:
            have = postings_of(self.docs) + postings_of(new)
            need = self.target(residue, have + 1) + skip * BM25_TILE - have
            new += fillers(need, (need + 400) // 401)
        at = len(self.docs)
        self.docs = self.docs + new
        self.counts[0] += 1
        self.push("A", ("add", new), at, f"add {len(new)}" + (f" to {residue:+d} of a tile" if residue is not None else ""))

    def remove(self, count, residue=None, ids=()):
        n = len(self.docs)
        must = sorted({self.best()} | {int(i) % n for i in ids})
        pool = [int(i) for i in self.rng.permutation(n) if int(i) not in must]
        take = must + pool[:max(0, count - len(must))]
        if residue is not None:
            have = postings_of([d for i, d in enumerate(self.docs) if i not in set(take)])
            t = residue  # the largest total on the residue that is still at or below what is left
            while t + BM25_TILE <= have:
                t += BM25_TILE
            assert 0 < t <= have, (t, have)
            left = have - t
            for i in sorted(pool[count:], key=lambda i: -len(set(self.docs[i]))):  # (largest first: the fillers go)
                c = len(set(self.docs[i]))
                if c <= left:
                    take.append(i)
                    left -= c
                if left == 0:
                    break
            assert left == 0, left
        take = sorted(take)
        gone = set(take)
        self.docs = [d for i, d in enumerate(self.docs) if i not in gone]
        self.counts[1] += 1
        self.push("Rm", ("remove", take), take[0], f"remove {len(take)}" + (f" to {residue:+d} of a tile" if residue is not None else ""))

    def replace(self, ids, residue=None, new=None):
        n = len(self.docs)
        given = dict(zip([int(i) % n for i in ids], new)) if new is not None else {}
        ids = sorted({self.best()} | {int(i) % n for i in ids})
        new = self.new_docs(len(ids))
        new = [given.get(i, d) for i, d in zip(ids, new)]
        if residue is not None:
            # the last `m` new documents are fillers that bring the total onto the residue
            rest = postings_of([d for i, d in enumerate(self.docs) if i not in set(ids)])
            for m in range(1, len(ids) + 1):
                fixed = postings_of(new[: len(ids) - m])
                t = self.target(residue, rest + fixed + m)
                if t - rest - fixed <= 401 * m:
                    new = new[: len(ids) - m] + fillers(t - rest - fixed, m)
                    break
            else:
                raise AssertionError("replace: the residue is out of reach for these ids")
        assert len(new) == len(ids)
        for i, d in zip(ids, new):
            self.docs[i] = list(d)
        self.counts[2] += 1
        self.push("Rp", ("replace", ids, [list(d) for d in new]), ids[0],
                  f"replace {len(ids)} from {ids[0]}" + (f" to {residue:+d} of a tile" if residue is not None else ""))

    def refused(self, which):
        prev = self.states[-1]
        self.states.append(BM25State(len(self.states), "X", ("refused", which), self.docs, prev.at, f"refused: {which}", self.counts))


def _script_bm25(b):
    b.add(5)                                    # new terms appear
    b.refused(BM25_X[0])
    b.add(3, residue=0, skip=1)                 # A -> A: the total ON a multiple of the tile (the second), by an add
    b.remove(4)                                 # A -> Rm: only<i> terms go with their last document
    b.refused(BM25_X[2])
    b.remove(3, residue=-1, ids=(0,))           # Rm -> Rm: one below a multiple, by a remove; document 0 goes: the order of
    b.replace((7, 150, -1))                     # the vocabulary changes.  Rm -> Rp
    b.refused(BM25_X[1])
    b.replace((0, 14), residue=1)               # Rp -> Rp: one above, by a replace; document 0 replaced
    b.add(4, residue=-1)                        # Rp -> A: one below, by an add
    b.replace((3, 4, 5), residue=0)             # A -> Rp: on the multiple, by a replace
    b.remove(2, residue=1)                      # Rp -> Rm: one above, by a remove
    b.add(2, residue=1)                         # Rm -> A: one above, by an add
    b.refused(BM25_X[0])
    b.remove(5, residue=0)                      # A -> Rm: on the multiple, by a remove
    b.replace((40, 41), residue=-1)             # one below, by a replace
    # a word's first appearance moves: the word first seen in document 1 is given to document 0, in front of "all"
    w = next(x for x in b.docs[1] if x != "all" and x not in b.docs[0]) if len(b.docs[1]) > 1 else "z0"
    b.replace((0,), new=[[w, "all", "moved"]])
    b.refused(BM25_X[1])
    b.add(2, bulk=2 * BM25_TILE + 60)           # the head list "all" across three tiles
    b.replace((BM25_TILE - 1, BM25_TILE, 2 * BM25_TILE - 1, 2 * BM25_TILE, -1))  # at the tile edges of that list
    b.remove(2 * BM25_TILE, ids=(BM25_TILE - 1, BM25_TILE))                      # back to a small corpus
    b.refused(BM25_X[2])
    b.add(3)


@functools.lru_cache(maxsize=None)
def bm25_states():
    b = _BM25Builder()
    _script_bm25(b)
    return tuple(b.states)


@functools.lru_cache(maxsize=None)
def bm25_oracle(step):
    """(the oracle fitted from nothing on the state's documents, its CSR)."""
    from oracle import bm25 as OB
    ob = OB.BM25Okapi(bm25_states()[step].docs)
    return ob, OB.to_csr(ob)


def bm25_queries(step, n=24):
    """(term-id queries of bm25_update_cases.queries_for over the state's vocabulary, the same as words)."""
    from bm25_update_cases import queries_for
    st = bm25_states()[step]
    words = list(st.vocab)
    qs = queries_for(np.random.default_rng(7300 + step), len(words), n)
    return qs, [[words[t] if 0 <= t < len(words) else "no-such-word" for t in q] for q in qs]


def bm25_transitions(states):
    pairs, refused_after, last = set(), set(), None
    for s in states:
        if s.kind in BM25_KINDS:
            if last:
                pairs.add((last, s.kind))
            last = s.kind
        elif s.kind == "X" and last:
            refused_after.add((last, s.op[1]))
    return pairs, refused_after


def bm25_events(states):
    ev = {}

    def hit(name, s):
        ev.setdefault(name, []).append(s.step)
    for a, b in zip(states, states[1:]):
        if b.kind not in BM25_KINDS:
            continue
        if b.residue:
            hit(f"postings on {b.residue} by {b.kind}", b)
        if set(b.vocab) - set(a.vocab):
            hit(f"terms appear by {b.kind}", b)
        if set(a.vocab) - set(b.vocab):
            hit(f"terms go with their last document by {b.kind}", b)
        common = [w for w in a.vocab if w in b.vocab]
        if [w for w in b.vocab if w in a.vocab] != common:
            hit(f"the order of the surviving terms changes by {b.kind}", b)
        if b.n > 2 * BM25_TILE and all("all" in d for d in b.docs[: 2 * BM25_TILE + 1]):
            hit("the list of 'all' spans three tiles", b)
    return ev


def bm25_coverage_table():
    states = bm25_states()
    lines = [f"bm25: {len(states) - 1} steps"]
    for s in states:
        lines.append(f"  {s.step:>2} {s.kind:<6} docs={s.n:<5} terms={len(s.vocab):<5} postings={s.postings:<6} "
                     f"{s.residue or '':<7} {s.note}")
    pairs, ref = bm25_transitions(states)
    lines.append("  pairs: " + ", ".join(f"{a}->{b}" for a, b in sorted(pairs)))
    lines.append("  refused: " + ", ".join(f"{w} after {k}" for k, w in sorted(ref)))
    for name, steps in sorted(bm25_events(states).items()):
        lines.append(f"  {name}: steps {steps}")
    return "\n".join(lines)


def bm25_span_items(st):
    """One phrase, one Near, one union and one class span over tokens of the documents on both sides of the seam
    (term ids of the state's vocabulary): (phrases, nears, unions, class items)."""
    import class_span_cases as CC
    import near_cases as NC
    # the nearest documents of two tokens or more before the seam and from it on (a phrase has at least two tokens)
    lo = next((i for i in range(min(st.at, st.n) - 1, -1, -1) if len(st.docs[i]) >= 2), None)
    hi = next((i for i in range(min(st.at, st.n - 1), st.n) if len(st.docs[i]) >= 2), None)
    lo, hi = (lo if lo is not None else hi), (hi if hi is not None else lo)
    a = [st.vocab[w] for w in st.docs[lo]]
    b = [st.vocab[w] for w in st.docs[hi]]
    phrases = [b[:3], a[:2]]
    nears = [NC.near([a[0], b[-1]], 40), NC.near([b[0], b[-1]], len(b), ordered=True), NC.phrase(a[-2:])]
    unions = [[a[-1], b[-1]], [b[-1]]]
    classes = [CC.near_of([CC.cls(*{a[-1], b[-1]}), b[0]], 60), CC.phrase_of([a[0], CC.cls(*set(a[1:2] + b[1:2] + [b[-1]]))])]
    return phrases, nears, unions, classes


# =========================================================================================================================
# ColBERT: a list of [len, 128] float32 documents.  Integers in {-7 .. 7} on both sides ("large" tokens times 8): the
# exactness conditions of maxsim_adversary (split_expected / f32_expected assert them on every state).  Query 0 has a
# ladder — the documents Q[0][:m], m = 6 .. 32, whose scores rise with m — and the other queries tie documents (copies of
# Q[t][:16]).  The model predicts amdr_maxsim_info (csrc/maxsim_store.hip): token capacity (create: the tokens; a growing add:
# max(2 cap, tokens); a rebuild — remove, replace —: the tokens; the document capacity likewise), the scale exponent,
# whether the split-fp16 images exist (a non-finite value takes them away, the rebuild that removes the last one brings
# them back; an add never does) and the conversions (+1 per create-like rebuild of a finite store and per add that raises
# the scale).  A-in: neither capacity grows; A-grow: either does.  A rebuild leaves both capacities exact, so neither
# Rm -> A-in nor Rp -> A-in can occur.
# =========================================================================================================================
MS_DIM = 128
MS_NQ, MS_QLEN, MS_K = 8, 32, 10
MS_NQS = (1, 7, 8)
MS_X = ("remove id == n", "replace an id twice", "add an empty document", "remove every document")


@functools.lru_cache(maxsize=None)
def ms_queries():
    rng = np.random.default_rng(7401)
    Q = rng.integers(-7, 8, size=(MS_NQ, MS_QLEN, MS_DIM)).astype(np.float32)
    Q[:, 0, 5] = np.where(np.arange(MS_NQ) % 2 == 0, 7.0, -7.0)  # the scale of every query
    return Q


def ms_store(docs):
    ptr = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(docs), dtype=np.float32), ptr


def ms_rank_scores(docs, Q):
    """fp64 MaxSim of every document by the rule of include/amdretrieval.h (a NaN similarity never wins a maximum)."""
    import maxsim_adversary as MS
    D, ptr = ms_store(docs)
    return MS.nonfinite_expected(D, ptr, Q).astype(np.float64)


class MsState:
    def __init__(self, step, kind, op, b, at, note):
        self.step, self.kind, self.op, self.note, self.at = step, kind, op, note, int(at)
        self.docs = [d.copy() for d in b.docs]
        self.n = len(self.docs)
        self.tokens = sum(len(d) for d in self.docs)
        self.cap_tokens, self.cap_docs = b.cap_tokens, b.cap_docs
        self.images, self.conversions, self.amax = b.images, b.conversions, b.amax

    @property
    def finite(self):
        return all(np.all(np.isfinite(d)) for d in self.docs)

    def stats(self):
        """amdr_maxsim_stats as float32: (d_scale, d_norm_max) — the power of two that brings the largest |component|
        into [0.5, 1) and the largest L2 norm of the scaled token rows (ms_tokmax_kernel); (1, 0) without images.  On the
        integer family every scaled square and every partial sum is exact in fp32, so the fp32 square root of the exact
        sum is the one value any summation order gives."""
        if not self.images:
            return np.float32(1.0), np.float32(0.0)
        scale = np.ldexp(1.0, -scale_exp(self.amax))
        ss = max(float(np.sum((d.astype(np.float64) * scale) ** 2, axis=1).max()) for d in self.docs)
        assert np.float32(ss) == ss  # (exact in fp32)
        return np.float32(scale), np.sqrt(np.float32(ss))

    def info(self):
        """amdr_maxsim_info: (docs, tokens, token capacity, e of the scale 2^e, images, conversions)."""
        e = -scale_exp(self.amax) if self.images else 0
        return (self.n, self.tokens, self.cap_tokens, e, int(self.images), self.conversions)


def _ms_amax(docs):
    """The largest |component| as ms_absmax orders it: NaN on top, then infinity."""
    a = np.abs(np.concatenate(docs))
    return float("nan") if np.isnan(a).any() else float(a.max())


def _ms_fold(a, b):
    return float("nan") if np.isnan(a) or np.isnan(b) else max(a, b)


class _MsBuilder:
    def __init__(self):
        self.rng = np.random.default_rng(7402)
        self.Q = ms_queries()
        lens = self.rng.integers(1, 221, size=48)
        lens[[0, 1, 47]] = (220, 1, 17)
        self.docs = [self.background(int(n)) for n in lens]
        self.docs[0][0, 3] = 7.0  # the store's scale, whatever the ladder does
        spots = [int(i) for i in self.rng.permutation(np.arange(2, 47))]
        for m in (6, 7, 8):
            self.docs[spots.pop()] = self.ladder_doc(m)
        for t in range(1, MS_NQ):
            for _ in range(3):
                self.docs[spots.pop()] = self.tie_doc(t)
        self.cap_tokens, self.cap_docs = sum(len(d) for d in self.docs), len(self.docs)
        self.amax = _ms_amax(self.docs)
        self.images = bool(self.amax <= FLT_MAX)
        self.conversions = int(self.images)
        self.turn = 0
        self.states = [MsState(0, "create", ("create",), self, 0, "create")]

    def background(self, n):
        return self.rng.integers(-3, 4, size=(n, MS_DIM)).astype(np.float32)

    def ladder_doc(self, m, large=False):
        return (self.Q[0, :m] * np.float32(8.0 if large else 1.0)).astype(np.float32)

    def tie_doc(self, t):
        return self.Q[t, :16].copy()

    def best0(self):
        s = ms_rank_scores(self.docs, self.Q[:1])[0]
        i = int(np.lexsort((np.arange(s.size), -s))[0])
        return i, float(s[i])

    def next_ladder(self, large=False):
        top = self.best0()[1]
        for m in range(6, MS_QLEN + 1):
            d = self.ladder_doc(m, large)
            if ms_rank_scores([d], self.Q[:1])[0, 0] > top:
                return d
        raise AssertionError("the ladder is used up")

    def push(self, kind, op, at, note):
        self.states.append(MsState(len(self.states), kind, op, self, at, note))

    def rebuilt(self):
        self.cap_tokens, self.cap_docs = sum(len(d) for d in self.docs), len(self.docs)
        self.amax = _ms_amax(self.docs)
        self.images = bool(self.amax <= FLT_MAX)
        self.conversions += int(self.images)

    def add(self, count, grow, large=False, bad=None, long=False, heavy=False):
        new = [self.background(int(n)) for n in self.rng.integers(60 if long else 1, 221 if long else 40, size=count)]
        slots = [int(i) for i in self.rng.permutation(count)]
        new[slots.pop()] = self.next_ladder(large)
        if slots:
            self.turn += 1
            new[slots.pop()] = self.tie_doc(1 + self.turn % (MS_NQ - 1))
        if heavy:  # tokens of +-7 in every component: the largest token norm of the store, at the scale it has
            new[slots.pop() if slots else 0] = (7 * self.rng.choice([-1, 1], size=(3, MS_DIM))).astype(np.float32)
        if bad is not None:
            d = self.background(5)
            d[2, 9] = bad
            new[slots.pop()] = d
        t1, n1 = sum(len(d) for d in self.docs + new), len(self.docs) + count
        grows = t1 > self.cap_tokens or n1 > self.cap_docs
        assert grows == grow, (grows, t1, self.cap_tokens, n1, self.cap_docs)
        if t1 > self.cap_tokens:
            self.cap_tokens = max(2 * self.cap_tokens, t1)
        if n1 > self.cap_docs:
            self.cap_docs = max(2 * self.cap_docs, n1)
        old = self.amax
        self.amax = _ms_fold(self.amax, _ms_amax(new))
        if self.images:
            if not self.amax <= FLT_MAX:
                self.images = False
            elif scale_exp(self.amax) != scale_exp(old):
                self.conversions += 1
        at = len(self.docs)
        self.docs = self.docs + new
        self.push("A-grow" if grow else "A-in", ("add", new), at,
                  f"add {count}" + (" large" if large else "") + (" heavy" if heavy else "") + (f" {bad}" if bad is not None else ""))

    def remove(self, to, large=False, bad=False):
        n = len(self.docs)
        must = {self.best0()[0]}
        if large:
            must |= {i for i, d in enumerate(self.docs) if np.nanmax(np.abs(d)) > 7 and np.all(np.isfinite(d))}
        if bad:
            must |= {i for i, d in enumerate(self.docs) if not np.all(np.isfinite(d))}
        must.discard(0)  # (document 0 holds the store's scale)
        pool = [int(i) for i in self.rng.permutation(np.arange(1, n)) if int(i) not in must]
        keep_out = set() if bad else {i for i, d in enumerate(self.docs) if not np.all(np.isfinite(d))}
        pool = [i for i in pool if i not in keep_out]
        ids = sorted(must | set(pool[: max(0, n - to - len(must))]))
        assert n - len(ids) == to, (n, len(ids), to)
        self.docs = [d for i, d in enumerate(self.docs) if i not in set(ids)]
        self.rebuilt()
        self.push("Rm", ("remove", ids), ids[0], f"remove {len(ids)}" + (" large" if large else "") + (" non-finite out" if bad else ""))

    def replace(self, at=(), new=None, large=False, unlarge=False, clean=False):
        n = len(self.docs)
        best = self.best0()[0]
        put = {best: self.background(int(self.rng.integers(1, 40)))}
        if unlarge:
            put.update({i: self.background(9) for i, d in enumerate(self.docs) if np.all(np.isfinite(d)) and np.abs(d).max() > 7})
        if clean:
            put.update({i: self.background(9) for i, d in enumerate(self.docs) if not np.all(np.isfinite(d))})
        self.turn += 1
        for j, r in enumerate(at):
            r = int(r) % n
            put[r] = new[j] if new is not None else self.tie_doc(1 + (self.turn + j) % (MS_NQ - 1))
        if large:
            r = next(i for i in range(n - 1, 0, -1) if i != best)
            self.docs[best] = put[best]
            put[r] = self.next_ladder(True)
        ids = sorted(put)
        docs = [put[i] for i in ids]
        for i, d in zip(ids, docs):
            self.docs[i] = d
        self.rebuilt()
        self.push("Rp", ("replace", ids, docs), ids[0], f"replace {len(ids)} from {ids[0]}" + (" large" if large else "") +
                  (" large out" if unlarge else "") + (" non-finite out" if clean else ""))

    def refused(self, which):
        prev = self.states[-1]
        self.states.append(MsState(len(self.states), "X", ("refused", which), self, prev.at, f"refused: {which}"))


def _script_colbert(b):
    b.remove(38)                                # below 4 k <= n_docs at k = 10: the one-pass form
    b.add(3, grow=True)                         # 41: the two-pass form again (Rm -> A-grow)
    b.remove(39)                                # A-grow -> Rm
    b.add(1, grow=True)                         # 40: the last two-pass corpus
    b.refused(MS_X[0])
    b.add(2, grow=False)                        # A-grow -> A-in
    b.add(2, grow=False)                        # A-in -> A-in
    b.refused(MS_X[2])
    b.add(3, grow=False, heavy=True)            # the largest token norm rises, the scale does not: d_norm_max by an add alone
    # a one-token first document (its first token: it holds the store's scale) and a 220-token last one
    b.replace(at=(0, -1), new=[b.docs[0][:1].copy(), b.background(220)])
    b.refused(MS_X[1])
    b.add(3, grow=True)                         # Rp -> A-grow
    b.add(1, grow=False, large=True)            # the scale rises by an add: conversions + 1
    b.remove(40, large=True)                    # A-in -> Rm: the scale falls
    b.refused(MS_X[3])
    b.remove(39)                                # Rm -> Rm
    b.replace(at=(5,), large=True)              # Rm -> Rp: the scale rises by a rebuild
    b.replace(at=(6, 20), unlarge=True)         # Rp -> Rp: and falls by one
    b.remove(38)                                # Rp -> Rm
    b.add(2, grow=True)
    b.add(30, grow=True, long=True)             # A-grow -> A-grow: the token capacity doubles again
    b.add(2, grow=False)
    b.add(130, grow=True, long=True)            # A-in -> A-grow
    b.replace(at=(0, 100, -1))                  # A-grow -> Rp
    b.add(3, grow=True, bad=np.nan)             # a NaN token: the images go
    b.refused(MS_X[2])
    b.add(1, grow=False)                        # an add to a store without images
    b.remove(120, bad=True)                     # the NaN document out by a remove: the images are back
    b.add(3, grow=True, bad=np.nan)
    b.replace(at=(7,), clean=True)              # the NaN document out by a replace: the images are back
    b.add(3, grow=True, bad=np.inf)             # an infinity
    b.remove(44, bad=True)
    b.remove(39)
    b.add(1, grow=True)                         # 40


@functools.lru_cache(maxsize=None)
def ms_states():
    b = _MsBuilder()
    _script_colbert(b)
    return tuple(b.states)


def ms_events(states):
    ev = {}

    def hit(name, s):
        ev.setdefault(name, []).append(s.step)
    for a, b in zip(states, states[1:]):
        if b.kind not in KINDS:
            continue
        if b.images and a.images and scale_exp(b.amax) > scale_exp(a.amax):
            hit(f"scale up by {b.kind}", b)
        if b.images and a.images and scale_exp(b.amax) < scale_exp(a.amax):
            hit(f"scale down by {b.kind}", b)
        if a.images and b.images and b.kind in ("A-in", "A-grow") and scale_exp(b.amax) == scale_exp(a.amax) and \
                max(np.linalg.norm(d, axis=1).max() for d in b.docs) > max(np.linalg.norm(d, axis=1).max() for d in a.docs):
            hit("the largest token norm rises by an add that keeps the scale", b)
        if a.images and not b.images:
            hit(f"images gone by {b.kind}", b)
        if b.images and not a.images:
            hit(f"images back by {b.kind}", b)
        if not a.images and not b.images:
            hit(f"{b.kind} on a store without images", b)
        if b.cap_tokens > a.cap_tokens and b.kind == "A-grow":
            hit("token capacity grows", b)
        if b.cap_docs > a.cap_docs and b.kind == "A-grow":
            hit("document capacity grows", b)
        if (a.n >= 4 * MS_K) != (b.n >= 4 * MS_K):
            hit("two-pass condition " + ("on" if b.n >= 4 * MS_K else "off"), b)
        if b.kind == "Rp" and any(len(d) == 1 for d in b.op[2]) and any(len(d) == 220 for d in b.op[2]):
            hit("one-token and 220-token replacements", b)
    return ev


def ms_coverage_table():
    states = ms_states()
    lines = [f"colbert: {len(states) - 1} steps"]
    for s in states:
        lines.append(f"  {s.step:>2} {s.kind:<6} info={s.info()}  {s.note}")
    pairs, ref = transitions(states)
    lines.append("  pairs: " + ", ".join(f"{a}->{b}" for a, b in sorted(pairs)))
    lines.append("  refused after: " + ", ".join(sorted(ref)))
    for name, steps in sorted(ms_events(states).items()):
        lines.append(f"  {name}: steps {steps}")
    return "\n".join(lines)


# =========================================================================================================================
# Serving: a dense matrix (d = 64, random unit rows) and a BM25 corpus edited in lockstep, across the 2 048 rows up to which
# HybridEngine.search_batch of 1-4 queries is ONE launch (hybrid_small_applies).  The one profile without an exact
# reference: the live engine — kept across the steps — is compared with an engine of fresh handles.
# =========================================================================================================================
SERVING_D, SERVING_N0, SERVING_MAX = 64, 2040, 2048


class ServingState:
    def __init__(self, step, kind, op, X, docs, at, note):
        self.step, self.kind, self.op, self.at, self.note = step, kind, op, int(at), note
        self.X, self.docs, self.n = X.copy(), [list(d) for d in docs], len(docs)


@functools.lru_cache(maxsize=None)
def serving_states():
    from bm25_update_cases import make_docs
    rng = np.random.default_rng(7501)

    def rows(n):
        X = rng.standard_normal((n, SERVING_D)).astype(np.float32)
        return X / np.linalg.norm(X, axis=1, keepdims=True)
    X, docs = rows(SERVING_N0), make_docs(rng, SERVING_N0)
    states = [ServingState(0, "create", ("create",), X, docs, 0, "create")]

    def push(kind, op, at, note):
        states.append(ServingState(len(states), kind, op, X, docs, at, note))
    for kind, arg in (("A", 10), ("Rm", 3), ("A", 1), ("X", None), ("A", 1), ("Rp", 4), ("Rm", 1), ("Rp", 3), ("Rm", 2), ("A", 3)):
        n = len(docs)
        if kind == "A":
            R, new = rows(arg), make_docs(rng, arg, lambda i: [f"s{len(states)}"])
            X, docs = np.concatenate([X, R]), docs + new
            push("A", ("add", R, new), n, f"add {arg}")
        elif kind == "Rm":
            ids = np.sort(rng.choice(n, size=arg, replace=False)).astype(np.int64)
            keep = np.ones(n, bool)
            keep[ids] = False
            X, docs = np.ascontiguousarray(X[keep]), [d for i, d in enumerate(docs) if keep[i]]
            push("Rm", ("remove", ids), int(ids[0]), f"remove {arg}")
        elif kind == "Rp":
            ids = np.sort(np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), size=arg - 2, replace=False)])).astype(np.int64)
            R, new = rows(arg), make_docs(rng, arg, lambda i: [f"s{len(states)}"])
            X = X.copy()
            X[ids] = R
            docs = list(docs)
            for i, d in zip(ids, new):
                docs[int(i)] = d
            push("Rp", ("replace", ids, R, new), int(ids[0]), f"replace {arg}")
        else:
            push("X", ("refused",), states[-1].at, "refused: id == n")
    return tuple(states)


# ---- the two-pass bound across a scale-lowering rebuild ---------------------------------------------------------------
# On the integer family above the hi-only first pass is exact, so no value of d_norm_max can change a result there: what
# a bound kept from BEFORE a rebuild does is shown on a store whose first pass is inexact.  rounding_adversary's inversion
# store (k true targets per query whose fp16 images round down, competitors whose images round up) behind ONE document of
# one token with one component of 8 x the store's largest: it sets the scale three steps lower and its scaled norm is below
# 1, while the other tokens' scaled norms are then 8 times smaller than they are once it is gone.  Removing it (or
# replacing it by a small document) raises the scale by three steps and the true bound by the same; a handle that kept
# d_norm_max would search with a margin ~4.6 times too small.
BOUND_K = 10


@functools.lru_cache(maxsize=None)
def ms_bound_case():
    """dict(Q, before = (D, doc_ptr) with the large document first, after = (D, doc_ptr) without it, small = the document
    a replace puts in its place, top = the fp64 oracle's top-k ids of `after`)."""
    import rounding_adversary as RA
    c = RA.maxsim_inversion(np.random.default_rng(910), 16, BOUND_K, groups=8, reps=2, nc=12)
    D, ptr = np.ascontiguousarray(c["D"], np.float32), np.asarray(c["doc_ptr"], np.int64)
    big = np.zeros((1, MS_DIM), np.float32)
    big[0, 7] = np.float32(8.0) * np.abs(D).max()
    small = np.zeros((1, MS_DIM), np.float32)
    small[0, 7] = np.abs(D).min()
    before = (np.concatenate([big, D]), np.concatenate([[0], ptr + 1]).astype(np.int64))
    return dict(Q=np.ascontiguousarray(c["Q"], np.float32), before=before, after=(D, ptr), small=small, top=c["top"])


def ms_scaled_norm_max(D):
    """The largest L2 norm of the token rows at the store's own power-of-two scale, in fp64."""
    import rounding_adversary as RA
    d_scale, _ = RA.maxsim_scales(np.zeros((1, 1, MS_DIM)), D)
    return float(np.linalg.norm(np.asarray(D, np.float64) * d_scale, axis=1).max())


def ms_eps_with_norm(Q, D, dmax):
    """rounding_adversary.maxsim_eps with the store's largest scaled token norm given (the handle's d_norm_max)."""
    import rounding_adversary as RA
    d_scale, q_scale = RA.maxsim_scales(Q, D)
    nsum = np.linalg.norm(np.asarray(Q, np.float64) * q_scale[:, None, None], axis=2).sum(axis=1)
    return (1.5 * 9.765625e-4 * nsum * dmax * 1.0001 + Q.shape[1] * 256.0 * 2.98023224e-8) / (q_scale * d_scale)

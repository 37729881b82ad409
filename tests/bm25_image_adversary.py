"""Adversarial corpora for the fp32-image ranking of the BM25 channel (csrc/bm25_core.hpp, bm25_select_f32).  Not a
test module: tests/test_bm25_image_adversary.py proves on the CPU that the data is what it claims,
tests/test_bm25_image_adversary_gpu.py runs it.

The selector picks candidates on fp32 IMAGES of the fp64 scores and then checks that the image order is the exact order.
Everything here puts documents whose images are equal and whose fp64 scores are not around the cut (position k - 1 of
the sorted survivors), above all with the LARGER score on the HIGHER document id, behind at least k equal ones: an order
taken from (image desc, document asc) alone is then wrong.

Exact scores by construction: every document holds exactly one term once and every doc_len equals avgdl, so with
k1 = 1.5, b = 0.75 the per-posting factor is 1 * 2.5 / (1 + 1.5 * (0.25 + 0.75)) = 1.0 exactly and a document's score is
0.0 + idf * 1.0 = the idf of its term, whatever the accumulation order.  Documents of unlisted terms stay at +0.0.

The expected results come from ref_scores / ref_topk (plain numpy fp64 over the CSR arrays) and from nothing else;
select_model restates the selector and only serves to prove that a case reaches the gap."""
from dataclasses import dataclass, field

import numpy as np

K1, B = 1.5, 0.75
DOC_LEN, AVGDL = 7, 7.0
REL = 1e-12  # relative distance of the exact scores inside one image run (fp32 resolves 6e-8)
DBL_MAX = float(np.finfo(np.float64).max)
SUB = 2.0 ** -149  # smallest fp32 subnormal

SHAPES = (200, 448, 591, 1000, 1260, 2048)  # one per register bucket of bm_run (slabs <= 256 ... 2 048 documents)
TINY = 48  # a slab that fits one register per lane: every document survives, no overflow branch
MULTI = (5000, 9000)  # 3 and 5 slabs at k <= 16
DEPTHS = (1, 2, 10, 16, 17, 40, 64)
ARGMAX, STAGED = "the register arg-max rounds", "the staged selector"


# ---- the plan of csrc/bm25.hip, restated --------------------------------------------------------------------------------
def bm_use_argmax(k, slab):
    return slab <= 2048 and (k <= 16 or (k <= 96 and k * ((slab + 63) >> 6) <= 480))


def bm_plan(n, k):
    """(slab, nslabs, arg-max?) of bm_plan: balanced slabs of <= 2 048 documents for the arg-max rounds, <= 4 096 else."""
    def balanced(slab_max):
        nslabs = (n + slab_max - 1) // slab_max
        slab = min(((n + nslabs - 1) // nslabs + 15) // 16 * 16, slab_max)
        return slab, (n + slab - 1) // slab
    slab, nslabs = balanced(2048)
    argmax = bm_use_argmax(k, slab)
    if not argmax:
        slab, nslabs = balanced(4096)
    return slab, nslabs, argmax


def nvt_bucket(slab):
    """Scores per lane the register ranking is compiled for (the NVT of bm25_score_topk_kernel<1, NVT>)."""
    nv = (slab + 63) // 64
    return next(b for b in (4, 8, 10, 16, 20, 32) if nv <= b)


def plan_text(n, k):
    """The two pieces of BM25Index.plan_info a case is built for."""
    slab, nslabs, argmax = bm_plan(n, k)
    return f"slabs={nslabs} of <= {slab} documents", ARGMAX if argmax else STAGED


def selector_runs(n, k):
    """bm25_select_f32 ranks the slabs of this (n, k) (unless AMDR_BM25_SELECT=0)."""
    return k <= 64 and bm_plan(n, k)[2]


# ---- corpus and reference ----------------------------------------------------------------------------------------------
def make_csr(n, term_docs, idf):
    """CSR arrays of BM25Index: term t holds the documents term_docs[t] (ascending), each once."""
    term_ptr = np.zeros(len(term_docs) + 1, dtype=np.int64)
    term_ptr[1:] = np.cumsum([len(d) for d in term_docs])
    post_doc = np.concatenate([np.asarray(d, dtype=np.int32) for d in term_docs]) if len(term_docs) else np.zeros(0, np.int32)
    return dict(term_ptr=term_ptr, post_doc=post_doc.astype(np.int32), post_tf=np.ones(post_doc.shape[0], dtype=np.int32),
                idf=np.asarray(idf, dtype=np.float64).copy(), doc_len=np.full(n, DOC_LEN, dtype=np.int32), avgdl=AVGDL,
                k1=K1, b=B)


def csr_per_document(scores):
    """Term d = document d with idf scores[d]: a query lists the documents it switches on."""
    n = len(scores)
    return make_csr(n, [[d] for d in range(n)], scores)


def posting_factor(csr):
    """rank_bm25's parenthesis per posting, operand for operand: q_freq * (k1 + 1) / (q_freq + k1 * (1 - b + b * len / avgdl))."""
    qf = csr["post_tf"].astype(np.float64)
    dl = csr["doc_len"][csr["post_doc"]].astype(np.float64)
    return qf * (csr["k1"] + 1) / (qf + csr["k1"] * (1 - csr["b"] + csr["b"] * dl / csr["avgdl"]))


def ref_scores(csr, queries):
    """fp64 scores [nq, n]: tokens in query order, duplicates counted, unknown ids skipped."""
    n, V = csr["doc_len"].shape[0], csr["idf"].shape[0]
    w, tp, pd, idf = posting_factor(csr), csr["term_ptr"], csr["post_doc"], csr["idf"]
    out = np.zeros((len(queries), n), dtype=np.float64)
    for qi, q in enumerate(queries):
        row = out[qi]
        for t in q:
            if 0 <= t < V:
                a, b = tp[t], tp[t + 1]
                row[pd[a:b]] += idf[t] * w[a:b]  # a posting list holds a document once
    return out


def ref_topk(row, k):
    """sorted(docs, key=(-(score + 0.0), id))[:k] and the scores as ranked; (-1, -DBL_MAX) behind them."""
    x = row + 0.0
    order = np.lexsort((np.arange(x.shape[0]), -x))[:k]
    ids = np.full(k, -1, dtype=np.int64)
    sc = np.full(k, -DBL_MAX, dtype=np.float64)
    ids[:order.shape[0]] = order
    sc[:order.shape[0]] = x[order]
    return ids, sc


def images(x):
    """fp32 images as the selector's 32-bit keys (ord32: -0.0 -> +0.0, NaN lowest)."""
    with np.errstate(over="ignore", under="ignore"):
        f = np.asarray(x, dtype=np.float64).astype(np.float32) + np.float32(0.0)
    u = f.view(np.uint32).astype(np.uint64)
    key = np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000)
    return np.where(f != f, 1, key).astype(np.uint64)


# ---- the selector, restated (one slab) ----------------------------------------------------------------------------------
def select_model(sc, k, NV, whole_run=False):
    """Document order bm25_select_f32<NV> returns for the slab scores `sc`, or None where it gives up (-1).
    whole_run=False: the check of pairs (j, j + 1) with j < k only; True: every pair of the run that reaches the cut."""
    m = len(sc)
    x = np.asarray(sc, dtype=np.float64) + 0.0
    x = np.where(x != x, -DBL_MAX, x)
    img = np.zeros(NV * 64, dtype=np.uint64)
    img[:m] = images(sc)
    img = img.reshape(NV, 64)
    lb = img.max(axis=0)
    T = 0
    for bit in range(31, -1, -1):
        cand = T | (1 << bit)
        if int((lb >= cand).sum()) >= k:
            T = cand
    Te = max(T, 1)
    v_of, l_of = np.nonzero(img >= Te)
    surv = [(int(img[v, l]), int(l + 64 * v)) for v, l in zip(v_of, l_of)]
    if len(surv) > 64:
        above = int((img > T).sum())
        if T == 0 or above > 64:
            return None
        need = max(k - above, 0)
        flat = img.reshape(-1)
        if need > 0:
            eq = np.nonzero(flat == T)[0]
            if np.any(x[eq] != x[eq[0]]):
                return None
        take = []
        for v in range(NV):
            hi = [l + 64 * v for l in range(64) if img[v, l] > T]
            eq = [l + 64 * v for l in range(64) if img[v, l] == T]
            ne = min(len(eq), need)
            take += [(int(flat[i]), i) for i in hi + eq[:ne]]
            need -= ne
        surv = take
    surv.sort(key=lambda t: (-t[0], t[1]))
    cnt = len(surv)
    for j in range(cnt - 1):
        in_reach = surv[j][0] >= surv[min(k, cnt) - 1][0] if whole_run else j < k
        if in_reach and surv[j][0] == surv[j + 1][0] and x[surv[j][1]] != x[surv[j + 1][1]]:
            return None
    return [d for _, d in surv[:min(cnt, k)]]


# ---- cases -------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    family: str
    name: str
    n: int
    k: int
    csr: dict
    queries: list
    slab_ix: int = 0
    run: list = field(default_factory=list)   # documents of the image run at the cut, ascending (query 0)
    high: list = field(default_factory=list)  # the run's documents that score more than its first ones
    reach: bool = False  # built to be DECIDED WRONGLY by a check of the pairs below k only

    def slab_scores(self, row):
        """The slab that holds the run, as the kernel sees it: (scores, first document, NV bucket)."""
        slab, _, _ = bm_plan(self.n, self.k)
        lo = self.slab_ix * slab
        return row[lo:min(lo + slab, self.n)], lo, nvt_bucket(slab)


def _geometry(n, k, slab_ix):
    slab, nslabs, _ = bm_plan(n, k)
    lo = slab_ix * slab
    return lo, min(lo + slab, n) - lo


def _exact32(rng, lo=0.5, hi=4.0):
    """A score that is its own fp32 image, so that a relative 1e-12 beside it cannot cross a rounding boundary."""
    return float(np.float32(rng.uniform(lo, hi)))


def _bump(a, i=0, rel=REL):
    """The i-th exact score above a inside a's image."""
    return a + abs(a) * rel * (i + 1)


def _lows(rng, L, hi_local):
    """L local ids below hi_local on L different lanes: the run alone fills k lane bests, so the cut is its image."""
    assert L <= min(64, hi_local), (L, hi_local)
    lanes = rng.permutation(min(64, hi_local))[:L]
    return sorted(int(l + 64 * rng.integers(0, (hi_local - 1 - l) // 64 + 1)) for l in lanes)


VARIANTS = ("at-k", "at-k+1", "run-end", "lane-63", "register>0", "slab-end")


def run_case(family, n, k, seed, variant, *, slab_ix=0, a=None, sign=1, smaller=False, high_vals=None, below=None,
             reach=True, name=None):
    """One image run across the cut in slab `slab_ix` of an n-document corpus: L >= k documents score a, then (higher
    ids) one to four that share a's fp32 image and score more (smaller=True: less).  Up to k - 1 documents of higher
    images sit above, documents of lower images below.  Returns None where the slab has no room for the variant.
    "at-k" puts the larger score at sorted position k exactly: the pair (k - 1, k) differs, which a check of the pairs
    below k sees too, so that variant is not marked as reaching the gap; every other one has k + 1 or more equal scores
    before the larger one."""
    rng = np.random.default_rng([seed, n, k, VARIANTS.index(variant), slab_ix, int(sign > 0), int(smaller)])
    lo, m = _geometry(n, k, slab_ix)
    if a is None:
        a = sign * _exact32(rng)
    nh = 1 if variant in ("run-end", "slab-end") else 1 + int(rng.integers(0, 4))
    L = k + {"at-k": 0, "at-k+1": 1, "run-end": 3}.get(variant, int(rng.choice([1, 2, 3])))
    if variant == "lane-63":
        regs = [r for r in range((m + 63) // 64) if L <= 63 + 64 * r < m]
        if not regs:
            return None
        hi_local = 63 + 64 * int(rng.choice(regs))
    elif variant == "register>0":
        if max(64, L) >= m:
            return None
        hi_local = int(rng.integers(max(64, L), m))
    elif variant == "slab-end":
        hi_local = m - 1
    else:
        hi_local = int(rng.integers(L, m))
    if L > min(64, hi_local) or L + nh > 64:
        return None
    lows = _lows(rng, L, hi_local)
    free = [i for i in range(hi_local + 1, m)]
    nh = min(nh, 1 + len(free))
    highs = [hi_local] + sorted(int(i) for i in rng.choice(free, size=nh - 1, replace=False)) if nh > 1 else [hi_local]
    if high_vals is None:
        hv = [(a - abs(a) * REL * (i + 1)) if smaller else _bump(a, i) for i in range(nh)]
    else:
        hv = [high_vals[i % len(high_vals)] for i in range(nh)]
    sc = np.zeros(n, dtype=np.float64)
    hot = np.zeros(n, dtype=bool)
    used = set(lows) | set(highs)
    rest = np.array([i for i in range(m) if i not in used], dtype=np.int64)
    rng.shuffle(rest)
    A = int(rng.integers(0, min(k - 1, 64 - L - nh) + 1)) if (seed % 2 and high_vals is None and variant != "at-k") else 0
    above, rest = rest[:A], rest[A:]
    for j, i in enumerate(above):  # distinct higher images (a < 0: the first of them is an untouched document at +0.0)
        sc[lo + i] = a + abs(a) * (1 + j)
        hot[lo + i] = sc[lo + i] != 0.0
    for i in lows:
        sc[lo + i], hot[lo + i] = a, True
    for i, v in zip(highs, hv):
        sc[lo + i], hot[lo + i] = v, True
    if below is None:
        below = [a / 2, a / 4] if a > 0 else [2 * a, 4 * a]
    if a > 0:  # the other documents: untouched, but for a few of lower images here and in the other slabs
        others = [lo + int(i) for i in rest[:int(rng.integers(0, 31))]]
        others += [int(d) for d in rng.choice(n, size=min(n, 12), replace=False) if not lo <= d < lo + m]
    else:      # a negative run ranks below every untouched document: all the others score lower still
        others = [d for d in range(n) if not hot[d] and not (lo <= d < lo + m and (d - lo) in set(above.tolist()))]
    for d in others:
        sc[d], hot[d] = below[int(rng.integers(0, len(below)))], True
    query = [int(d) for d in rng.permutation(np.nonzero(hot)[0])]
    return Case(family, name or f"{family} n={n} k={k} slab={slab_ix} {variant} seed={seed}" + (" neg" if a < 0 else ""),
                n, k, csr_per_document(sc), [query], slab_ix, [lo + i for i in lows + highs],
                [] if smaller else [lo + i for i in highs], reach and not smaller and variant != "at-k")


def f1(n, k, seed, slab_ix=0):
    """Run across the cut, LARGER score beyond it: every variant the slab has room for."""
    sign = -1 if seed % 3 == 2 else 1
    cs = [run_case("F1", n, k, seed, v, slab_ix=slab_ix, sign=sign) for v in VARIANTS]
    return [c for c in cs if c is not None]


def f2(n, k, seed, slab_ix=0):
    """Run across the cut, SMALLER score beyond it: the image order is the exact order."""
    sign = -1 if seed % 3 == 2 else 1
    cs = [run_case("F2", n, k, seed, v, slab_ix=slab_ix, sign=sign, smaller=True) for v in VARIANTS[:3] + VARIANTS[5:]]
    return [c for c in cs if c is not None]


def f3a(n, k, seed):
    """Overflow branch, mass tie AT the cut image: more than 64 documents of one exact score, one larger at a high id."""
    rng = np.random.default_rng([seed, n, k, 31])
    lo, m = _geometry(n, k, 0)
    if m < 80:
        return []
    a = _exact32(rng)
    hi_local = m - 1 - int(rng.integers(0, 5))
    lows = set(_lows(rng, 64, hi_local))
    extra = [i for i in rng.permutation(hi_local) if i not in lows][:int(rng.integers(1, 30))]
    lows = sorted(lows | {int(i) for i in extra})
    sc = np.zeros(n, dtype=np.float64)
    sc[lows] = a
    sc[hi_local] = _bump(a)
    free = [i for i in range(m) if sc[i] == 0.0]
    for j, i in enumerate(rng.permutation(free)[:int(rng.integers(0, k))]):
        sc[i] = a * (2 + j)
    for i in rng.permutation([i for i in range(m) if sc[i] == 0.0])[:20]:
        sc[i] = a / 2
    query = [int(d) for d in rng.permutation(np.nonzero(sc)[0])]
    return [Case("F3a", f"F3a n={n} k={k} seed={seed}", n, k, csr_per_document(sc), [query], 0, lows + [hi_local],
                 [hi_local], False)]


def f3b(n, k, seed):
    """Overflow branch, the documents ABOVE the cut image hold an F1 run.  They sit in one lane column (local ids
    congruent mod 64): one lane best, so the cut falls to the image of a mass tie below while above >= k."""
    rng = np.random.default_rng([seed, n, k, 32])
    lo, m = _geometry(n, k, 0)
    sign = -1 if seed % 3 == 2 else 1
    lanes = [c for c in range(64) if len(range(c, m, 64)) >= k + 2]  # k + 1 equal scores and a larger one
    if k < 2 or not lanes or m < 80:
        return []
    c = int(rng.choice(lanes))
    col = list(range(c, m, 64))
    L = min(k + int(rng.choice([1, 2, 3])), len(col) - 1)
    nh = min(1 + int(rng.integers(0, 4)), len(col) - L)
    pick = sorted(int(i) for i in rng.choice(col, size=L + nh, replace=False))
    lows, highs = pick[:L], pick[L:]
    a = sign * _exact32(rng)
    tie = a / 2 if a > 0 else 2 * a
    sc = np.zeros(n, dtype=np.float64)
    hot = np.zeros(n, dtype=bool)
    sc[lows], hot[lows] = a, True
    for j, i in enumerate(highs):
        sc[i], hot[i] = _bump(a, j), True
    free = np.array([i for i in range(m) if not hot[i] and i % 64 != c])
    if a > 0:  # every other lane holds a document of the tie, 64 + a few in all
        ties = {int(rng.choice(free[free % 64 == l])) for l in range(64) if l != c}
        ties |= {int(i) for i in rng.choice(free, size=int(rng.integers(2, 40)), replace=False)}
        lower = [int(i) for i in rng.permutation([i for i in free if i not in ties])[:15]]
    else:      # negative scores: every document is listed; the tie takes most, the rest lie lower
        ties = {int(i) for i in free if rng.random() < 0.8} | {int(rng.choice(free[free % 64 == l])) for l in range(64) if l != c}
        lower = [i for i in range(m) if not hot[i] and i not in ties]
    for i in ties:
        sc[i], hot[i] = tie, True
    for i in lower:
        sc[i], hot[i] = tie / 2 if a > 0 else 2 * tie, True
    query = [int(d) for d in rng.permutation(np.nonzero(hot)[0])]
    return [Case("F3b", f"F3b n={n} k={k} seed={seed} column={c}" + (" neg" if a < 0 else ""), n, k, csr_per_document(sc),
                 [query], 0, lows + highs, highs, True)]


def tiny_case(name, k, seed, a, high_vals, above_vals, *, n=TINY, reach=True, low_vals=()):
    """A slab of n <= 64 documents, ALL of them one image run but for Z < k documents above: the run's first L ids score
    a (a = 0.0: untouched), the highest ids score more (high_vals) or less (low_vals).  For images that nothing can lie
    below (-inf) or that untouched documents share (+-0)."""
    rng = np.random.default_rng([seed, k, n, 33])
    assert n <= 64 and k < n
    nh = 1 + int(rng.integers(0, min(4, n - k - 1)))
    nl = int(rng.integers(0, min(3, n - k - nh + 1))) if low_vals else 0
    Z = int(rng.integers(0, min(k, n - k - nh - nl + 1))) if above_vals else 0  # at least k equal scores open the run
    ids = rng.permutation(n)
    above = sorted(int(i) for i in ids[:Z])
    run = sorted(int(i) for i in ids[Z:])
    tail = [int(i) for i in rng.permutation(run[-(nh + nl):])]
    sc = np.full(n, float(a), dtype=np.float64)
    for j, i in enumerate(above):
        sc[i] = above_vals[j % len(above_vals)]
    for j, i in enumerate(tail[:nh]):
        sc[i] = high_vals[j % len(high_vals)]
    for j, i in enumerate(tail[nh:]):
        sc[i] = low_vals[j % len(low_vals)]
    query = [int(d) for d in rng.permutation(n) if sc[d] != 0.0 or np.signbit(sc[d])]
    return Case("F4", f"F4 {name} n={n} k={k} seed={seed}", n, k, csr_per_document(sc), [query], 0, run,
                sorted(tail[:nh]), reach)


def f4(n, k, seed):
    """Scores the fp32 image cannot tell apart because they lie outside its range: +-inf, +-0, subnormal images."""
    out = []
    for sign in (1, -1):
        s = "neg " if sign < 0 else ""
        # images +-inf: 1e300 against 2e300 (the larger is the less negative one below zero)
        if sign > 0:
            out.append(run_case("F4", n, k, seed, VARIANTS[seed % 3], a=1e300, high_vals=[2e300, 1.5e300, 1e301],
                                below=[1.0, 3e38, 0.5], name=f"F4 +inf n={n} k={k} seed={seed}"))
        # subnormal images: a relative 1e-12 apart, and a third of a subnormal step apart
        out.append(run_case("F4", n, k, seed, VARIANTS[(seed + 1) % 3], a=sign * 5 * SUB, below=[sign * SUB * (1 if sign > 0 else 9)],
                            name=f"F4 {s}subnormal n={n} k={k} seed={seed}"))
        out.append(run_case("F4", n, k, seed, VARIANTS[3 + seed % 3], a=sign * 3 * SUB, high_vals=[sign * 3 * SUB + 0.4 * SUB, sign * 3 * SUB + 0.3 * SUB],
                            below=[sign * SUB * (1 if sign > 0 else 9)], name=f"F4 {s}subnormal-wide n={n} k={k} seed={seed}"))
    # images +-0 beside untouched documents at +0.0: more than 64 documents share the image, so this is the overflow
    # branch's mass tie (or, above 64 survivors of a higher image, nothing special); the tiny slabs below reach the check
    rng = np.random.default_rng([seed, n, k, 34])
    sc = np.zeros(n, dtype=np.float64)
    ids = rng.permutation(n)
    sc[ids[:3]], sc[ids[3:6]], sc[ids[6]] = 1e-50, -1e-50, -0.0
    sc[ids[7:7 + int(rng.integers(0, k))]] = 1.0
    query = [int(d) for d in ids[:7 + k]]
    out.append(Case("F4", f"F4 zero-images n={n} k={k} seed={seed}", n, k, csr_per_document(sc), [query], 0,
                    sorted(int(i) for i in np.nonzero(sc != 1.0)[0]), sorted(int(i) for i in ids[:3]), False))
    return [c for c in out if c is not None]


def f4_tiny(k, seed):
    """The same collisions in a slab of 48 documents, where every document survives and the pair check decides."""
    return [
        tiny_case("-inf", k, seed, -2e300, [-1e300, -1.5e300], [1.0, 0.0, -3e38]),
        tiny_case("+inf", k, seed, 1e300, [2e300, 1e301], []),
        tiny_case("zero: 1e-50 above untouched", k, seed, 0.0, [1e-50, 1e-60], [1.0], low_vals=[-1e-50, -0.0]),
        tiny_case("zero: untouched above -1e-50", k, seed, -1e-50, [0.0, 1e-50, -1e-51], [1.0]),
        tiny_case("subnormal", k, seed, 7 * SUB, [7.3 * SUB, 7 * SUB * (1 + REL)], [1.0], low_vals=[6.8 * SUB]),
        tiny_case("neg subnormal", k, seed, -7 * SUB, [-6.8 * SUB, -7 * SUB * (1 - REL)], [1.0, 0.0], low_vals=[-7.3 * SUB]),
    ]


def f5(n, seed, ks, nq):
    """Seeded fuzz: image classes c, c/2, c/4, ... with one to three exact values 1e-12 apart each, placed at random.
    ONE corpus (term d: document d at +value, term n + d: at -value) and, per depth, nq queries as subsets of its terms
    for one search call: a random share of the documents stays at 0, a third of the queries take the negative terms."""
    rng = np.random.default_rng([seed, n, 35])
    c = _exact32(rng)
    ncls = int(rng.choice([1, 2, 4]))
    vals = np.array([c / 2 ** j * (1 + REL * i) for j in range(ncls) for i in range(int(rng.integers(1, 4)))])
    val = rng.choice(vals, size=n)
    csr = make_csr(n, [[d] for d in range(n)] * 2, np.concatenate([val, -val]))
    out = []
    for k in ks:
        queries = []
        for _ in range(nq):
            hot = np.nonzero(rng.random(n) < rng.choice([8.0 / n, 16.0 / n, 0.05, 0.3, 1.0]))[0]
            neg = rng.random() < 1 / 3
            queries.append([int(d) + (n if neg else 0) for d in rng.permutation(hot)])
        out.append(Case("F5", f"F5 n={n} k={k} seed={seed}", n, k, csr, queries))
    return out


def selector_depths(n):
    return [k for k in DEPTHS if selector_runs(n, k) and k < n]


def control_depths(n):
    """k = 64 (every survivor pair is below k: no gap), 65 (arg-max rounds without the selector) and 100 (staged
    selector), asked of data built for a shallower cut."""
    return [k for k in (64, 65, 100) if k < n and (k != 65 or bm_plan(n, k)[2])]


def with_depth(case, k, family):
    return Case(family, case.name + f" asked k={k}", case.n, k, case.csr, case.queries, case.slab_ix, case.run, case.high, False)


def hand_made(seeds=(1, 2)):
    """Every F1-F4 case and the controls: a list of Case."""
    out = []
    for seed in seeds:
        for n in SHAPES:
            for k in selector_depths(n):
                out += f1(n, k, seed) + f2(n, k, seed) + f3a(n, k, seed) + f3b(n, k, seed) + f4(n, k, seed)
            base = f1(n, 10, seed) + f3b(n, 10, seed) + f4(n, 10, seed)[:2]
            out += [with_depth(c, k, "control") for k in control_depths(n) for c in base]
        for n in MULTI:
            nslabs = bm_plan(n, 10)[1]
            for k in (1, 2, 10, 16):
                for six in (0, nslabs // 2, nslabs - 1):
                    out += f1(n, k, seed, six)[seed % 2::2] + f2(n, k, seed, six)[:1]
            out += [with_depth(c, k, "control") for k in (17, 100) for c in f1(n, 10, seed, nslabs - 1)[:2]]
        for k in (1, 2, 10, 16, 17, 40):
            out += f4_tiny(k, seed)
    return out


def fuzz(seed=1, nq=64):
    out = []
    for n in (TINY,) + SHAPES:
        out += f5(n, seed, selector_depths(n) + control_depths(n)[1:], nq)
    return out

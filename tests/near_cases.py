"""Cases of the proximity resolver (amdr_span_lists: csrc/phrase_scope.hip, csrc/near_rule.hpp): small corpora given as one
token SEQUENCE per document (phrase_cases.SeqCorpus), Nears and phrases over them, and the reference — a plain scan of
EVERY window of EVERY document, which shares nothing with near_rule.hpp: no anchors, no driver, no greedy cursor, no slot
mask, no lanes.  numpy only: the CPU test (tests/test_near_scope.py) checks the certificates below — each builder certifies
its own case — and the GPU test (tests/test_near_scope_gpu.py) compares the device lists and the host twin's with
`item_list`.

An ITEM of a call is (kind, term ids, distance): kind 0 a phrase (distance unused), 1 a Near unordered, 2 a Near ordered.
In a constraint (tests/term_scope_cases.py: (groups, base)) the term id n_terms + p names item p of the batch.
"""
from collections import Counter
from itertools import combinations
from typing import Dict, List, Sequence, Tuple

import numpy as np

import phrase_cases as PC
import term_scope_cases as TC
from phrase_cases import SeqCorpus

MUST, ANY, NOT = TC.MUST, TC.ANY, TC.NOT
PHRASE, UNORDERED, ORDERED = 0, 1, 2
TILE, LANES = PC.TILE, PC.LANES
MAX_TERMS, MAX_DIST = 8, 255  # kNearMaxTerms, kNearMaxDist

Item = Tuple[int, List[int], int]


def near(terms: Sequence[int], n: int, ordered: bool = False) -> Item:
    return (ORDERED if ordered else UNORDERED, [int(t) for t in terms], int(n))


def phrase(terms: Sequence[int]) -> Item:
    return (PHRASE, [int(t) for t in terms], 0)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def _subsequence(win: Sequence[int], terms: Sequence[int]) -> bool:
    it = iter(win)
    return all(t in it for t in terms)


def near_holds(seq: Sequence[int], terms: Sequence[int], n: int, ordered: bool) -> bool:
    """Every run of n + 1 consecutive tokens of ONE document (clamped at its end), each checked on its own: the multiset of
    the run covers the multiset of the Near / the Near is a subsequence of the run."""
    want = Counter(terms)
    for s in range(len(seq)):
        win = list(seq[s:s + n + 1])
        if ordered:
            if _subsequence(win, terms):
                return True
        else:
            have = Counter(win)
            if all(have[t] >= c for t, c in want.items()):
                return True
    return False


def near_holds_tuples(seq: Sequence[int], terms: Sequence[int], n: int, ordered: bool) -> bool:
    """The definitions spelt out on position TUPLES (small documents only): ordered — ascending positions that carry the
    terms in order, last - first <= n; unordered — any assignment of distinct positions to the terms, max - min <= n."""
    M = len(terms)
    for pos in combinations(range(len(seq)), M):
        if pos[-1] - pos[0] > n:
            continue
        got = [seq[p] for p in pos]
        if (got == list(terms)) if ordered else (Counter(got) == Counter(terms)):
            return True
    return False


def item_holds(seq: Sequence[int], item: Item) -> bool:
    kind, terms, n = item
    return PC.holds(seq, terms) if kind == PHRASE else near_holds(seq, terms, n, kind == ORDERED)


def item_list(corpus: SeqCorpus, item: Item) -> np.ndarray:
    """The ascending documents that hold the item; empty with an id outside the vocabulary anywhere in it."""
    if any(t < 0 or t >= corpus.n_terms for t in item[1]):
        return np.zeros(0, dtype=np.int32)
    kept = corpus.__dict__.setdefault("_item_lists", {})  # (computed once per corpus object and item, never changed)
    key = (item[0], tuple(item[1]), item[2])
    if key not in kept:
        kept[key] = np.asarray([d for d, seq in enumerate(corpus.docs) if item_holds(seq, item)], dtype=np.int32)
        kept[key].setflags(write=False)
    return kept[key]


def expected_lists(corpus: SeqCorpus, items: Sequence[Item]):
    """(list_ptr i64 [n + 1], docs i32) of a batch of items."""
    lists = [item_list(corpus, it) for it in items]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    return ptr, (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int32)).astype(np.int32)


def driver_len(corpus: SeqCorpus, item: Item) -> int:
    """The item's candidate count by the rule — the smallest document frequency among its tokens; 0 with an unknown one —
    which is also the host's upper bound of its list."""
    return PC.driver_len(corpus, item[1])


def bounds(corpus: SeqCorpus, items: Sequence[Item]):
    """(cand_max, rows_cap) that always suffice: the largest and the sum of the upper bounds."""
    ub = [driver_len(corpus, it) for it in items]
    return max(ub, default=0), int(sum(ub))


def operands(items: Sequence[Item]):
    """(item_ptr i64 [n + 1], item_terms i32, item_kind i32 [n], item_dist i32 [n]) of the ABI."""
    ptr = np.zeros(len(items) + 1, dtype=np.int64)
    np.cumsum([len(it[1]) for it in items], out=ptr[1:])
    return (ptr, np.asarray([t for it in items for t in it[1]], dtype=np.int32),
            np.asarray([it[0] for it in items], dtype=np.int32), np.asarray([it[2] for it in items], dtype=np.int32))


def expected_constraint(corpus: SeqCorpus, con, bases, items) -> np.ndarray:
    """Set algebra over the documents' tokens; a term id >= n_terms names an item of `items`."""
    groups, base = con

    def have(t):
        if 0 <= t < corpus.n_terms:
            return corpus.holders(t)
        p = t - corpus.n_terms
        return {int(d) for d in item_list(corpus, items[p])} if 0 <= p < len(items) else set()
    sat = lambda ids: set.intersection(*[have(t) for t in ids])  # noqa: E731
    out = set(range(corpus.n_docs))
    anys = [sat(ids) for k, ids in groups if k == ANY]
    for k, ids in groups:
        if k == MUST:
            out &= sat(ids)
        elif k == NOT:
            out -= sat(ids)
    if anys:
        out &= set.union(*anys)
    if base >= 0:
        out &= {int(r) for r in bases[base]}
    return np.asarray(sorted(out), dtype=np.int64)


def expected_table(corpus: SeqCorpus, fam: TC.Family, items):
    lists = [expected_constraint(corpus, con, fam.bases, items) for con in fam.cons]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    return ptr, (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64))


def upper_bounds(corpus: SeqCorpus, items) -> np.ndarray:
    """df extended by the items' upper bounds: what the host packer hands to driver_length."""
    return np.concatenate([corpus.df(), np.asarray([driver_len(corpus, it) for it in items], dtype=np.int64)])


# ---- "edge": hand-made documents, one per shape the rule can go wrong at ---------------------------------------------------
A, B, C_, X = 0, 1, 2, 3
E8 = list(range(4, 12))              # eight distinct tokens
P_, Q_, F = 12, 13, 14               # the lane-stride pair and the filler of its documents
U, V, G = 15, 16, 17                 # the long documents' pair and their filler
Y, Z = 18, 19                        # the pair of the exact-distance documents
NONE = 20                            # in no document
EDGE_TERMS = 21
GAPS = (1, 2, 3, 64, 65, 255, 256)   # n and n + 1 for n = 1, 2, 64, 255
DISTANCES = (1, 2, 64, 255)
LONG_LEN = 4550
STRIDE_N = 40                        # the distance of the lane-stride Nears whose partner lies a round further
# (document length, anchor position of P_, position of Q_)
STRIDE_DOCS = ((129, 62, 63), (129, 63, 64), (129, 64, 65), (129, 127, 128), (129, 63, 63 + STRIDE_N),
               (129, 63, 64 + STRIDE_N), (129, 62, 62 + STRIDE_N), (129, 64, 64 + STRIDE_N), (129, 0, 128),
               (63, 61, 62), (64, 62, 63), (65, 63, 64), (127, 62, 126), (128, 63, 127), (128, 127, 64))


def edge_corpus():
    """-> (corpus, {name: document id}).  Every named document is described by its certificate in `edge_certificates`."""
    docs, at = [], {}

    def add(name, seq):
        at[name] = len(docs)
        docs.append(list(seq))
    add("first: a b", [A, B])                                     # document 0
    add("empty", [])
    add("one a", [A])                                             # shorter than any Near; Near(a, a) on one a
    add("boundary left", [B] + [X] * 6 + [A])                     # a and b within 5 only ACROSS this document and the next
    add("boundary right", [B] + [X] * 6 + [A])
    add("clamped at the end", [X, X, X, A, B])
    add("b x a", [B, X, A])                                       # hit unordered, miss ordered
    add("a a b", [A, A, B])                                       # n = 1 ordered: only from the second anchor
    add("a x x b a", [A, X, X, B, A])                             # n = 1 unordered: the window starts at b
    add("a x a", [A, X, A])                                       # Near(a, a, 2): two a, n apart
    add("a x x a", [A, X, X, A])                                  # ... n + 1 apart
    add("a b a", [A, B, A])
    add("a x b x a", [A, X, B, X, A])                             # Near(a, a, b): span 4
    add("b a b a", [B, A, B, A])
    add("eight c", [C_] * 8)
    add("seven c", [C_] * 7)
    add("four c x four c", [C_] * 4 + [X] + [C_] * 4)
    add("eight distinct, reversed", E8[::-1])
    add("eight distinct, one gap", E8[:7] + [X, E8[7]])
    add("seven of eight", E8[:7])
    for g in GAPS:
        add(f"y z {g} apart", [X, Y] + [X] * (g - 1) + [Z, X])
    for n, p, q in STRIDE_DOCS:
        seq = [F] * n
        seq[p], seq[q] = P_, Q_
        add(f"stride len {n} p {p} q {q}", seq)
    add("long", [V] + [G] * 300 + [U] + [G] * (LONG_LEN - 306) + [U, G, G, V])
    add("long none", [V] + [G] * 300 + [U] + [G] * (LONG_LEN - 311) + [U] + [G] * 7 + [V])
    add("last: b a", [B, A])                                      # document n - 1
    return SeqCorpus("near edge", EDGE_TERMS, docs), at


def edge_items() -> List[Item]:
    out = []
    for n in DISTANCES:
        out += [near([Y, Z], n), near([Y, Z], n, True), near([Z, Y], n, True)]
    for n in (1, 2, 3, 5):
        out += [near([A, B], n), near([A, B], n, True), near([B, A], n, True)]
    out += [near([A, A], 1), near([A, A], 2), near([A, A], 3), near([A, A], 2, True),
            near([A, A, B], 2), near([A, A, B], 3), near([A, A, B], 4), near([B, A, A], 3),
            near([A, B, A], 2, True), near([A, B, A], 3, True), near([A, A, B], 2, True),
            near([C_] * 8, 7), near([C_] * 8, 7, True), near([C_] * 8, 8), near([C_] * 8, 6),
            near(E8, 7), near(E8, 7, True), near(E8[::-1], 7, True), near(E8, 8), near(E8, 8, True), near(E8, 6)]
    for n in (1, STRIDE_N, STRIDE_N + 1, 64, 128, 255):
        out += [near([P_, Q_], n), near([P_, Q_], n, True), near([Q_, P_], n, True)]
    out += [near([U, V], 5), near([U, V], 3, True), near([U, V], 2), near([U, V], 255), near([V, U], 255, True)]
    out += [near([A, NONE], 5), near([NONE, A], 5, True)]                          # an empty driver
    for bad in (-1, EDGE_TERMS):                                                   # an id outside the vocabulary, anywhere
        out += [near([bad, A], 2), near([A, bad], 2, True), near([A, bad, B], 2), near([A, B, bad], 2, True)]
    return out


def edge_certificates(corpus: SeqCorpus, at: Dict[str, int]) -> None:
    """What each document of the edge corpus is there for, asserted on the reference; and the reference itself against the
    definitions spelt out on position tuples, for every item on every document short enough to enumerate."""
    d = corpus.docs
    n_docs = corpus.n_docs
    h = lambda name, terms, n, o=False: near_holds(d[at[name]], terms, n, o)  # noqa: E731
    assert at["first: a b"] == 0 and at["last: b a"] == n_docs - 1 and d[at["empty"]] == [] and d[at["one a"]] == [A]
    for n in DISTANCES:  # exactly n apart: hit; n + 1 apart: miss — both forms; the reverse order never
        assert h(f"y z {n} apart", [Y, Z], n) and h(f"y z {n} apart", [Y, Z], n, True)
        assert not h(f"y z {n + 1} apart", [Y, Z], n) and not h(f"y z {n + 1} apart", [Y, Z], n, True)
        assert h(f"y z {n} apart", [Z, Y], n) and not h(f"y z {n} apart", [Z, Y], n, True)
    le, ri = at["boundary left"], at["boundary right"]
    assert ri == le + 1 and not near_holds(d[le], [A, B], 5, False) and not near_holds(d[ri], [A, B], 5, False)
    assert near_holds(d[le] + d[ri], [A, B], 1, True) and {A, B} <= set(d[le]) and {A, B} <= set(d[ri])  # only across it
    assert h("clamped at the end", [A, B], 5) and len(d[at["clamped at the end"]]) == 5
    assert not h("one a", [A, A], 3) and not h("one a", [A, A], 2, True)
    assert h("b x a", [A, B], 2) and not h("b x a", [A, B], 2, True) and not h("b x a", [A, B], 1)
    assert h("a a b", [A, B], 1, True) and d[at["a a b"]][0] == A and d[at["a a b"]][:2] == [A, A]
    assert h("a x x b a", [A, B], 1) and not h("a x x b a", [A, B], 1, True) and h("a x x b a", [A, B], 3, True)
    assert h("a x a", [A, A], 2) and not h("a x a", [A, A], 1) and not h("a x x a", [A, A], 2) and h("a x x a", [A, A], 3)
    assert h("a b a", [A, A, B], 2) and not h("a x b x a", [A, A, B], 3) and h("a x b x a", [A, A, B], 4)
    assert not h("first: a b", [A, A, B], 4)  # one a is not two
    assert h("eight c", [C_] * 8, 7) and not h("seven c", [C_] * 8, 7) and not h("eight c", [C_] * 8, 6)
    assert not h("four c x four c", [C_] * 8, 7) and h("four c x four c", [C_] * 8, 8)
    assert h("eight distinct, reversed", E8, 7) and not h("eight distinct, reversed", E8, 7, True)
    assert h("eight distinct, reversed", E8[::-1], 7, True)
    assert not h("eight distinct, one gap", E8, 7) and h("eight distinct, one gap", E8, 8, True)
    assert not h("seven of eight", E8, 255)
    assert h("a b a", [A, B, A], 2, True) and not h("a a b", [A, B, A], 3, True) and h("b a b a", [A, B, A], 2, True)
    for n, p, q in STRIDE_DOCS:
        seq = d[at[f"stride len {n} p {p} q {q}"]]
        assert len(seq) == n and seq.count(P_) == 1 and seq.count(Q_) == 1 and seq.index(P_) == p and seq.index(Q_) == q
        gap = abs(q - p)
        assert near_holds(seq, [P_, Q_], gap, False) and (gap == 1 or not near_holds(seq, [P_, Q_], gap - 1, False))
        assert near_holds(seq, [P_, Q_], gap, True) == (q > p)
    # the lane stride's edges: an anchor in lane 62 / 63 of the first round, lane 0 / 63 of the second, and partners in the
    # next round's range (63 -> 64, 63 -> 63 + n; 63 + n + 1 is the miss)
    pairs = {(p, q) for _, p, q in STRIDE_DOCS}
    assert {(62, 63), (63, 64), (64, 65), (127, 128), (63, 63 + STRIDE_N), (63, 64 + STRIDE_N)} <= pairs
    assert {n for n, _, _ in STRIDE_DOCS} == {63, 64, 65, 127, 128, 129}
    long_, none = d[at["long"]], d[at["long none"]]
    assert len(long_) == LONG_LEN == len(none)
    assert near_holds(long_, [U, V], 3, True) and not near_holds(long_[:-1], [U, V], 255, False)  # only in the last tokens
    assert not near_holds(none, [U, V], 5, False) and {U, V} <= set(none) and near_holds(none, [U, V], 8, True)
    for it in edge_items():
        for seq in d:
            if len(seq) <= 9 and it[0] != PHRASE:
                assert near_holds(seq, it[1], it[2], it[0] == ORDERED) == near_holds_tuples(seq, it[1], it[2], it[0] == ORDERED)
    # a Near is neither its conjunction nor its phrase
    assert PC.phrase_list(corpus, [A, B]).size < item_list(corpus, near([A, B], 1)).size < PC.conjunction(corpus, [A, B]).size
    assert driver_len(corpus, near([A, NONE], 5)) == 0


# ---- "tiles": drivers of exactly 0 / 1 / 255 / 256 / 257 / 513 candidates (phrase_cases.tiles_corpus) ----------------------
DRIVER_LENGTHS = PC.DRIVER_LENGTHS


def tiles_items() -> List[Item]:
    """Per driver length the rare term next to the common one: unordered at distance 1, then ordered at distance 1."""
    return ([near([PC.T_RARE[m], PC.T_COMMON], 1) for m in DRIVER_LENGTHS]
            + [near([PC.T_RARE[m], PC.T_COMMON], 1, True) for m in DRIVER_LENGTHS])


def tiles_certificates(corpus: SeqCorpus) -> None:
    assert DRIVER_LENGTHS == (0, 1, 255, 256, 257, 513)
    items = tiles_items()
    for m, it in zip(DRIVER_LENGTHS * 2, items):
        assert driver_len(corpus, it) == m
        got = item_list(corpus, it)
        assert (got.size == m == 0) or (m == 1 and got.size == 1) or 0 < got.size < m  # kept and dropped candidates
    for it in (items[len(DRIVER_LENGTHS) - 1], items[-1]):
        longest = item_list(corpus, it)
        assert longest[0] == 0 and longest[-1] == corpus.n_docs - 1  # documents 0 and n - 1 among the kept


# ---- "rand": phrase_cases' 700 random documents; 65 items, Nears mixed with phrases ----------------------------------------
def rand_items(corpus: SeqCorpus, count: int = 65) -> List[Item]:
    """Every third item a phrase of phrase_cases.rand_phrases; the others Nears of 2 to 8 tokens drawn from a document's
    window (shuffled for the unordered form) or at random, at distances 1 to 12 and now and then 255."""
    rng = np.random.default_rng(11)
    phrases = PC.rand_phrases(corpus, count)
    out, seen = [], set()
    while len(out) < count:
        k = len(out)
        if k % 3 == 0:
            it = phrase(phrases[k])
        else:
            M = MAX_TERMS if k % 10 == 4 else int(rng.integers(5, MAX_TERMS)) if k % 5 == 4 else int(rng.integers(2, 5))
            n = MAX_DIST if k % 13 == 7 else int(rng.integers(1, 13))
            ordered = bool(k % 2)
            if k % 7 == 5:
                terms = rng.integers(0, corpus.n_terms, size=M).tolist()
            else:
                seq = corpus.docs[int(rng.integers(0, corpus.n_docs))]
                if len(seq) < M:
                    continue
                s = int(rng.integers(0, len(seq) - M + 1))
                win = seq[s:s + max(M, min(n + 1, 2 * M))]
                pick = sorted(rng.choice(len(win), size=M, replace=False).tolist())
                terms = [win[i] for i in pick]
                if not ordered:
                    terms = rng.permutation(terms).tolist()
            it = near(terms, n, ordered)
        key = (it[0], tuple(it[1]), it[2])
        if key not in seen:
            seen.add(key)
            out.append(it)
    return out


def rand_certificates(corpus: SeqCorpus, items) -> None:
    sizes = [item_list(corpus, it).size for it in items]
    conj = [PC.conjunction(corpus, it[1]).size for it in items]
    kinds = Counter(it[0] for it in items)
    assert len(items) == 65 and min(kinds.values()) >= 15 and min(sizes) == 0 and max(sizes) > TILE
    assert sum(1 for it, s, c in zip(items, sizes, conj) if it[0] != PHRASE and 0 < s < c) > 15  # Near is not conjunction
    assert any(len(it[1]) == MAX_TERMS for it in items) and any(len(set(it[1])) < len(it[1]) for it in items if it[0] != PHRASE)
    assert max(driver_len(corpus, it) for it in items) > 2 * TILE


def identity_terms(corpus: SeqCorpus) -> List[List[int]]:
    """Token lists without a repeat: pairs and triples of the most frequent terms, and a pair with a rare one."""
    order = [int(x) for x in np.argsort(-corpus.df())]
    return [[order[0], order[1]], [order[1], order[0]], [order[2], order[0]], [order[0], order[-1]],
            [order[0], order[1], order[2]], [order[3], order[1], order[0], order[2]]]


def scope_family(corpus: SeqCorpus):
    """phrase_cases.scope_family over `scope_items`: an item as MUST and driver; as MUST beside a rarer plain term (not the
    driver); two items as MUST; as ANY next to a plain group; as NOT; inside a tuple group; an id past the virtual lists;
    the first three again inside a base scope."""
    return PC.scope_family(corpus, None)


def scope_items(corpus: SeqCorpus) -> List[Item]:
    """A Near ordered, a Near unordered and a phrase — the three kinds in one list array — of the most frequent terms."""
    order = np.argsort(-corpus.df())
    a, b, c = (int(x) for x in order[:3])
    return [near([a, b], 2, True), near([c, b, a], 6), phrase([a, a, c])]


def scope_certificates(corpus: SeqCorpus, fam: TC.Family, items) -> None:
    lists = [item_list(corpus, it) for it in items]
    assert all(x.size > TILE for x in lists[:2]) and lists[2].size > 0
    ub = upper_bounds(corpus, items)
    V_ = corpus.n_terms
    rare = int(np.argmin(corpus.df()))
    assert ub[rare] < lists[1].size and ub[V_ + 0] > lists[0].size  # a plain term drives constraint 1; a bound is no length
    sizes = [expected_constraint(corpus, con, fam.bases, items).size for con in fam.cons]
    assert sizes[8] == 0 and all(s > 0 for i, s in enumerate(sizes) if i != 8)
    assert sizes[0] < PC.conjunction(corpus, items[0][1]).size

"""Cases of the union step (csrc/union_lists.hip, csrc/union_rule.hpp) and of the term step over its lists: synthetic
posting corpora, union items over them, and the reference — a Python `set` union over the documents' tokens, which shares
nothing with the rule header (no tile, no bitmap, no binary search).  numpy only, in the manner of near_cases.py: the CPU test
(tests/test_union_lists.py) checks the certificates below — each builder certifies its own case — and the GPU test
(tests/test_union_lists_gpu.py) compares the device lists and the host twin's with `item_list`.

A union item is a list of term ids; an id outside [0, n_terms) names a token no document holds.  In a constraint
(tests/term_scope_cases.py: (groups, base)) the term id n_terms + k names virtual list k of the call: the span step's lists
first, the unions behind them.
"""
from typing import Dict, List, Sequence

import numpy as np

import phrase_cases as PC
import term_scope_cases as TC

MUST, ANY, NOT = TC.MUST, TC.ANY, TC.NOT
THREADS = 256  # threads of a block (kUnThreads): an item of more terms than this makes the waves go round


class SetCorpus(TC.Corpus):
    """term_scope_cases.Corpus with the documents inverted once (the edge corpora have hundreds of terms)."""

    def holders(self, t: int) -> set:
        kept = self.__dict__.get("_inverted")
        if kept is None:
            kept = self.__dict__["_inverted"] = [set() for _ in range(self.n_terms)]
            for d, have in enumerate(self.docs):
                for x in have:
                    kept[x].add(d)
        return kept[t]


# ---- the reference ---------------------------------------------------------------------------------------------------------
def item_list(corpus, item: Sequence[int]) -> np.ndarray:
    """The ascending documents that hold at least one of the item's tokens."""
    out = set()
    for t in item:
        if 0 <= t < corpus.n_terms:
            out |= corpus.holders(int(t))
    return np.asarray(sorted(out), dtype=np.int32)


def expected_lists(corpus, items, before=None):
    """(list_ptr i64 [n + 1], docs i32) of a batch of items; `before` = (list_ptr, docs): the array they continue."""
    lists = [item_list(corpus, it) for it in items]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    docs = (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int32)).astype(np.int32)
    if before is not None:
        ptr = np.concatenate([before[0], before[0][-1] + ptr[1:]])
        docs = np.concatenate([before[1], docs]).astype(np.int32)
    return ptr, docs


def upper_bound(corpus, item) -> int:
    """What a host packer knows: min(n_docs, the sum of the document frequencies of the item's distinct known ids)."""
    df = corpus.df()
    return min(corpus.n_docs, int(sum(df[t] for t in {int(t) for t in item} if 0 <= t < corpus.n_terms)))


def rows_cap(corpus, items) -> int:
    return sum(upper_bound(corpus, it) for it in items)


def operands(items):
    """(item_ptr i64 [n + 1], item_terms i32) of the ABI."""
    ptr = np.zeros(len(items) + 1, dtype=np.int64)
    np.cumsum([len(it) for it in items], out=ptr[1:])
    return ptr, np.asarray([t for it in items for t in it], dtype=np.int32)


# ---- "edge": n documents, for n around the word and the tile --------------------------------------------------------------
E_ALL, E_MARKS, E_STRADDLE, E_EVEN, E_THIRD, E_SIXTH, E_EVEN2, E_ODD, E_NONE = range(9)
E_SPARSE = 9         # the first of 300 sparse terms
E_TERMS = E_SPARSE + 300


def edge_sizes(tile: int):
    return (1, 31, 32, 33, tile - 1, tile, tile + 1, 3 * tile + 1)


def edge_corpus(n: int, tile: int) -> SetCorpus:
    """Term by term: every document (df = n) | documents 0, tile - 1, tile and n - 1 | the six documents around the first
    tile boundary (a list that straddles it) | the even documents | every third | every sixth (nested in both) | the even
    ones again (an identical list) | the odd ones (disjoint from the even) | none | 300 sparse terms of three documents."""
    inside = lambda xs: sorted({int(x) for x in xs if 0 <= x < n})  # noqa: E731
    lists = [range(n), inside([0, tile - 1, tile, n - 1]), inside(range(tile - 3, tile + 3)), range(0, n, 2), range(0, n, 3),
             range(0, n, 6), range(0, n, 2), range(1, n, 2), []]
    for j in range(300):
        lists.append(inside([j * 7919 % n, (j * 104729 + 5) % n, n - 1 - j * 31 % n]))
    docs = [set() for _ in range(n)]
    for t, x in enumerate(lists):
        for d in x:
            docs[d].add(t)
    return SetCorpus(f"edge-{n}", n, E_TERMS, [frozenset(h) for h in docs])


def edge_items(corpus) -> Dict[str, List[int]]:
    V = corpus.n_terms
    return {
        "one term": [E_MARKS], "two identical ids": [E_THIRD, E_THIRD], "identical lists": [E_EVEN, E_EVEN2],
        "disjoint": [E_EVEN, E_ODD], "nested": [E_THIRD, E_SIXTH], "overlapping": [E_THIRD, E_EVEN],
        "300 terms": list(range(E_SPARSE, E_SPARSE + 300)), "no term": [], "unknown -1": [-1], "unknown n_terms": [V],
        "unknown ids": [-1, V, 2**31 - 1], "mixed": [-1, E_THIRD, V, E_MARKS], "every document": [E_ALL],
        "straddle": [E_STRADDLE], "marks and straddle": [E_MARKS, E_STRADDLE], "empty list": [E_NONE, E_NONE],
    }


def edge_certificates(corpus, tile: int) -> None:
    """What each term and item of an edge corpus is there for, asserted."""
    n, df, items = corpus.n_docs, corpus.df(), edge_items(corpus)
    L = {name: item_list(corpus, it) for name, it in items.items()}
    assert df[E_ALL] == n and df[E_NONE] == 0 and len(items["300 terms"]) > THREADS
    assert set(L["one term"].tolist()) == {d for d in (0, tile - 1, tile, n - 1) if d < n} == corpus.holders(E_MARKS)
    if n > tile:  # the straddling list has postings on both sides of the boundary, next to each other
        s = L["straddle"]
        assert s.tolist() == [d for d in range(tile - 3, tile + 3) if d < n] and s[0] < tile <= s[-1]
    assert np.array_equal(L["two identical ids"], np.arange(0, n, 3))
    assert np.array_equal(L["identical lists"], np.arange(0, n, 2)) and corpus.holders(E_EVEN) == corpus.holders(E_EVEN2)
    assert np.array_equal(L["disjoint"], np.arange(n)) and not corpus.holders(E_EVEN) & corpus.holders(E_ODD)
    assert np.array_equal(L["nested"], np.arange(0, n, 3)) and corpus.holders(E_SIXTH) <= corpus.holders(E_THIRD)
    for name in ("no term", "unknown -1", "unknown n_terms", "unknown ids", "empty list"):
        assert L[name].size == 0, name
    assert np.array_equal(L["mixed"], item_list(corpus, [E_THIRD, E_MARKS])) and np.array_equal(L["every document"], np.arange(n))
    assert L["every document"][0] == 0 and L["every document"][-1] == n - 1
    if n > 3:  # merged, not concatenated: smaller than the sum of the lists, larger than the longest
        assert max(df[E_THIRD], df[E_EVEN]) < L["overlapping"].size < df[E_THIRD] + df[E_EVEN]
        assert upper_bound(corpus, items["overlapping"]) == min(n, df[E_THIRD] + df[E_EVEN]) >= L["overlapping"].size
    many = L["300 terms"]
    assert 0 < many.size <= 900 and np.all(np.diff(many) > 0)
    if n >= 3 * tile:
        assert len({int(d) // tile for d in many}) == 4  # the sparse terms reach every tile
    for name, lst in L.items():
        assert lst.size <= upper_bound(corpus, items[name]), name


def batch(corpus, count: int) -> List[List[int]]:
    """`count` items of an edge corpus: the named ones first, then random picks of 0 to 6 ids, unknown ones among them."""
    items = list(edge_items(corpus).values())
    rng = np.random.default_rng(1000 + count)
    while len(items) < count:
        ids = rng.integers(-1, corpus.n_terms + 2, size=int(rng.integers(0, 7))).tolist()
        items.append([int(t) for t in ids])
    return items[:count]


# ---- "rand" (phrase_cases.rand_corpus: token sequences, so that a span step can stand in front) ------------------------------
def chain_unions(corpus) -> List[List[int]]:
    """Four unions over the "rand" corpus: the two most frequent terms; the two rarest; three of the middle; one with an
    unknown id."""
    order = [int(t) for t in np.argsort(-corpus.df())]
    return [order[:2], order[-2:], order[4:7], [order[-1], -1, order[3]]]


def scope_family(corpus):
    """Constraints in the shape of phrase_cases.scope_family over the lists [phrase, union 0 .. union 3] (`scope_lists`):
    a union as MUST and driver; as MUST beside a rarer plain term; as ANY; as NOT; inside a tuple group next to a phrase;
    two unions as MUST; an id past the lists; inside a base scope (as the driver's rival and beside a phrase)."""
    V = corpus.n_terms
    rare, common = int(np.argmin(corpus.df())), int(np.argmax(corpus.df()))
    base_short = np.arange(0, corpus.n_docs, 9, dtype=np.int64)
    base_long = np.arange(2, corpus.n_docs, dtype=np.int64)
    c = TC.c
    cons = [c([(MUST, [V + 2])]), c([(MUST, [V + 1]), (MUST, [rare])]), c([(MUST, [common]), (ANY, [V + 2]), (ANY, [rare])]),
            c([(MUST, [common]), (NOT, [V + 2])]), c([(MUST, [V + 0, V + 3])]), c([(MUST, [V + 2]), (MUST, [V + 3])]),
            c([(MUST, [V + 5])]), c([(NOT, [V + 4, V + 0])]),
            c([(MUST, [V + 2])], 0), c([(MUST, [V + 1])], 1), c([(MUST, [V + 0]), (ANY, [V + 3]), (ANY, [V + 4])], 1)]
    return TC.Family("unions in constraints", "rand", cons, [base_short, base_long])


def scope_lists(corpus):
    """(the phrases of the span step in front, the unions behind them)."""
    return [PC.scope_phrases(corpus)[0]], chain_unions(corpus)


def expected_constraint(corpus, con, bases, phrases, unions) -> np.ndarray:
    """Set algebra over the documents' tokens; the id n_terms + k names phrase k, then union k - len(phrases)."""
    groups, base = con

    def have(t):
        if 0 <= t < corpus.n_terms:
            return corpus.holders(t)
        k = t - corpus.n_terms
        if 0 <= k < len(phrases):
            return {int(d) for d in PC.phrase_list(corpus, phrases[k])}
        k -= len(phrases)
        return {int(d) for d in item_list(corpus, unions[k])} if 0 <= k < len(unions) else set()
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


def expected_table(corpus, fam, phrases, unions):
    lists = [expected_constraint(corpus, con, fam.bases, phrases, unions) for con in fam.cons]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    return ptr, (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64))


def list_bounds(corpus, phrases, unions) -> np.ndarray:
    """df extended by the upper bounds of the virtual lists: what the host packer hands to driver_length."""
    return np.concatenate([corpus.df(), np.asarray([PC.driver_len(corpus, p) for p in phrases]
                                                   + [upper_bound(corpus, u) for u in unions], dtype=np.int64)])


def scope_certificates(corpus, fam, phrases, unions) -> None:
    df, V = corpus.df(), corpus.n_terms
    rare = int(np.argmin(df))
    lists = [item_list(corpus, u) for u in unions]
    ub = list_bounds(corpus, phrases, unions)
    assert ub[rare] < lists[0].size                       # the plain term drives constraint 1, the union does not
    for u, lst in zip(unions, lists):                     # merged: below the bound unless the lists are disjoint
        assert max(df[t] for t in u if t >= 0) <= lst.size <= upper_bound(corpus, u)
    assert lists[0].size < df[unions[0][0]] + df[unions[0][1]]
    sizes = [expected_constraint(corpus, con, fam.bases, phrases, unions).size for con in fam.cons]
    assert sizes[6] == 0 and all(s > 0 for i, s in enumerate(sizes) if i != 6), sizes
    both = set(PC.phrase_list(corpus, phrases[0]).tolist()) & set(lists[2].tolist())
    assert sizes[4] == len(both) < min(PC.phrase_list(corpus, phrases[0]).size, lists[2].size)  # the tuple group cuts both

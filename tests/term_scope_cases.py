"""Cases of the term-constraint resolver (csrc/term_scope.hip, csrc/term_scope_rule.hpp): small corpora given as one token
set per document, batches of constraints over them, and the reference — Python set algebra over the per-document token
sets, which shares nothing with the rule header (no posting list, no driver, no binary search).  numpy only: the CPU test
(tests/test_term_scope.py) checks the certificates below, the GPU test (tests/test_term_scope_gpu.py) compares the device
table and the host twin's table with `expected`.

A constraint is (groups, base): groups = [(kind, [term ids])], kind 0 MUST / 1 ANY / 2 NOT; base = an index into the
batch's base scopes or -1.  A document satisfies a group when it holds every term of it; -1 is in no document.
"""
from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Tuple

import numpy as np

MUST, ANY, NOT = 0, 1, 2
TILE = 1024

# ---- corpora -----------------------------------------------------------------------------------------------------------
# BIG: 4 100 documents, 24 terms.  Term t's documents, by design:
BIG_N = 4100
T_ALL, T_NONE, T_ENDS, T_ONE = 0, 1, 2, 3          # every document | none (an empty list) | {0, n - 1} | {7}
T_1023, T_1024, T_1025, T_2049 = 4, 5, 6, 7         # lists of exactly these lengths (the tile edges)
T_TIE_A, T_TIE_B = 8, 9                             # two lists of 500 documents each
T_RANDOM = range(10, 24)                            # densities from 0.6 down to 0.01


@dataclass
class Corpus:
    name: str
    n_docs: int
    n_terms: int
    docs: List[frozenset]  # per document: the term ids it holds

    def postings(self):
        """(term_ptr i64, post_doc i32, post_tf i32, idf f64, doc_len i32, avgdl): the arrays BM25Index takes.  tf = 1;
        the idf values are arbitrary finite numbers (no score is compared here)."""
        lists = [[] for _ in range(self.n_terms)]
        for d, have in enumerate(self.docs):
            for t in sorted(have):
                lists[t].append(d)
        term_ptr = np.zeros(self.n_terms + 1, dtype=np.int64)
        np.cumsum([len(x) for x in lists], out=term_ptr[1:])
        post_doc = np.asarray([d for x in lists for d in x], dtype=np.int32)
        doc_len = np.asarray([max(len(h), 1) for h in self.docs], dtype=np.int32)
        idf = np.linspace(0.5, 3.0, self.n_terms)
        return term_ptr, post_doc, np.ones_like(post_doc), idf, doc_len, float(doc_len.mean())

    def holders(self, t: int) -> set:
        """The documents whose token set holds term t (kept per term: the families ask for the same terms again)."""
        kept = self.__dict__.setdefault("_holders", {})
        if t not in kept:
            kept[t] = {d for d, have in enumerate(self.docs) if t in have}
        return kept[t]

    def df(self) -> np.ndarray:
        out = np.zeros(self.n_terms, dtype=np.int64)
        for have in self.docs:
            for t in have:
                out[t] += 1
        return out


def _from_lists(name: str, n: int, lists: Sequence[Sequence[int]]) -> Corpus:
    docs = [set() for _ in range(n)]
    for t, x in enumerate(lists):
        for d in x:
            docs[int(d)].add(t)
    return Corpus(name, n, len(lists), [frozenset(h) for h in docs])


def big_corpus() -> Corpus:
    rng = np.random.default_rng(417)
    n = BIG_N
    pick = lambda m: np.sort(rng.choice(n, size=m, replace=False))  # noqa: E731
    lists = [np.arange(n), [], [0, n - 1], [7], pick(1023), pick(1024), pick(1025), pick(2049), pick(500), pick(500)]
    for j, _ in enumerate(T_RANDOM):
        dens = 0.6 * (0.01 / 0.6) ** (j / (len(T_RANDOM) - 1))
        lists.append(np.flatnonzero(rng.random(n) < dens))
    return _from_lists("big", n, lists)


def iota_corpus(n: int) -> Corpus:
    """n documents, 4 terms: 0 every document, 1 the even ones, 2 {n - 1}, 3 none."""
    return _from_lists(f"iota-{n}", n, [np.arange(n), np.arange(0, n, 2), [n - 1], []])


# ---- constraints -------------------------------------------------------------------------------------------------------
Constraint = Tuple[List[Tuple[int, List[int]]], int]


@dataclass
class Family:
    name: str
    corpus: str                       # "big", "iota-1", "iota-1024", "iota-1025"
    cons: List[Constraint]
    bases: List[np.ndarray] = field(default_factory=list)


def c(groups, base=-1) -> Constraint:
    return [(int(k), [int(t) for t in ids]) for k, ids in groups], int(base)


def _random_constraints(count: int, seed: int) -> List[Constraint]:
    rng = np.random.default_rng(seed)
    terms = list(T_RANDOM) + [T_1023, T_2049, T_TIE_A]
    out = []
    for _ in range(count):
        groups = [(MUST, list(rng.choice(terms, size=int(rng.integers(1, 3)), replace=False)))]
        for kind in (ANY, ANY, NOT):
            if rng.random() < 0.5:
                groups.append((kind, list(rng.choice(terms, size=int(rng.integers(1, 3))))))
        out.append(c(groups))
    return out


def families() -> List[Family]:
    n = BIG_N
    every, evens = np.arange(n, dtype=np.int64), np.arange(0, n, 2, dtype=np.int64)
    short = np.asarray([0, 5, 7, 1000, n - 1], dtype=np.int64)          # shorter than every list below but T_ONE's
    long_ = np.arange(3, n - 3, dtype=np.int64)                         # longer than every list
    tie = np.arange(100, 600, dtype=np.int64)                           # as long as T_TIE_A's list: the base drives
    r0 = T_RANDOM[0]
    rare = T_RANDOM[-1]
    sixty5 = _random_constraints(65, 5)
    return [
        # driver lengths 0, 1, 1 023, 1 024, 1 025, 2 049 (the second group keeps a part of each driver)
        Family("driver lengths", "big", [c([(MUST, [T_NONE])]), c([(MUST, [T_ONE])]), c([(MUST, [T_1023]), (NOT, [r0])]),
                                         c([(MUST, [T_1024]), (ANY, [r0])]), c([(MUST, [T_1025]), (NOT, [r0 + 1])]),
                                         c([(MUST, [T_2049]), (ANY, [r0 + 2])]), c([(MUST, [T_1024])])]),
        # candidates at document 0 and at n - 1
        Family("first and last document", "big", [c([(MUST, [T_ENDS])]), c([(MUST, [T_ENDS]), (NOT, [T_ONE])]),
                                                   c([(MUST, [T_ALL]), (ANY, [T_ENDS])])]),
        Family("one constraint", "big", sixty5[:1]),
        Family("two constraints", "big", sixty5[:2]),
        Family("65 constraints", "big", sixty5),
        Family("MUST only", "big", [c([(MUST, [r0])]), c([(MUST, [r0 + 3]), (MUST, [r0 + 1])])]),
        Family("ANY only", "big", [c([(ANY, [rare])]), c([(ANY, [rare]), (ANY, [T_ONE]), (ANY, [T_ENDS])])]),
        Family("NOT only", "big", [c([(NOT, [r0])]), c([(NOT, [r0]), (NOT, [r0 + 1])])]),
        Family("all three", "big", [c([(MUST, [r0 + 2]), (ANY, [r0 + 4]), (ANY, [r0 + 5]), (NOT, [r0 + 3])]),
                                    c([(MUST, [T_2049]), (MUST, [r0]), (ANY, [T_1023]), (NOT, [T_1025])])]),
        Family("multi-token groups", "big", [c([(MUST, [r0, r0 + 1])]), c([(MUST, [r0]), (ANY, [r0 + 2, r0 + 3]), (ANY, [rare, r0])]),
                                             c([(MUST, [T_2049]), (NOT, [r0, r0 + 1, r0 + 2])])]),
        Family("a repeated term", "big", [c([(MUST, [r0 + 4, r0 + 4])]), c([(MUST, [r0 + 4]), (MUST, [r0 + 4])]),
                                          c([(MUST, [T_1025]), (ANY, [r0, r0]), (NOT, [r0 + 1, r0 + 1])])]),
        # -1: in a MUST group (empty), in an ANY group (ignored unless all are unknown), in a NOT group (ignored)
        Family("unknown terms", "big", [c([(MUST, [r0 + 4, -1])]), c([(MUST, [r0 + 4]), (ANY, [-1]), (ANY, [r0])]),
                                        c([(MUST, [r0 + 4]), (ANY, [-1]), (ANY, [-1, r0])]), c([(MUST, [r0 + 4]), (NOT, [-1])]),
                                        c([(MUST, [r0 + 4]), (NOT, [r0, -1])]), c([(MUST, [r0 + 4])])]),
        # base scope shorter and longer than the rarest list, a base alone, an empty base
        Family("base scopes", "big", [c([(MUST, [T_1023])], 0), c([(MUST, [T_1023])], 1), c([(MUST, [T_1023])], 2), c([], 2),
                                      c([(NOT, [r0])], 3), c([(ANY, [r0 + 1])], 0), c([(MUST, [T_ALL])], 4)],
               [short, long_, evens, every, np.zeros(0, dtype=np.int64)]),
        # ties: two lists of one length (the first named drives), a base as long as the list (the base drives)
        Family("driver ties", "big", [c([(MUST, [T_TIE_A]), (MUST, [T_TIE_B])]), c([(MUST, [T_TIE_B]), (MUST, [T_TIE_A])]),
                                      c([(MUST, [T_TIE_A])], 0), c([(MUST, [T_TIE_A]), (NOT, [r0])], 0)], [tie]),
        # the iota form (no MUST term, no base): candidates 0 .. n - 1
        Family("iota n=1", "iota-1", [c([(ANY, [0])]), c([(NOT, [3])]), c([(NOT, [0])]), c([(ANY, [2])])]),
        Family("iota n=1024", "iota-1024", [c([(ANY, [1])]), c([(NOT, [1])]), c([(ANY, [2]), (ANY, [3])]), c([(NOT, [3])])]),
        Family("iota n=1025", "iota-1025", [c([(ANY, [1])]), c([(NOT, [1])]), c([(ANY, [2]), (ANY, [3])]), c([(NOT, [2])])]),
    ]


def corpora() -> Dict[str, Corpus]:
    return {"big": big_corpus(), "iota-1": iota_corpus(1), "iota-1024": iota_corpus(1024), "iota-1025": iota_corpus(1025)}


# ---- the reference: set algebra over the per-document token sets -------------------------------------------------------
def expected(corpus: Corpus, con: Constraint, bases: Sequence[np.ndarray]) -> np.ndarray:
    groups, base = con
    holders = corpus.holders  # (-1 is in no document's set)
    sat = lambda ids: set.intersection(*[holders(t) for t in ids])  # noqa: E731
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


def expected_table(corpus: Corpus, fam: Family):
    """(scope_ptr i64 [n_cons + 1], rows i64) of a family."""
    lists = [expected(corpus, con, fam.bases) for con in fam.cons]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    return ptr, (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64))


def doc_qualifies(d: int, have: frozenset, con: Constraint, base_set) -> bool:
    """The rule on ONE document, written out (the certificate that `expected` is what the issue's semantics say)."""
    groups, _ = con
    sat = lambda ids: all(t in have for t in ids)  # noqa: E731
    if not all(sat(ids) for k, ids in groups if k == MUST):
        return False
    anys = [ids for k, ids in groups if k == ANY]
    if anys and not any(sat(ids) for ids in anys):
        return False
    if any(sat(ids) for k, ids in groups if k == NOT):
        return False
    return base_set is None or d in base_set


def operands(fam: Family):
    """The seven operand arrays of the ABI (BM25Index.TERM_OPS order) of a family."""
    grp_ptr, grp_kind, grp_term_ptr, grp_terms, cons_base = [0], [], [0], [], []
    for groups, base in fam.cons:
        for k, ids in groups:
            grp_kind.append(k)
            grp_terms.extend(ids)
            grp_term_ptr.append(len(grp_terms))
        grp_ptr.append(len(grp_kind))
        cons_base.append(base)
    base_ptr = np.zeros(len(fam.bases) + 1, dtype=np.int64)
    if fam.bases:
        np.cumsum([b.size for b in fam.bases], out=base_ptr[1:])
    base_rows = np.concatenate(fam.bases).astype(np.int64) if fam.bases else np.zeros(0, dtype=np.int64)
    return (np.asarray(grp_ptr, np.int64), np.asarray(grp_kind, np.int32), np.asarray(grp_term_ptr, np.int64),
            np.asarray(grp_terms, np.int32), base_ptr, base_rows, np.asarray(cons_base, np.int32))

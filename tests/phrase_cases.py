"""Cases of the phrase resolver (csrc/phrase_scope.hip, csrc/phrase_rule.hpp) and of the term step over its lists
(csrc/term_scope.hip with virtual posting lists): small corpora given as one token SEQUENCE per document, phrases and
constraints over them, and the reference — a plain Python window scan plus set algebra, which shares nothing with the rule
headers (no posting list, no driver, no binary search, no lanes).  numpy only: the CPU test (tests/test_phrase_scope.py)
checks the certificates below — each builder certifies its own case, e.g. that conjunction and phrase differ — and the GPU
test (tests/test_phrase_scope_gpu.py) compares the device lists and the host twin's with `phrase_list`.

A phrase is a list of term ids.  In a constraint (tests/term_scope_cases.py: (groups, base)) the term id n_terms + p names
phrase p of the batch: a document holds it when the phrase stands in its sequence.
"""
from dataclasses import dataclass
from typing import Dict, List, Sequence

import numpy as np

import term_scope_cases as TC

MUST, ANY, NOT = TC.MUST, TC.ANY, TC.NOT
TILE = 256      # candidates per block (kPhTile)
LANES = 64      # start positions per round of a document's scan (kPhLanes)
MAX_LEN = 16    # kPhMaxLen


@dataclass
class SeqCorpus:
    name: str
    n_terms: int
    docs: List[List[int]]  # per document: its term ids in text order

    @property
    def n_docs(self) -> int:
        return len(self.docs)

    def postings(self):
        """(term_ptr i64, post_doc i32, post_tf i32, idf f64, doc_len i32, avgdl): the arrays BM25Index takes; doc_len is
        the true token count (0 for an empty document); the idf values are arbitrary finite numbers."""
        lists = [[] for _ in range(self.n_terms)]
        tfs = [[] for _ in range(self.n_terms)]
        for d, seq in enumerate(self.docs):
            terms, counts = np.unique(np.asarray(seq, dtype=np.int64), return_counts=True)
            for t, c in zip(terms.tolist(), counts.tolist()):
                lists[t].append(d)
                tfs[t].append(c)
        term_ptr = np.zeros(self.n_terms + 1, dtype=np.int64)
        np.cumsum([len(x) for x in lists], out=term_ptr[1:])
        post_doc = np.asarray([d for x in lists for d in x], dtype=np.int32)
        post_tf = np.asarray([c for x in tfs for c in x], dtype=np.int32)
        doc_len = np.asarray([len(s) for s in self.docs], dtype=np.int32)
        return term_ptr, post_doc, post_tf, np.linspace(0.5, 3.0, self.n_terms), doc_len, float(max(doc_len.mean(), 1e-3))

    def stream(self):
        """(doc_ptr i64 [n + 1], tokens i32): the operands of amdr_bm25_set_tokens."""
        doc_ptr = np.zeros(self.n_docs + 1, dtype=np.int64)
        np.cumsum([len(s) for s in self.docs], out=doc_ptr[1:])
        return doc_ptr, np.asarray([t for s in self.docs for t in s], dtype=np.int32)

    def df(self) -> np.ndarray:
        out = np.zeros(self.n_terms, dtype=np.int64)
        for seq in self.docs:
            for t in set(seq):
                out[t] += 1
        return out

    def holders(self, t: int) -> set:
        kept = self.__dict__.setdefault("_holders", {})
        if t not in kept:
            kept[t] = {d for d, seq in enumerate(self.docs) if t in seq}
        return kept[t]


# ---- the reference ---------------------------------------------------------------------------------------------------------
def holds(seq: Sequence[int], phrase: Sequence[int]) -> bool:
    """The plain window scan of ONE document."""
    L = len(phrase)
    return any(list(seq[p:p + L]) == list(phrase) for p in range(len(seq) - L + 1))


def starts(seq: Sequence[int], phrase: Sequence[int]) -> List[int]:
    L = len(phrase)
    return [p for p in range(len(seq) - L + 1) if list(seq[p:p + L]) == list(phrase)]


def phrase_list(corpus: SeqCorpus, phrase: Sequence[int]) -> np.ndarray:
    """The ascending documents that hold the phrase; empty with an id outside the vocabulary anywhere in it."""
    if any(t < 0 or t >= corpus.n_terms for t in phrase):
        return np.zeros(0, dtype=np.int32)
    return np.asarray([d for d, seq in enumerate(corpus.docs) if holds(seq, phrase)], dtype=np.int32)


def conjunction(corpus: SeqCorpus, phrase: Sequence[int]) -> np.ndarray:
    """The documents that hold every token of the phrase, anywhere."""
    if any(t < 0 or t >= corpus.n_terms for t in phrase):
        return np.zeros(0, dtype=np.int32)
    return np.asarray(sorted(set.intersection(*[corpus.holders(t) for t in phrase])), dtype=np.int32)


def expected_lists(corpus: SeqCorpus, phrases: Sequence[Sequence[int]]):
    """(list_ptr i64 [n_phr + 1], docs i32) of a batch of phrases."""
    lists = [phrase_list(corpus, p) for p in phrases]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    return ptr, (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int32)).astype(np.int32)


def driver_len(corpus: SeqCorpus, phrase: Sequence[int]) -> int:
    """The phrase's candidate count by the rule: the smallest document frequency among its tokens; 0 with an unknown one.
    It is also the host's upper bound of the phrase's list."""
    if any(t < 0 or t >= corpus.n_terms for t in phrase):
        return 0
    df = corpus.df()
    return int(min(df[t] for t in phrase))


def operands(phrases: Sequence[Sequence[int]]):
    """(phr_ptr i64 [n_phr + 1], phr_terms i32) of the ABI."""
    ptr = np.zeros(len(phrases) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in phrases], out=ptr[1:])
    return ptr, np.asarray([t for p in phrases for t in p], dtype=np.int32)


def expected_constraint(corpus: SeqCorpus, con, bases, phrases) -> np.ndarray:
    """Set algebra over the documents' tokens; a term id >= n_terms names a phrase of `phrases`."""
    groups, base = con

    def have(t):
        if 0 <= t < corpus.n_terms:
            return corpus.holders(t)
        p = t - corpus.n_terms
        return {int(d) for d in phrase_list(corpus, phrases[p])} if 0 <= p < len(phrases) else set()
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


def expected_table(corpus: SeqCorpus, fam: TC.Family, phrases):
    lists = [expected_constraint(corpus, con, fam.bases, phrases) for con in fam.cons]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    return ptr, (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64))


def upper_bounds(corpus: SeqCorpus, phrases) -> np.ndarray:
    """df extended by the phrases' upper bounds: what the host packer hands to driver_length."""
    return np.concatenate([corpus.df(), np.asarray([driver_len(corpus, p) for p in phrases], dtype=np.int64)])


# ---- "edge": hand-made documents, one per shape the issue names ------------------------------------------------------
A, B, C_, D, X = 0, 1, 2, 3, 4
W16 = list(range(5, 21))             # the sixteen tokens of the longest phrase, in order
P_, Q_, F = 21, 22, 23               # the lane-stride phrase (P_, Q_) and the filler of its documents
U, V, G = 24, 25, 26                 # the long document's phrase (U, V) and its filler
EDGE_TERMS = 27
AB, ABC, ABAC, AA, PQ, UV = [A, B], [A, B, C_], [A, B, A, C_], [A, A], [P_, Q_], [U, V]
STRIDE_LENGTHS = (63, 64, 65, 127, 128, 129)
STRIDE_STARTS = (62, 63, 64, 127)
LONG_LEN = 4550


def _stride_doc(n: int, start: int) -> List[int]:
    """n tokens with (P_, Q_) at `start` only: a lone Q_ in front and a lone P_ behind keep both tokens present elsewhere
    where there is room, never adjacent in order."""
    seq = [F] * n
    seq[start], seq[start + 1] = P_, Q_
    if start >= 2:
        seq[0] = Q_
    if start + 3 < n:
        seq[n - 1] = P_
    return seq


def edge_corpus():
    """-> (corpus, {name: document id}).  Every named document is described by its certificate in `edge_certificates`."""
    docs, at = [], {}

    def add(name, seq):
        at[name] = len(docs)
        docs.append(list(seq))
    add("first: the whole document is the phrase", AB)                       # document 0; position 0 and the last L tokens
    add("empty", [])
    add("shorter than the phrase", [A])
    add("boundary left", [B, X, A])                                          # A B only ACROSS this document and the next
    add("boundary right", [B, X, A])
    add("wrong order", [B, A])
    add("not adjacent", [A, X, B])
    add("overlap a b a c", [A, B, A, B, A, C_])
    add("a a a", [A, A, A])
    add("all tokens of a b a c, no match", [C_, A, B, A, B, A])
    add("match at the last L tokens", [X, X, X, A, B])
    add("16 at the end", [X] + W16)
    add("16 exactly", W16)
    add("16 present, not adjacent", W16[:15] + [X, W16[15]])
    add("15 of 16", W16[:15])
    add("a b c", ABC)
    add("a b x c", [A, B, X, C_])
    add("x a b c x", [X, A, B, C_, X])
    for n in STRIDE_LENGTHS:
        for s in STRIDE_STARTS:
            if s + 2 <= n:
                add(f"stride len {n} start {s}", _stride_doc(n, s))
        add(f"stride len {n} last", _stride_doc(n, n - 2))
        add(f"stride len {n} none", [Q_] + [F] * (n - 2) + [P_])
    add("long", [V, U] + [G] * (LONG_LEN - 4) + [U, V])
    add("long none", [V, U] + [G] * 40 + [V, G, U])
    add("last: the whole document is the phrase", AB)                        # document n - 1
    return SeqCorpus("edge", EDGE_TERMS, docs), at


EDGE_PHRASES = [AB, ABC, ABAC, AA, W16, PQ, UV, [B, A], [A, B, C_, D]]     # D is in no document: an empty driver


def edge_certificates(corpus: SeqCorpus, at: Dict[str, int]) -> None:
    """What each document of the edge corpus is there for, asserted."""
    d = corpus.docs
    n = corpus.n_docs
    assert at["first: the whole document is the phrase"] == 0 and at["last: the whole document is the phrase"] == n - 1
    assert starts(d[0], AB) == [0] and len(d[0]) == 2 and starts(d[n - 1], AB) == [0]
    assert d[at["empty"]] == [] and len(d[at["shorter than the phrase"]]) < 2
    le, ri = at["boundary left"], at["boundary right"]
    assert ri == le + 1 and d[le][-1] == A and d[ri][0] == B and not holds(d[le], AB) and not holds(d[ri], AB)
    assert holds(d[le] + d[ri], AB)  # the phrase exists only across the boundary
    for name in ("wrong order", "not adjacent", "boundary left", "boundary right"):
        assert {A, B} <= set(d[at[name]]) and not holds(d[at[name]], AB), name
    assert starts(d[at["overlap a b a c"]], ABAC) == [2] and starts(d[at["overlap a b a c"]], [A, B, A]) == [0, 2]
    assert starts(d[at["a a a"]], AA) == [0, 1]
    none = d[at["all tokens of a b a c, no match"]]
    assert set(ABAC) <= set(none) and not holds(none, ABAC)
    assert starts(d[at["match at the last L tokens"]], AB) == [3] and len(d[at["match at the last L tokens"]]) == 5
    assert len(W16) == MAX_LEN and starts(d[at["16 at the end"]], W16) == [1] and starts(d[at["16 exactly"]], W16) == [0]
    assert set(W16) <= set(d[at["16 present, not adjacent"]]) and not holds(d[at["16 present, not adjacent"]], W16)
    assert len(d[at["15 of 16"]]) == 15
    assert holds(d[at["a b c"]], ABC) and not holds(d[at["a b x c"]], ABC) and starts(d[at["x a b c x"]], ABC) == [1]
    seen = set()
    for n_ in STRIDE_LENGTHS:
        for s in list(STRIDE_STARTS) + [n_ - 2]:
            name = f"stride len {n_} start {s}" if s in STRIDE_STARTS and s + 2 <= n_ else f"stride len {n_} last"
            if s + 2 <= n_:
                assert len(d[at[name]]) == n_ and starts(d[at[name]], PQ) == [s if "start" in name else n_ - 2], name
                seen.add((n_, starts(d[at[name]], PQ)[0]))
        miss = d[at[f"stride len {n_} none"]]
        assert len(miss) == n_ and {P_, Q_} <= set(miss) and not holds(miss, PQ)
    # the lane stride's edge: a match in lane 62 / 63 of the first round, lane 0 of the second, lane 63 of the second
    assert {(64, 62), (65, 63), (127, 64), (129, 127), (128, 64), (129, 64)} <= seen
    assert len(d[at["long"]]) == LONG_LEN and starts(d[at["long"]], UV) == [LONG_LEN - 2]
    assert {U, V} <= set(d[at["long none"]]) and not holds(d[at["long none"]], UV)
    # conjunction and phrase differ for every phrase with a match
    for p in (AB, ABC, ABAC, W16, PQ, UV):
        assert 0 < phrase_list(corpus, p).size < conjunction(corpus, p).size, p
    assert phrase_list(corpus, [B, A]).size > 0 and driver_len(corpus, [A, B, C_, D]) == 0


# ---- "tiles": phrase drivers of exactly 0 / 1 / tile - 1 / tile / tile + 1 / 2 tile + 1 candidates ---------------------
DRIVER_LENGTHS = (0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
TILES_N = 700
T_COMMON, T_FILL = 0, 1                 # in every document | a filler
T_RARE = {m: 2 + i for i, m in enumerate(DRIVER_LENGTHS)}  # the term that is in exactly m documents
TILES_TERMS = 2 + len(DRIVER_LENGTHS)


def tiles_corpus() -> SeqCorpus:
    """Every document holds T_COMMON.  The rare term of m sits in exactly m documents — documents 0 and n - 1 among them
    for the longest — followed by T_COMMON in two of three of them (the phrase) and preceded by it in the third (both
    tokens, no phrase)."""
    rng = np.random.default_rng(2718)
    docs = [[T_FILL, T_COMMON, T_FILL] for _ in range(TILES_N)]
    for m, t in T_RARE.items():
        if m == 0:
            continue
        pool = np.arange(1, TILES_N - 1)
        if m == max(DRIVER_LENGTHS):
            where = np.concatenate([[0, TILES_N - 1], rng.choice(pool, size=m - 2, replace=False)])
        else:
            where = rng.choice(pool, size=m, replace=False)
        for j, d in enumerate(sorted(int(x) for x in where)):
            docs[d] += [t, T_COMMON, T_FILL] if (j % 3 != 1 or d in (0, TILES_N - 1)) else [T_COMMON, T_FILL, t, T_FILL]
    return SeqCorpus("tiles", TILES_TERMS, docs)


def tiles_phrases() -> List[List[int]]:
    return [[T_RARE[m], T_COMMON] for m in DRIVER_LENGTHS]


def tiles_certificates(corpus: SeqCorpus) -> None:
    df = corpus.df()
    for m, p in zip(DRIVER_LENGTHS, tiles_phrases()):
        assert driver_len(corpus, p) == m == df[p[0]] and df[T_COMMON] == corpus.n_docs
        got = phrase_list(corpus, p)
        assert (got.size == m == 0) or (m == 1 and got.size == 1) or 0 < got.size < m  # kept and dropped candidates
    longest = phrase_list(corpus, tiles_phrases()[-1])
    assert longest[0] == 0 and longest[-1] == corpus.n_docs - 1  # documents 0 and n - 1


# ---- "rand": 700 random documents over 12 terms; 65 phrases; constraints that use phrases ------------------------------
RAND_N, RAND_TERMS = 700, 12


def rand_corpus() -> SeqCorpus:
    rng = np.random.default_rng(99)
    p = 1.0 / np.arange(1, RAND_TERMS + 1)
    p /= p.sum()
    docs = [rng.choice(RAND_TERMS, size=int(n), p=p).tolist() for n in rng.integers(0, 81, size=RAND_N)]
    return SeqCorpus("rand", RAND_TERMS, docs)


def rand_phrases(corpus: SeqCorpus, count: int = 65) -> List[List[int]]:
    """Windows of the documents (they match somewhere) and random sequences (most of the longer ones match nowhere), of 2
    to 5 tokens, each phrase once."""
    rng = np.random.default_rng(7)
    out, seen = [], set()
    while len(out) < count:
        L = int(rng.integers(2, 6))
        if len(out) % 3 == 2:
            ph = rng.integers(0, RAND_TERMS, size=L).tolist()
        else:
            seq = corpus.docs[int(rng.integers(0, corpus.n_docs))]
            if len(seq) < L:
                continue
            s = int(rng.integers(0, len(seq) - L + 1))
            ph = seq[s:s + L]
        if tuple(ph) not in seen:
            seen.add(tuple(ph))
            out.append([int(t) for t in ph])
    return out


def rand_certificates(corpus: SeqCorpus, phrases) -> None:
    sizes = [phrase_list(corpus, p).size for p in phrases]
    conj = [conjunction(corpus, p).size for p in phrases]
    assert len(phrases) == 65 and min(sizes) == 0 and max(sizes) > TILE  # empty lists and lists of more than one tile
    assert sum(1 for s, c in zip(sizes, conj) if s < c) > 40              # conjunction and phrase differ
    assert min(len(s) for s in corpus.docs) == 0 and max(driver_len(corpus, p) for p in phrases) > 2 * TILE


def scope_family(corpus: SeqCorpus, phrases):
    """Constraints over the "rand" corpus whose term ids n_terms + p name `phrases` (three phrases, chosen by
    `scope_phrases`): a phrase as MUST and driver; as MUST beside a rarer plain term (not the driver); two phrases as
    MUST; as ANY next to a plain group; as NOT; inside a tuple group; an id past the virtual lists (in no document);
    each of the first three again inside a base scope."""
    V = corpus.n_terms
    rare = int(np.argmin(corpus.df()))
    common = int(np.argmax(corpus.df()))
    base_short = np.arange(0, corpus.n_docs, 9, dtype=np.int64)
    base_long = np.arange(2, corpus.n_docs, dtype=np.int64)
    c = TC.c
    cons = [c([(MUST, [V + 0])]), c([(MUST, [V + 1]), (MUST, [rare])]), c([(MUST, [V + 0]), (MUST, [V + 1])]),
            c([(MUST, [common]), (ANY, [V + 2]), (ANY, [rare])]), c([(MUST, [common]), (NOT, [V + 0])]),
            c([(MUST, [common, V + 1])]), c([(ANY, [V + 2])]), c([(NOT, [V + 1, V + 0])]),
            c([(MUST, [V + 3])]), c([(MUST, [common]), (NOT, [V + 3])]),
            c([(MUST, [V + 0])], 0), c([(MUST, [V + 1]), (MUST, [rare])], 1), c([(MUST, [V + 0]), (MUST, [V + 1])], 1)]
    return TC.Family("phrases in constraints", "rand", cons, [base_short, base_long])


def scope_phrases(corpus: SeqCorpus):
    """Three phrases of the corpus's two most frequent terms with long, different, overlapping lists."""
    order = np.argsort(-corpus.df())
    a, b, c = (int(x) for x in order[:3])
    return [[a, b], [b, a], [a, a, c]]


def scope_certificates(corpus: SeqCorpus, fam: TC.Family, phrases) -> None:
    from_lists = [phrase_list(corpus, p) for p in phrases]
    assert all(x.size > TILE for x in from_lists[:2]) and from_lists[2].size > 0
    ub = upper_bounds(corpus, phrases)
    V = corpus.n_terms
    rare = int(np.argmin(corpus.df()))
    assert ub[rare] < from_lists[1].size  # the plain term drives constraint 1, the phrase does not
    assert ub[V + 0] > from_lists[0].size  # the host's bound of a phrase list is not its length
    sizes = [expected_constraint(corpus, con, fam.bases, phrases).size for con in fam.cons]
    common = int(np.argmax(corpus.df()))
    assert sizes[8] == 0 and sizes[9] == len(corpus.holders(common))  # an id past the virtual lists is in no document
    assert all(s > 0 for i, s in enumerate(sizes) if i != 8)
    # a phrase constraint is not its conjunction
    assert sizes[0] < conjunction(corpus, phrases[0]).size

"""Cases of the unit-span resolver (amdr_unit_spans: csrc/unit_span.hip, csrc/unit_span_rule.hpp; `Within` of
retrieval/terms.py): a seeded corpus given as one token SEQUENCE and one BREAK byte per token and document, unit items
whose slots are plain tokens and token classes, and a brute-force evaluator written from the docstrings — it shares nothing
with `Within.within`, `pack()` or the rule header: no ballots, no rounds, no carry, no driver; the unordered form is decided
by a bipartite matching over the positions of each unit.  numpy only: the CPU test (tests/test_unit_span.py) checks the
certificates below and the GPU test (tests/test_unit_span_gpu.py) compares the device lists and the host twin's with
`item_list`.

An ITEM is (kind, slots): kind bit 0 ordered, bit 1 paragraph; a slot is a plain term id (int; outside [0, n_terms): an
unknown token) or a CLASS, the ascending tuple of its member ids.  A break byte is 0, 1 (the token begins a sentence) or 3
(it begins a paragraph, and so a sentence); a document's first token begins both whatever its byte says.
"""
from typing import Dict, List, Sequence, Tuple, Union

import numpy as np

from phrase_cases import SeqCorpus

ORDERED, PARAGRAPH = 1, 2
TILE, LANES = 256, 64
SEED = 20261

Slot = Union[int, Tuple[int, ...]]
Item = Tuple[int, List[Slot]]

N_PLAIN = 60                       # ids 0 .. 59: plain tokens
K0, K_COUNT = 100, 300             # ids 100 .. 399: the words k000 .. k299
N_TERMS = K0 + K_COUNT
F, F2, A, B, G = 0, 1, 50, 51, 52  # two fillers; the hand-made documents' members
COMMON, R255, R256, R257 = 53, 54, 55, 56
NOWHERE = 59                       # a token no document holds
UNKNOWN = N_TERMS + 5000           # a slot id past the vocabulary and past every class of a call
PAIR = (K0, K0 + 1)                # a union of 2 ids
ALL_K = tuple(range(K0, K0 + K_COUNT))  # a union of 300


def word(t: int) -> str:
    if t < 0 or t >= N_TERMS:
        return f"unknown{t}"
    return f"k{t - K0:03d}" if t >= K0 else f"w{t}"


class UnitCorpus(SeqCorpus):
    """A SeqCorpus with one break byte per token: breaks[d][i] of token i of document d."""

    def __init__(self, name: str, n_terms: int, docs, breaks):
        super().__init__(name, n_terms, docs)
        assert len(breaks) == len(docs) and all(len(b) == len(s) for b, s in zip(breaks, docs))
        self.breaks = [[int(x) for x in b] for b in breaks]

    def flags(self) -> np.ndarray:
        """u8 [n_tokens]: the operand of amdr_bm25_set_breaks."""
        return np.asarray([x for b in self.breaks for x in b], dtype=np.uint8)


# ---- the evaluator ---------------------------------------------------------------------------------------------------------
def fills(slot: Slot, t: int) -> bool:
    return t in slot if isinstance(slot, tuple) else t == slot


def units_of(brk: Sequence[int], bit: int) -> List[Tuple[int, int]]:
    """The [begin, end) units of one document: token 0 begins one, and so does every token whose byte has `bit`."""
    n = len(brk)
    if n == 0:
        return []
    begins = [0] + [i for i in range(1, n) if brk[i] & bit]
    return list(zip(begins, begins[1:] + [n]))


def matching(cands: List[List[int]]) -> bool:
    """Whether the slots can take DISTINCT positions, slot j one of cands[j]: augmenting paths (Kuhn)."""
    owner: Dict[int, int] = {}

    def augment(j: int, seen: set) -> bool:
        for q in cands[j]:
            if q in seen:
                continue
            seen.add(q)
            if q not in owner or augment(owner[q], seen):
                owner[q] = j
                return True
        return False
    return all(augment(j, set()) for j in range(len(cands)))


def unit_holds(seq: Sequence[int], b: int, e: int, kind: int, slots: Sequence[Slot]) -> bool:
    if kind & ORDERED:
        p = b
        for s in slots:
            while p < e and not fills(s, seq[p]):
                p += 1
            if p == e:
                return False
            p += 1
        return True
    return matching([[q for q in range(b, e) if fills(s, seq[q])] for s in slots])


def holds(seq: Sequence[int], brk: Sequence[int], item: Item, n_terms: int = N_TERMS) -> bool:
    kind, slots = item
    if not (0 <= kind <= 3 and 2 <= len(slots) <= 8):
        return False
    if any(not isinstance(s, tuple) and not 0 <= s < n_terms for s in slots):
        return False
    return any(unit_holds(seq, b, e, kind, slots) for b, e in units_of(brk, 2 if kind & PARAGRAPH else 1))


def item_list(corpus: UnitCorpus, item: Item) -> np.ndarray:
    """The ascending documents that hold the item; computed once per corpus object and item, never changed."""
    kept = corpus.__dict__.setdefault("_us_lists", {})
    key = (item[0], tuple(item[1]))
    if key not in kept:
        kept[key] = np.asarray([d for d in range(corpus.n_docs) if holds(corpus.docs[d], corpus.breaks[d], item, corpus.n_terms)],
                               dtype=np.int32)
        kept[key].setflags(write=False)
    return kept[key]


def slot_docs(corpus: UnitCorpus, s: Slot) -> set:
    if isinstance(s, tuple):
        out = set()
        for t in s:
            if 0 <= t < corpus.n_terms:
                out |= corpus.holders(int(t))
        return out
    return corpus.holders(int(s)) if 0 <= s < corpus.n_terms else set()


def conjunction(corpus: UnitCorpus, item: Item) -> set:
    """The candidates of an item: the documents that hold a token for every slot (none with an unknown slot)."""
    if any(not isinstance(s, tuple) and not 0 <= s < corpus.n_terms for s in item[1]):
        return set()
    out = None
    for s in item[1]:
        out = slot_docs(corpus, s) if out is None else out & slot_docs(corpus, s)
    return out or set()


def driver_len(corpus: UnitCorpus, item: Item) -> int:
    """The length of the driving list: the shortest slot list; 0 with an unknown slot or an item the rule does not define."""
    kind, slots = item
    if not (0 <= kind <= 3 and 2 <= len(slots) <= 8) or any(not isinstance(s, tuple) and not 0 <= s < corpus.n_terms for s in slots):
        return 0
    return min(len(slot_docs(corpus, s)) for s in slots)


def bounds(corpus: UnitCorpus, items: Sequence[Item]) -> Tuple[int, int]:
    ub = [driver_len(corpus, it) for it in items]
    return max(ub, default=0), int(sum(ub))


def classes_of(items: Sequence[Item]) -> List[Tuple[int, ...]]:
    out: List[Tuple[int, ...]] = []
    for it in items:
        for s in it[1]:
            if isinstance(s, tuple) and s not in out:
                out.append(s)
    return out


def operands(items: Sequence[Item], n_terms: int, cls_first: int = 0):
    """((item_ptr i64 [n + 1], item_slots i32, item_kind i32 [n]), (cls_ptr i64 [n_cls + 1], cls_terms i32)) of the ABI: equal
    tuples are one class, class c is the slot id n_terms + cls_first + c."""
    classes = classes_of(items)
    ptr = np.zeros(len(items) + 1, dtype=np.int64)
    np.cumsum([len(it[1]) for it in items], out=ptr[1:])
    slots = [n_terms + cls_first + classes.index(s) if isinstance(s, tuple) else int(s) for it in items for s in it[1]]
    c_ptr = np.zeros(len(classes) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in classes], out=c_ptr[1:])
    return ((ptr, np.asarray(slots, dtype=np.int32), np.asarray([it[0] for it in items], dtype=np.int32)),
            (c_ptr, np.asarray([t for c in classes for t in c], dtype=np.int32)))


def _array(lists, before=None):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    docs = (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int32)).astype(np.int32)
    if before is not None:
        ptr = np.concatenate([before[0], before[0][-1] + ptr[1:]])
        docs = np.concatenate([before[1], docs]).astype(np.int32)
    return ptr, docs


def expected_lists(corpus: UnitCorpus, items: Sequence[Item], before=None):
    """(list_ptr i64 [n + 1], docs i32) of a batch of items; `before` = (list_ptr, docs): the array they continue."""
    return _array([item_list(corpus, it) for it in items], before)


def class_lists(corpus: UnitCorpus, items: Sequence[Item], before=None):
    """(list_ptr, docs) of the classes' document lists, in the order of `operands`: what the union step writes."""
    return _array([np.asarray(sorted(slot_docs(corpus, c)), dtype=np.int32) for c in classes_of(items)], before)


# ---- the corpus ------------------------------------------------------------------------------------------------------------
def make_corpus(seed: int = SEED):
    """-> (corpus, {name: document id}).  The named documents are the shapes at which the walk can go wrong; `certificates`
    says what each is there for.  Behind them random documents of 2 .. 200 tokens with sparse and dense breaks, and the
    holders of R255 / R256 / R257: drivers of exactly 255, 256 and 257 candidates."""
    rng = np.random.default_rng(seed)
    docs, breaks, at = [], [], {}

    def add(name, seq, flagged=(), value=1, paragraphs=()):
        brk = [0] * len(seq)
        for p in flagged:
            brk[p] = value
        for p in paragraphs:
            brk[p] = 3
        if name is not None:
            at[name] = len(docs)
        docs.append([int(t) for t in seq])
        breaks.append(brk)

    add("1 token", [A])
    add("63 tokens, members at the ends", [A] + [F] * 61 + [B])
    add("64 tokens, members at the ends", [A] + [F] * 62 + [B])
    add("65 tokens, members at the ends", [A] + [F] * 63 + [B])
    add("128 tokens, members at the ends", [A] + [F] * 126 + [B])
    add("129 tokens, members at the ends", [A] + [F] * 127 + [B])
    add("unit begins at lane 0", [A, B] + [F] * 10, flagged=[2])
    add("unit begins at lane 63", [F] * 63 + [A, B] + [F] * 5, flagged=[63])
    add("unit begins at lane 64", [F] * 64 + [A, B] + [F] * 5, flagged=[64])
    add("break at lane 64 between the members", [F] * 63 + [A, B] + [F] * 5, flagged=[64])
    add("unit over a round boundary, a member on each side", [F] * 60 + [A] + [F] * 10 + [B] + [F] * 9, flagged=[58, 75])
    add("unit over three rounds", [F] * 10 + [A] + [F] * 169 + [B] + [F] * 19, flagged=[5, 190])
    add("unit of one token", [F, A, B, F], flagged=[1, 2])
    add("64 units in one round", [F] * 10 + [A, B] + [F] * 52, flagged=range(64))
    add("g g in one unit", [F, G, F2, G, F], flagged=[1])
    add("g g split over two adjacent units", [F, G, F2, G, F], flagged=[3])
    add("g once", [F, G, F2])
    add("ordered: right order across a break", [A, F, B, F], flagged=[2])
    add("ordered: wrong order inside a unit", [F, B, F2, A, F], flagged=[1])
    add("one paragraph, two sentences", [F, A, F, B, F], flagged=[3], paragraphs=[1])
    add("two paragraphs", [F, A, F, B, F], paragraphs=[3])
    add("ends with a member", [F, F, A])
    add("first byte says nothing, previous document ends with a member", [B, F, F])
    add("pair member and b", [F, K0 + 1, F2, B], flagged=[1])
    add("pair member and b apart", [F, K0, F2, B], flagged=[3])
    add("k299 and b", [B, F, K0 + 299])
    add("k299 and b apart", [B, F, K0 + 299], flagged=[2])
    add("empty", [])
    n_named = len(docs)
    # random documents: plain tokens 2 .. 40 by a skewed draw, now and then a word of the 300; a break every 2 .. 30 tokens,
    # a quarter of them paragraph breaks; every ninth document long (two or three rounds), every seventh without a break
    weights = 1.0 / (1.0 + np.arange(39))
    weights /= weights.sum()
    n_rand = 620
    for i in range(n_rand):
        n = int(rng.integers(100, 201)) if i % 9 == 0 else int(rng.integers(2, 60))
        seq = (2 + rng.choice(39, size=n, p=weights)).tolist()
        for p in range(n):
            if rng.random() < 0.06:
                seq[p] = K0 + int(rng.integers(0, K_COUNT))
        every = 0 if i % 7 == 0 else int(rng.integers(2, 31))
        brk = [0] * n
        for p in range(n):
            if every and rng.integers(0, every) == 0:
                brk[p] = 3 if rng.integers(0, 4) == 0 else 1
        docs.append(seq + [COMMON])
        breaks.append(brk + [0])
    # the drivers: R255, R256 and R257 stand in exactly that many random documents, in the unit of the COMMON token at the
    # document's end; every third holder gets a break between the two
    for tok, count in ((R255, 255), (R256, 256), (R257, 257)):
        for j, d in enumerate(sorted(rng.choice(n_rand, size=count, replace=False).tolist())):
            d += n_named
            docs[d] = docs[d][:-1] + [tok, COMMON]
            breaks[d] = breaks[d][:-1] + [0, 1 if j % 3 == 0 else 0]
    return UnitCorpus("units", N_TERMS, docs, breaks), at


def named_items() -> Dict[str, Item]:
    S, P = 0, PARAGRAPH
    return {
        "a b /s": (S, [A, B]), "a b /p": (P, [A, B]), "a b +s": (S | ORDERED, [A, B]), "a b +p": (P | ORDERED, [A, B]),
        "b a +s": (S | ORDERED, [B, A]), "b a /s": (S, [B, A]),
        "g g /s": (S, [G, G]), "g g +s": (S | ORDERED, [G, G]), "g g /p": (P, [G, G]),
        "pair b /s": (S, [PAIR, B]), "all k b /s": (S, [ALL_K, B]), "all k b +p": (P | ORDERED, [B, ALL_K]),
        "unknown -1": (S, [A, -1]), "unknown past the classes": (P, [UNKNOWN, A]), "nowhere": (S, [A, NOWHERE]),
        "r255 /s": (S, [R255, COMMON]), "r256 /s": (S, [COMMON, R256]), "r257 +s": (S | ORDERED, [R257, COMMON]),
        "r257 /p": (P, [R257, COMMON]),
    }


def batch(corpus: UnitCorpus, count: int, seed: int = SEED) -> List[Item]:
    """`count` items: the named ones first, then random ones of 2 .. 4 slots (now and then 8) over the frequent plain tokens
    and small classes — the slots of an unordered item pairwise disjoint or the same slot again — with an unknown slot now
    and then."""
    items = list(named_items().values())
    rng = np.random.default_rng(seed + 1)
    plain = list(range(2, 14))
    disjoint = plain + [(14, 15), (16, 17, 18), PAIR, (K0 + 2, K0 + 3, K0 + 4)]
    loose = disjoint + [(2, 3), (3, 14), ALL_K]
    while len(items) < count:
        kind = int(rng.integers(0, 4))
        src = loose if kind & ORDERED else disjoint
        M = 8 if len(items) % 13 == 12 else int(rng.integers(2, 5))
        slots = [src[int(rng.integers(0, len(src)))] for _ in range(M)]
        if len(items) % 9 == 8:
            slots[int(rng.integers(0, M))] = -1 if len(items) % 2 else UNKNOWN
        items.append((kind, slots))
    return items[:count]


N_ITEMS = 72


# ---- the wrong models: what a broken walk would compute --------------------------------------------------------------------
def no_breaks(corpus: UnitCorpus, item: Item) -> List[int]:
    """Breaks ignored: the plain conjunction with multiplicities (one unit per document)."""
    return [d for d in range(corpus.n_docs) if holds(corpus.docs[d], [0] * len(corpus.docs[d]), item, corpus.n_terms)]


def no_carry(corpus: UnitCorpus, item: Item) -> List[int]:
    """Every round boundary treated as a break: a walk that forgets the open unit."""
    out = []
    for d in range(corpus.n_docs):
        brk = [3 if i % LANES == 0 else x for i, x in enumerate(corpus.breaks[d])]
        if holds(corpus.docs[d], brk, item, corpus.n_terms):
            out.append(d)
    return out


def sentence_for_paragraph(corpus: UnitCorpus, item: Item) -> List[int]:
    """Sentence flags used for paragraph items."""
    return item_list(corpus, (item[0] & ~PARAGRAPH, item[1])).tolist()


def certificates(corpus: UnitCorpus, at: Dict[str, int]) -> None:
    """What each named document is there for, asserted with the evaluator alone."""
    it = named_items()
    L = {name: set(item_list(corpus, x).tolist()) for name, x in it.items()}
    d = corpus.docs
    assert [len(d[at[f"{n} tokens, members at the ends"]]) for n in (63, 64, 65, 128, 129)] == [63, 64, 65, 128, 129]
    assert len(d[at["1 token"]]) == 1 and at["1 token"] not in L["a b /s"]
    for n in (63, 64, 65, 128, 129):  # one unit, however many rounds
        assert at[f"{n} tokens, members at the ends"] in L["a b /s"] & L["a b +p"]
    for lane in (0, 63, 64):
        assert at[f"unit begins at lane {lane}"] in L["a b /s"] & L["a b +s"]
    cut = at["break at lane 64 between the members"]
    assert corpus.breaks[cut][64] == 1 and cut not in L["a b /s"] and cut in L["a b /p"]
    over = at["unit over a round boundary, a member on each side"]
    assert d[over].index(A) < 64 <= d[over].index(B) and over in L["a b /s"] and over not in L["b a +s"]
    three = at["unit over three rounds"]
    assert d[three].index(A) < 64 and d[three].index(B) >= 128 and three in L["a b +s"]
    assert at["unit of one token"] not in L["a b /s"] and at["unit of one token"] in L["a b /p"]
    many = at["64 units in one round"]
    assert all(corpus.breaks[many]) and many not in L["a b /s"] and many in L["a b /p"]
    assert at["g g in one unit"] in L["g g /s"] & L["g g +s"] and at["g g split over two adjacent units"] not in L["g g /s"]
    assert at["g g split over two adjacent units"] in L["g g /p"] and at["g once"] not in L["g g /p"]
    assert at["ordered: right order across a break"] not in L["a b +s"] and at["ordered: right order across a break"] in L["a b +p"]
    wrong = at["ordered: wrong order inside a unit"]
    assert wrong not in L["a b +s"] and wrong in L["a b /s"] and wrong in L["b a +s"]
    two = at["one paragraph, two sentences"]
    assert two not in L["a b /s"] and two in L["a b /p"] and at["two paragraphs"] not in L["a b /p"]
    first = at["first byte says nothing, previous document ends with a member"]
    assert first - 1 == at["ends with a member"] and d[first - 1][-1] == A and d[first][0] == B and corpus.breaks[first][0] == 0
    assert first not in L["a b /p"] and first - 1 not in L["a b /p"]  # no unit crosses two documents
    assert at["pair member and b"] in L["pair b /s"] and at["pair member and b apart"] not in L["pair b /s"]
    assert at["k299 and b"] in L["all k b /s"] and at["k299 and b apart"] not in L["all k b /s"]
    assert at["k299 and b"] in L["all k b +p"] and len(ALL_K) == 300 and len(PAIR) == 2
    assert not L["unknown -1"] and not L["unknown past the classes"] and not L["nowhere"]
    for tok, n, name in ((R255, 255, "r255 /s"), (R256, 256, "r256 /s"), (R257, 257, "r257 +s")):
        assert len(corpus.holders(tok)) == n == driver_len(corpus, it[name]) and 0 < len(L[name]) < n
    assert L["r257 /p"] > L["r257 +s"]

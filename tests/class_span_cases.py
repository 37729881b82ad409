"""Cases of the class-span resolver (amdr_class_spans: csrc/class_span.hip, csrc/class_span_rule.hpp): small corpora given
as one token SEQUENCE per document (phrase_cases.SeqCorpus), items whose slots are plain tokens and token classes, and the
reference — `PhraseOf.within` / `NearOf.within` over the documents' WORDS, which shares nothing with the rule header: no
masks, no driver, no first-unfilled-slot tally (the unordered form is a bipartite matching), no lanes.  numpy only: the
CPU test (tests/test_class_span.py) checks the certificates below — each builder certifies its own case — and the GPU test
(tests/test_class_span_gpu.py) compares the device lists and the host twin's with `item_list`.

An ITEM is (kind, slots, distance): kind 0 a phrase (distance unused), 1 unordered, 2 ordered (near_cases); a slot is a
plain term id (int; outside [0, n_terms): an unknown token) or a CLASS, the ascending tuple of its member ids.  `operands`
turns a batch into the arrays of the ABI: equal tuples are one class, class c is the slot id n_terms + cls_first + c.
"""
from typing import Dict, List, Sequence, Tuple, Union

import numpy as np

import phrase_cases as PC
import term_scope_cases as TC
from phrase_cases import SeqCorpus

MUST, ANY, NOT = TC.MUST, TC.ANY, TC.NOT
PHRASE, UNORDERED, ORDERED = 0, 1, 2
TILE, LANES = PC.TILE, PC.LANES

Slot = Union[int, Tuple[int, ...]]
Item = Tuple[int, List[Slot], int]

K0, K_COUNT = 100, 4096           # the ids 100 .. 4195 are the words k0000 .. k4095: Prefix("k") names 4 096 tokens
N_TERMS = K0 + K_COUNT + 4        # ... and four plain tokens behind them
ALL_K = tuple(range(K0, K0 + K_COUNT))


def word(t: int) -> str:
    """The word of term id t; an id outside the vocabulary is a word no document holds."""
    if t < 0 or t >= N_TERMS:
        return f"unknown{t}"
    return f"k{t - K0:04d}" if K0 <= t < K0 + K_COUNT else f"w{t}"


def member(slot: Slot):
    from legal_rag_amd.retrieval.terms import OneOf, Prefix
    if isinstance(slot, tuple):
        if slot == ALL_K:
            return Prefix("k")  # (4 096 alternatives as one bisection-free startswith)
        return OneOf(*[word(t) for t in slot]) if slot else OneOf("no-such-word")
    return word(slot)


def as_object(item: Item):
    """The item as the public class over words: what the reference is asked."""
    from legal_rag_amd.retrieval.terms import NearOf, PhraseOf
    kind, slots, n = item
    ms = [member(s) for s in slots]
    return PhraseOf(*ms) if kind == PHRASE else NearOf(*ms, distance=n, ordered=kind == ORDERED)


def cls(*ids) -> Tuple[int, ...]:
    return tuple(sorted(int(i) for i in ids))


def near_of(slots: Sequence[Slot], n: int, ordered: bool = False) -> Item:
    return (ORDERED if ordered else UNORDERED, list(slots), int(n))


def phrase_of(slots: Sequence[Slot]) -> Item:
    return (PHRASE, list(slots), 0)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def words_of(corpus: SeqCorpus) -> List[List[str]]:
    kept = corpus.__dict__.get("_words")
    if kept is None:
        kept = corpus.__dict__["_words"] = [[word(t) for t in seq] for seq in corpus.docs]
    return kept


def slot_known(corpus: SeqCorpus, s: Slot) -> bool:
    return isinstance(s, tuple) or 0 <= s < corpus.n_terms


def item_list(corpus: SeqCorpus, item: Item) -> np.ndarray:
    """The ascending documents that hold the item by `within`; computed once per corpus object and item, never changed."""
    kept = corpus.__dict__.setdefault("_cs_lists", {})
    key = (item[0], tuple(item[1]), item[2])
    if key not in kept:
        obj = as_object(item)
        kept[key] = np.asarray([d for d, ws in enumerate(words_of(corpus)) if obj.within(ws)], dtype=np.int32)
        kept[key].setflags(write=False)
    return kept[key]


def expected_lists(corpus: SeqCorpus, items: Sequence[Item], before=None):
    """(list_ptr i64 [n + 1], docs i32) of a batch of items; `before` = (list_ptr, docs): the array they continue."""
    lists = [item_list(corpus, it) for it in items]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    docs = (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int32)).astype(np.int32)
    if before is not None:
        ptr = np.concatenate([before[0], before[0][-1] + ptr[1:]])
        docs = np.concatenate([before[1], docs]).astype(np.int32)
    return ptr, docs


def slot_docs(corpus: SeqCorpus, s: Slot) -> set:
    """The documents that hold a token filling the slot: a posting list, or what the union step makes of a class."""
    if isinstance(s, tuple):
        out = set()
        for t in s:
            if 0 <= t < corpus.n_terms:
                out |= corpus.holders(int(t))
        return out
    return corpus.holders(int(s)) if 0 <= s < corpus.n_terms else set()


def driver(corpus: SeqCorpus, item: Item) -> Tuple[int, int]:
    """(the driving slot's position, its list's length) by the rule: the shortest slot list, ties -> the first slot;
    (-1, 0) with an unknown slot.  The length is also the smallest bound a caller can give."""
    if not all(slot_known(corpus, s) for s in item[1]):
        return -1, 0
    lens = [len(slot_docs(corpus, s)) for s in item[1]]
    return int(np.argmin(lens)), int(min(lens))


def bounds(corpus: SeqCorpus, items: Sequence[Item]):
    """(cand_max, rows_cap) that always suffice: the largest and the sum of the drivers."""
    ub = [driver(corpus, it)[1] for it in items]
    return max(ub, default=0), int(sum(ub))


def classes_of(items: Sequence[Item]) -> List[Tuple[int, ...]]:
    out: List[Tuple[int, ...]] = []
    for it in items:
        for s in it[1]:
            if isinstance(s, tuple) and s not in out:
                out.append(s)
    return out


def operands(items: Sequence[Item], n_terms: int, cls_first: int = 0):
    """((item_ptr i64 [n + 1], item_slots i32, item_kind i32 [n], item_dist i32 [n]), (cls_ptr i64 [n_cls + 1], cls_terms
    i32)) of the ABI."""
    classes = classes_of(items)
    ptr = np.zeros(len(items) + 1, dtype=np.int64)
    np.cumsum([len(it[1]) for it in items], out=ptr[1:])
    slots = [n_terms + cls_first + classes.index(s) if isinstance(s, tuple) else int(s) for it in items for s in it[1]]
    c_ptr = np.zeros(len(classes) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in classes], out=c_ptr[1:])
    return ((ptr, np.asarray(slots, dtype=np.int32), np.asarray([it[0] for it in items], dtype=np.int32),
             np.asarray([it[2] for it in items], dtype=np.int32)),
            (c_ptr, np.asarray([t for c in classes for t in c], dtype=np.int32)))


def class_lists(corpus: SeqCorpus, items: Sequence[Item], before=None):
    """(list_ptr, docs) of the classes' document lists, in the order of `operands`: what the union step writes."""
    lists = [np.asarray(sorted(slot_docs(corpus, c)), dtype=np.int32) for c in classes_of(items)]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    docs = (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int32)).astype(np.int32)
    if before is not None:
        ptr = np.concatenate([before[0], before[0][-1] + ptr[1:]])
        docs = np.concatenate([before[1], docs]).astype(np.int32)
    return ptr, docs


# ---- "edge": hand-made documents for one distance n and one class --------------------------------------------------------
B, F, G, NOWHERE = 5, 1, 2, 3     # the plain partner of the class, two fillers, a token no document holds
UNKNOWN = N_TERMS + 5000          # a slot id past the vocabulary AND past every class of a call (n_terms + c names class c)
SIZES = (1, 2, 64, 65, K_COUNT)   # member ids of the class
DIST = 5


def a_class(m: int) -> Tuple[int, ...]:
    return tuple(range(K0, K0 + m))


def edge_corpus(m: int, n: int = DIST):
    """-> (corpus, {name: document id}) for the class a_class(m) (first member a0 = K0, last member a9 = K0 + m - 1) and the
    plain token B, distance n.  The named documents are described by `edge_certificates`."""
    a0, a9 = K0, K0 + m - 1
    docs, at = [], {}

    def add(name, seq):
        at[name] = len(docs)
        docs.append([int(t) for t in seq])
    add("one token", [a0])                                                   # 1 token
    add("L - 1", [B])
    add("L: the whole document", [a9, B])                                    # a match at the first AND the last token
    add("63, match at the end", [F] * 61 + [a9, B])
    add("64, anchor in lane 63, partner in the next document", [F] * 63 + [a0])
    add("65, begins with the partner", [B] + [G] * 64)                       # ... which must not count for the one before
    add("64 + n, the window runs into the next round", [F] * 63 + [a0] + [F] * (n - 1) + [B])
    add("64 + n + 1, one too far", [F] * 63 + [a9] + [F] * n + [B])
    add("319, partner first", [B] + [G] * (n - 1) + [a9] + [G] * (319 - n - 1))
    add("320, match at the last two tokens", [F] * 318 + [a0, B])
    add("two members, no partner", [a0, F, a9])
    add("equal slots need two positions: one", [a0, G, G])
    add("equal slots need two positions: two", [a9, G, a0])
    add("empty", [])
    add("partner alone", [G, B, G])
    return SeqCorpus(f"edge-{m}", N_TERMS, docs), at


def edge_items(m: int, n: int = DIST) -> Dict[str, Item]:
    A = a_class(m)
    return {
        "near": near_of([A, B], n), "near reversed": near_of([B, A], n), "ordered": near_of([A, B], n, True),
        "ordered reversed": near_of([B, A], n, True), "phrase": phrase_of([A, B]), "ordered 1": near_of([A, B], 1, True),
        "equal slots": near_of([A, A], 2), "equal slots ordered": near_of([A, A], 2, True), "phrase of two": phrase_of([A, A]),
        "empty class": near_of([A, cls()], n), "nowhere": near_of([A, NOWHERE], n), "unknown -1": near_of([A, -1], n),
        "unknown past the classes": phrase_of([UNKNOWN, A]), "class and filler": near_of([A, F], 255),
        "three": near_of([A, B, F], n + 1), "every k": near_of([ALL_K, B], n),
    }


def edge_certificates(m: int, n: int = DIST) -> None:
    """What each document and item of an edge corpus is there for, asserted against the reference."""
    corpus, at = edge_corpus(m, n)
    items = edge_items(m, n)
    L = {name: set(item_list(corpus, it).tolist()) for name, it in items.items()}
    d = corpus.docs
    assert [len(d[at[k]]) for k in ("one token", "L - 1", "L: the whole document")] == [1, 1, 2]
    assert sorted(len(s) for s in d if len(s) >= 63)[:3] == [63, 64, 65] and {64 + n, 64 + n + 1, 319, 320} <= {len(s) for s in d}
    lane63, nxt = at["64, anchor in lane 63, partner in the next document"], at["65, begins with the partner"]
    assert nxt == lane63 + 1 and d[lane63][63] == K0 and d[nxt][0] == B
    for name in ("near", "ordered", "phrase"):  # the straddling match does not count, on either side
        assert lane63 not in L[name] and nxt not in L[name], name
    run = at["64 + n, the window runs into the next round"]
    assert d[run][63] == K0 and d[run][-1] == B and len(d[run]) == 64 + n > 64
    assert run in L["near"] and run in L["ordered"] and run in L["near reversed"] and run not in L["ordered reversed"]
    assert (run in L["phrase"]) == (n == 1)
    far = at["64 + n + 1, one too far"]
    assert far not in L["near"] and far not in L["ordered"] and far in L["three"] - L["near"]
    first = at["319, partner first"]
    assert first in L["near"] and first not in L["ordered"] and first in L["ordered reversed"]
    for k in ("L: the whole document", "63, match at the end", "320, match at the last two tokens"):
        assert at[k] in L["phrase"] and at[k] in L["ordered 1"], k  # matches that end at a document's last token
    assert L["phrase"] == L["ordered 1"]
    one, two = at["equal slots need two positions: one"], at["equal slots need two positions: two"]
    assert one not in L["equal slots"] and two in L["equal slots"] and two in L["equal slots ordered"]
    assert at["two members, no partner"] in L["equal slots"] and not L["phrase of two"]
    for name in ("empty class", "nowhere", "unknown -1", "unknown past the classes"):
        assert not L[name], name
    assert L["every k"] >= L["near"] and (m < K_COUNT or L["every k"] == L["near"])
    # drivers: the class list drives "near" when it is the shorter one, the plain posting otherwise; the three kinds occur
    dr = {name: driver(corpus, it) for name, it in items.items()}
    assert dr["nowhere"] == (1, 0) and dr["empty class"] == (1, 0) and dr["unknown -1"] == (-1, 0)
    assert dr["class and filler"][0] == (0 if len(slot_docs(corpus, a_class(m))) <= len(corpus.holders(F)) else 1)
    assert dr["equal slots"][0] == 0  # ties go to the first slot
    for name, lst in L.items():
        assert len(lst) <= dr[name][1] or dr[name][0] < 0 and not lst, name


# ---- "drivers": a driver of exactly `count` candidates, a class list or a plain posting ------------------------------------
DRIVER_COUNTS = (255, 256, 257, 3 * 256 + 1)
RARE, COMMON = 6, 7


def driver_corpus(count: int):
    """2 * count + 40 documents: RARE stands in exactly `count` of them, the class {K0, K0 + 1, K0 + 2} in exactly count + 1
    and COMMON in all; every third holder of RARE, and the last, has the two close together."""
    rng = np.random.default_rng(7000 + count)
    n_docs = 2 * count + 40
    docs = [[COMMON] + [int(x) for x in rng.integers(8, 40, size=int(rng.integers(2, 9)))] for _ in range(n_docs)]
    rare = sorted(rng.choice(n_docs, size=count, replace=False).tolist())
    close = [j % 3 == 0 or j == count - 1 for j in range(count)]  # (the last candidate too: a tile of one keeps it)
    for j, dd in enumerate(rare):
        docs[dd] += [RARE, F, K0 + j % 3] if close[j] else [RARE]
    cls_docs = {dd for j, dd in enumerate(rare) if close[j]}
    for dd in rng.permutation(n_docs).tolist():
        if len(cls_docs) == count + 1:
            break
        if dd not in cls_docs:
            cls_docs.add(dd)
            docs[dd] = [K0 + dd % 3] + [G] * 9 + docs[dd]
    return SeqCorpus(f"drivers-{count}", N_TERMS, docs)


def driver_items() -> Dict[str, Item]:
    A3 = cls(K0, K0 + 1, K0 + 2)
    return {"plain posting drives": near_of([A3, RARE], 2), "class list drives": near_of([A3, COMMON], 255),
            "class first of a tie": near_of([A3, A3], 255), "ordered": near_of([RARE, A3], 2, True),
            "phrase": phrase_of([RARE, F, A3])}


def driver_certificates(count: int) -> None:
    corpus = driver_corpus(count)
    items = driver_items()
    assert len(corpus.holders(RARE)) == count and len(slot_docs(corpus, cls(K0, K0 + 1, K0 + 2))) == count + 1
    assert driver(corpus, items["plain posting drives"]) == (1, count) and driver(corpus, items["class list drives"]) == (0, count + 1)
    assert driver(corpus, items["class first of a tie"]) == (0, count + 1)
    hit = item_list(corpus, items["plain posting drives"])
    assert 0 < hit.size < count and hit.size == item_list(corpus, items["phrase"]).size == item_list(corpus, items["ordered"]).size
    tiles = -(-count // TILE)
    assert len({int(np.searchsorted(sorted(corpus.holders(RARE)), dd)) // TILE for dd in hit.tolist()}) == tiles  # every tile keeps some


def batch(corpus: SeqCorpus, named: Dict[str, Item], count: int) -> List[Item]:
    """`count` items: the named ones first, then random ones over small classes and plain tokens (the slots of an unordered
    item pairwise equal or disjoint), an unknown slot now and then."""
    items = list(named.values())
    rng = np.random.default_rng(500 + count)
    pool = [cls(K0, K0 + 1), cls(K0 + 2), cls(8, 9, 10), cls(11, 12), B, F, G, RARE, COMMON, 20, 21]   # pairwise disjoint
    loose = pool + [cls(K0 + 1, K0 + 2), cls(B, 8), cls(F, G, 20)]                                      # overlapping ones
    while len(items) < count:
        kind = int(rng.integers(0, 3))
        src = pool if kind == UNORDERED else loose
        M = int(rng.integers(2, 5))
        slots = [src[int(rng.integers(0, len(src)))] for _ in range(M)]
        if len(items) % 9 == 8:
            slots[int(rng.integers(0, M))] = -1 if len(items) % 2 else UNKNOWN
        items.append((kind, slots, 0 if kind == PHRASE else int(rng.integers(1, 9))))
    return items[:count]

"""Cases of the marks kernel (csrc/marks.hip, csrc/marks_rule.hpp) and its reference: a plain-Python restatement of the rule
— which positions of a hit document a query marks, and its best window — that shares nothing with the rule header (no
rounds, no lanes, no staged run, no binary search).  A window's score is Python float adds in ascending slot order from
0.0: the same doubles in the same order as the kernel, so the bits are equal.  numpy only; the GPU test
(tests/test_marks_gpu.py) compares every output array of both forms with `expected`.

A query is a MarkQuery: table {term id: slot}, weights [32], the loose mask and the sequences (lists of slots)."""
from dataclasses import dataclass, field
from typing import Dict, List, Sequence

import numpy as np

import phrase_cases as PC

SLOTS = 32        # kMkSlots
MAX_MARKS = 1024  # kMkMaxMarks
MAX_LEN = 16      # kPhMaxLen


@dataclass
class MarkQuery:
    table: Dict[int, int]
    loose: int = 0
    seqs: List[List[int]] = field(default_factory=list)
    w: Sequence[float] = tuple(0.1 * (s + 1) for s in range(SLOTS))


def marks_of(tokens: Sequence[int], q: MarkQuery):
    """[(position, slot)] of every marked position of one document, ascending."""
    n = len(tokens)
    masks = []
    for t in tokens:
        s = q.table.get(int(t), -1)
        masks.append(1 << s if 0 <= s < SLOTS else 0)
    cover = [0] * n
    for sq in q.seqs:
        L = len(sq)
        if L < 2 or L > MAX_LEN or any(s < 0 or s >= SLOTS for s in sq):
            continue  # never occurs
        for p in range(n - L + 1):
            if all((masks[p + j] >> sq[j]) & 1 for j in range(L)):
                for j in range(L):
                    cover[p + j] |= 1 << sq[j]
    out = []
    for p in range(n):
        m = (masks[p] & q.loose) | cover[p]
        if m:
            out.append((p, (m & -m).bit_length() - 1))
    return out


def pair(tokens: Sequence[int], q: MarkQuery, window: int, cap: int):
    """(win [4], score, slots [2], marks [cap, 2], status) of one (query, hit) pair."""
    n = len(tokens)
    every = marks_of(tokens, q)
    kept = every[:MAX_MARKS]
    best = None  # (score, anchor index, end, bits, count)
    for i, (a, _) in enumerate(kept):
        e = min(a + window, n)
        bits, t = 0, i
        while t < len(kept) and kept[t][0] < e:
            bits |= 1 << kept[t][1]
            t += 1
        score = 0.0
        for s in range(SLOTS):
            if (bits >> s) & 1:
                score = score + float(q.w[s])
        if best is None or score > best[0]:  # (ties stay with the earlier anchor)
            best = (score, i, e, bits, t - i)
    marks = np.full((cap, 2), -1, np.int32)
    all_bits = 0
    for _, s in kept:
        all_bits |= 1 << s
    if best is None:
        return [0, min(window, n), 0, len(every)], 0.0, [0, all_bits], marks, 0
    score, i, e, bits, count = best
    for j in range(min(cap, count)):
        marks[j] = kept[i + j]
    return [kept[i][0], e, count, len(every)], score, [bits, all_bits], marks, int(len(every) > MAX_MARKS)


def expected(docs_tokens: Sequence[Sequence[int]], hits, queries: Sequence[MarkQuery], window: int, cap: int):
    """The five output arrays for hits i64 [nq, k] (an id outside [0, n_docs): no hit)."""
    hits = np.asarray(hits, np.int64)
    nq, k = hits.shape
    win, score = np.zeros((nq, k, 4), np.int32), np.zeros((nq, k), np.float64)
    slots, marks = np.zeros((nq, k, 2), np.uint32), np.full((nq, k, cap, 2), -1, np.int32)
    status = np.zeros((nq, k), np.int32)
    seen = {}
    for qi in range(nq):
        for j in range(k):
            d = int(hits[qi, j])
            if d < 0 or d >= len(docs_tokens):
                continue
            key = (qi, d)
            if key not in seen:
                seen[key] = pair(docs_tokens[d], queries[qi], window, cap)
            win[qi, j], score[qi, j], slots[qi, j], marks[qi, j], status[qi, j] = seen[key]
    return win, score, slots, marks, status


def operands(queries: Sequence[MarkQuery]):
    """(mk_ptr, mk_terms, mk_slot, slot_w [nq, 32], slot_loose, sq_ptr, sq_off, sq_slots) of amdr_bm25_marks."""
    mk_ptr, mk_terms, mk_slot, sq_ptr, sq_off, sq_slots = [0], [], [], [0], [0], []
    for q in queries:
        for t in sorted(q.table):
            mk_terms.append(t), mk_slot.append(q.table[t])
        mk_ptr.append(len(mk_terms))
        for sq in q.seqs:
            sq_slots.extend(sq), sq_off.append(len(sq_slots))
        sq_ptr.append(len(sq_off) - 1)
    w = np.asarray([list(q.w) for q in queries], np.float64).reshape(len(queries), SLOTS)
    loose = np.asarray([q.loose for q in queries], np.uint32)
    return (np.asarray(mk_ptr, np.int64), np.asarray(mk_terms, np.int32), np.asarray(mk_slot, np.int32), w, loose,
            np.asarray(sq_ptr, np.int64), np.asarray(sq_off, np.int64), np.asarray(sq_slots, np.int32))


# ---- the edge corpus ---------------------------------------------------------------------------------------------------------
A, B, C_, D, E, F, G, X = 0, 1, 2, 3, 4, 5, 6, 7  # X fills; nothing names it
CLS0, CLS_N = 100, 3000                          # the 3 000 members of the Prefix class: terms 100 .. 3 099
N_TERMS = CLS0 + CLS_N
LENGTHS = (0, 1, 63, 64, 65, 79, 128, 1500)
SEVEN = [A, B, C_, D, E, F, G]


def edge_corpus():
    """(corpus, at): one document per length of LENGTHS and the placements the rule's edges need; at: name -> document id."""
    docs, at = [], {}

    def add(name, seq):
        at[name] = len(docs)
        docs.append(list(seq))

    def fill(n, put):
        seq = [X] * n
        for p, t in put.items():
            seq[p] = t
        return seq

    add("len0", [])
    add("len1", [A])
    add("len63_ends_ab", fill(63, {5: B, 61: A, 62: B}))              # a phrase ending exactly at the document's end
    add("len64_tail_next", fill(64, {63: A}))                        # "a b" with its tail in the NEXT document:
    add("len65_starts_b", fill(65, {0: B, 30: A, 31: A, 32: B}))     # must not occur
    add("len79_straddle", fill(79, {**{60 + j: t for j, t in enumerate(SEVEN)}, 70: A, 78: C_}))  # positions 60 .. 66
    add("len128_overlap", fill(128, {10: A, 11: A, 12: A, 20: A, 50: B, 63: A, 64: A, 100: C_, 101: B, 102: A, 127: A}))
    add("len1500_all_a", [A] * 1500)                                  # 1 500 marks: past the cap
    add("len1500_mixed", [(A, X, B, X, X, C_, X)[i % 7] if i % 11 else CLS0 + (i * 37) % CLS_N for i in range(1500)])
    add("class_then_a", fill(70, {3: CLS0, 4: A, 40: CLS0 + CLS_N - 1, 41: A, 50: CLS0 + 1500, 51: B, 69: CLS0 + 7}))
    rng = np.random.default_rng(11)
    for i in range(6):
        add(f"rand{i}", rng.integers(0, 9, size=int(rng.integers(2, 200))).tolist())
    return PC.SeqCorpus("marks-edge", N_TERMS, docs), at


W123 = tuple([0.1, 0.2, 0.3] + [0.5 + s for s in range(SLOTS - 3)])  # 0.1 + 0.2 + 0.3 != 0.3 + 0.2 + 0.1


def edge_queries() -> Dict[str, MarkQuery]:
    cls = {CLS0 + i: 0 for i in range(CLS_N)}
    return {
        "ab_a_loose": MarkQuery({A: 0, B: 1}, loose=0b01, seqs=[[0, 1]], w=W123),       # a: loose and a member; b: member only
        "ab_phrase_only": MarkQuery({A: 0, B: 1}, loose=0, seqs=[[0, 1]], w=W123),
        "abc_loose": MarkQuery({A: 2, B: 1, C_: 0}, loose=0b111, seqs=[], w=W123),       # an empty sequence list
        "empty": MarkQuery({}, loose=0xFFFFFFFF, seqs=[], w=W123),                       # an empty mark table
        "seven": MarkQuery({t: j for j, t in enumerate(SEVEN)}, loose=0, seqs=[list(range(7))], w=W123),
        "aa": MarkQuery({A: 5}, loose=0, seqs=[[5, 5]], w=W123),                         # overlapping occurrences
        "prefix_class": MarkQuery({**cls, A: 1, B: 31}, loose=0b1, seqs=[[0, 1], [0, 31]], w=W123),
        "two_seqs": MarkQuery({A: 3, B: 4, C_: 9}, loose=1 << 9, seqs=[[3, 3, 4], [9, 4, 3], [3, 4]], w=W123),
        "aaaa16": MarkQuery({A: 0}, loose=0, seqs=[[0] * MAX_LEN], w=W123),
        "negative_w": MarkQuery({A: 0, B: 1, C_: 2}, loose=0b111, seqs=[], w=tuple([-1.0, 2.5, 0.0] + [1.0] * (SLOTS - 3))),
    }


def rand_queries(corpus, count: int, seed: int = 5) -> List[MarkQuery]:
    """Random tables over the small terms 0 .. 8 and the class, random loose masks, up to 3 sequences of 2 .. 4 slots."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n_slots = int(rng.integers(1, 6))
        table = {int(t): int(rng.integers(0, n_slots)) for t in rng.choice(9, size=int(rng.integers(0, 9)), replace=False)}
        if i % 5 == 0:
            table.update({CLS0 + int(t): n_slots - 1 for t in rng.choice(CLS_N, size=200, replace=False)})
        seqs = [[int(s) for s in rng.integers(0, n_slots, size=int(rng.integers(2, 5)))] for _ in range(int(rng.integers(0, 4)))]
        w = tuple(float(x) for x in rng.random(SLOTS))
        out.append(MarkQuery(table, loose=int(rng.integers(0, 1 << n_slots)), seqs=seqs, w=w))
    return out

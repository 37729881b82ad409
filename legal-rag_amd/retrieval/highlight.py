"""Term highlighting and the best-passage snippet of each hit: the output side of the query language of retrieval/terms.py.

No reference counterpart: legalrag returns whole chunks.  Here the GPU marks, in the resident token stream of the BM25
index, the tokens of each HIT chunk that the question and its `Terms` name, and picks the window of `Highlight.window`
tokens that holds the most of them (amdr_bm25_marks, csrc/marks.hip; the rule is csrc/marks_rule.hpp).  This module is the
host side: the result types, the SLOT TABLE of a (question, terms) pair — what the kernel takes — and the mapping of token
positions back to character spans of the chunk text.

Slots.  A slot is one query word, at most 32 per question:
  * the items of terms.all_of / any_of come first (none_of is never marked), then the question's tokens (question=True),
    cut with the DOCUMENT-side tokeniser so that "Security" marks "security"; a question token without a letter or a digit
    (the blanks and the punctuation a segmenter cuts as tokens of their own) is no query word;
  * a plain token, a Prefix (every vocabulary token with the stem), a Wildcard, a Fuzzy and a OneOf are LOOSE slots: they
    mark their tokens wherever they stand; so are the members of a Near / NearOf / Within;
  * a Phrase / PhraseOf is a SEQUENCE over its members' slots, which are loose only if something else makes them so: its
    members are marked only where the whole phrase stands;
  * a term id that belongs to two slots goes to the lower one; a slot's weight is the model's idf of its token, for a class
    the greatest among its members; with more than 32 slots the `terms` slots are kept first, then the heaviest question
    tokens (ties to the earliest), numbered in question order; a token the vocabulary does not hold gets no slot and its
    label goes to `missing`.
"""
from __future__ import annotations

from dataclasses import asdict, dataclass, field
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from .terms import Fuzzy, Near, NearOf, Phrase, PhraseOf, Prefix, Terms, Wildcard, Within, prefix_tokens

MAX_SLOTS = 32      # kMkSlots
MAX_WINDOW = 4096   # kMkMaxWindow
MAX_MARKS = 64      # kMkMaxCap


@dataclass(frozen=True)
class Highlight:
    """What to highlight: the best window of `window` tokens (1 .. 4096), at most `marks` marks of it returned (0 .. 64),
    and whether the question's own tokens are marked beside those of `terms`.  Frozen, validated."""
    window: int = 48
    marks: int = 32
    question: bool = True

    def __post_init__(self) -> None:
        for name, lo, hi in (("window", 1, MAX_WINDOW), ("marks", 0, MAX_MARKS)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"Highlight.{name}: an int in {lo} .. {hi}, got {v!r}")
            object.__setattr__(self, name, int(v))
        if not isinstance(self.question, (bool, np.bool_)):
            raise ValueError(f"Highlight.question: a bool, got {self.question!r}")
        object.__setattr__(self, "question", bool(self.question))


@dataclass(frozen=True)
class Mark:
    """One marked token: its position in the chunk's token run, its slot and the slot's label (the query word), and its
    character span in the chunk text (None when the text could not be mapped)."""
    token: int
    slot: int
    label: str
    char_start: Optional[int]
    char_end: Optional[int]


@dataclass
class HitHighlight:
    """The highlight of one hit.  window_tokens: the [start, end) token window shown — the best window's marks centred
    within `Highlight.window` tokens; window_chars / snippet: its character span and text (None when the text could not be
    mapped); score: the best window's score (the summed weights of its distinct slots); marks: the window's marks, at most
    `Highlight.marks`; found / missing: the labels of the slots with / without a mark in the chunk (missing also holds the
    words the vocabulary does not know); n_marks_in_chunk: every mark of the chunk; truncated: the chunk has more marks
    than the kernel keeps (1 024) — the window is then the best among the kept ones."""
    window_tokens: Tuple[int, int]
    window_chars: Optional[Tuple[int, int]]
    snippet: Optional[str]
    score: float
    marks: List[Mark] = field(default_factory=list)
    found: List[str] = field(default_factory=list)
    missing: List[str] = field(default_factory=list)
    n_marks_in_chunk: int = 0
    truncated: bool = False

    def as_dict(self) -> Dict[str, Any]:
        d = asdict(self)
        d["window_tokens"] = list(self.window_tokens)
        d["window_chars"] = None if self.window_chars is None else list(self.window_chars)
        return d


# ---- the slot table -------------------------------------------------------------------------------------------------------------
@dataclass
class SlotTable:
    """The operands of one question: labels / weights per slot, the loose mask, term id -> slot (ascending ids), the
    sequences as slot lists, and the labels that got no slot."""
    labels: List[str]
    weights: List[float]
    loose: int
    terms: Dict[int, int]
    seqs: List[List[int]]
    missing: List[str]


def _label(m) -> str:
    if isinstance(m, str):
        return m
    if isinstance(m, Prefix):
        return m.stem + "!"
    if isinstance(m, Wildcard):
        return m.pattern
    if isinstance(m, Fuzzy):
        return f"{m.token}~{m.edits}"
    return "(" + " ".join(_label(x) for x in m.members) + ")"


def _member_ids(m, vocab: Mapping[str, int], sorted_vocab: Sequence[str],
                expansions: Optional[Mapping[Any, Any]] = None) -> List[int]:
    """The term ids a slot member names: a token, a Prefix's vocabulary tokens, the tokens `expansions` holds for a Wildcard
    or a Fuzzy (terms.pack: ValueError without an entry), a OneOf's members; [] when unknown."""
    if isinstance(m, str):
        return [vocab[m]] if m in vocab else []
    if isinstance(m, Prefix):
        return [vocab[t] for t in prefix_tokens(m.stem, sorted_vocab)]
    if isinstance(m, (Wildcard, Fuzzy)):
        if expansions is None or m not in expansions:
            raise ValueError(f"{m!r}: no expansion of this pattern was given (expansions=)")
        return sorted({vocab[w] for w in (e if isinstance(e, str) else e[0] for e in expansions[m]) if w in vocab})
    out: List[int] = []
    for x in m.members:
        out.extend(_member_ids(x, vocab, sorted_vocab, expansions))
    return sorted(set(out))


def slot_table(question_tokens: Sequence[str], terms: Optional[Terms], vocab: Mapping[str, int], idf,
               sorted_vocab: Sequence[str], expansions: Optional[Mapping[Any, Any]] = None) -> SlotTable:
    """The slot table of a (question, terms) pair.  question_tokens: the question cut with the document-side tokeniser
    ([] for question=False); vocab: token -> term id; idf: token -> weight, or a sequence indexed by term id;
    sorted_vocab: the vocabulary ascending (for Prefix); expansions: the tokens each Wildcard / Fuzzy names (None: the
    terms hold no pattern)."""
    words: Optional[List[str]] = None

    def weight_of(ids: Sequence[int]) -> float:
        nonlocal words
        if isinstance(idf, Mapping):
            if words is None:
                words = [None] * len(vocab)  # type: ignore[list-item]
                for w, t in vocab.items():
                    words[t] = w
            return max(float(idf[words[t]]) for t in ids)
        return max(float(idf[t]) for t in ids)

    slots: List[dict] = []       # in order of appearance: key, label, ids, weight, loose, origin
    by_key: Dict[Any, dict] = {}
    seqs: List[List[dict]] = []
    missing: List[str] = []

    def miss(label: str) -> None:
        if label not in missing:
            missing.append(label)

    def slot_for(m, loose: bool, origin: str) -> Optional[dict]:
        key = m if isinstance(m, str) else repr(m)
        s = by_key.get(key)
        if s is None:
            ids = _member_ids(m, vocab, sorted_vocab, expansions)
            if not ids:
                miss(_label(m))
                return None
            s = by_key[key] = {"label": _label(m), "ids": ids, "weight": weight_of(ids), "loose": False, "origin": origin}
            slots.append(s)
        s["loose"] = s["loose"] or loose
        return s

    if terms is not None:
        for group in list(terms.all_of or ()) + list(terms.any_of or ()):
            for item in group:
                if isinstance(item, (Phrase, PhraseOf)):
                    members = item.tokens if isinstance(item, Phrase) else item.members
                    unknown = [m for m in members if not _member_ids(m, vocab, sorted_vocab, expansions)]
                    if unknown:  # the phrase stands nowhere: none of its members is marked for it
                        for m in unknown:
                            miss(_label(m))
                        continue
                    seqs.append([slot_for(m, False, "terms") for m in members])
                elif isinstance(item, (Near, NearOf, Within)):
                    for m in (item.tokens if isinstance(item, Near) else item.members):
                        slot_for(m, True, "terms")
                else:
                    slot_for(item, True, "terms")
    for tok in question_tokens:
        if any(ch.isalnum() for ch in tok):  # (a tokeniser that cuts blanks and punctuation as tokens: no query words)
            slot_for(tok, True, "question")
    # the cut: the terms' slots first, then the heaviest question tokens (ties to the earliest), in question order
    kept = [s for s in slots if s["origin"] == "terms"][:MAX_SLOTS]
    rest = [(i, s) for i, s in enumerate(slots) if s["origin"] == "question"]
    room = MAX_SLOTS - len(kept)
    chosen = sorted(sorted(rest, key=lambda p: (-p[1]["weight"], p[0]))[:room], key=lambda p: p[0])
    kept += [s for _, s in chosen]
    number = {id(s): j for j, s in enumerate(kept)}
    for s in slots:
        if id(s) not in number:
            miss(s["label"])
    term_slot: Dict[int, int] = {}
    for j, s in enumerate(kept):
        for t in s["ids"]:
            term_slot.setdefault(int(t), j)  # (a term of two slots goes to the lower one)
    out_seqs = [[number[id(s)] for s in sq] for sq in seqs if len(sq) >= 2 and all(id(s) in number for s in sq)]
    loose = 0
    for j, s in enumerate(kept):
        if s["loose"]:
            loose |= 1 << j
    return SlotTable([s["label"] for s in kept], [s["weight"] for s in kept], loose, dict(sorted(term_slot.items())), out_seqs,
                     missing)


def pack_tables(tables: Sequence[SlotTable]):
    """The operand arrays of BM25Index.marks for a batch of slot tables."""
    mk_ptr, mk_terms, mk_slot, sq_ptr, sq_off, sq_slots = [0], [], [], [0], [0], []
    w = np.zeros((len(tables), MAX_SLOTS), np.float64)
    loose = np.zeros(len(tables), np.uint32)
    for q, t in enumerate(tables):
        mk_terms.extend(t.terms.keys()), mk_slot.extend(t.terms.values())
        mk_ptr.append(len(mk_terms))
        for sq in t.seqs:
            sq_slots.extend(sq), sq_off.append(len(sq_slots))
        sq_ptr.append(len(sq_off) - 1)
        w[q, :len(t.weights)] = t.weights
        loose[q] = t.loose
    return (np.asarray(mk_ptr, np.int64), np.asarray(mk_terms, np.int32), np.asarray(mk_slot, np.int32), w, loose,
            np.asarray(sq_ptr, np.int64), np.asarray(sq_off, np.int64), np.asarray(sq_slots, np.int32))


# ---- token positions -> character spans ------------------------------------------------------------------------------------------
def char_spans(text: str, tokens: Sequence[str], lowered: bool) -> Optional[List[Tuple[int, int]]]:
    """The [start, end) character span of each of `tokens` — the text cut again with the document-side tokeniser — in
    `text`, by in-order substring search in the string the tokeniser saw (`lowered`: the lower-cased text).  None when
    lower-casing changed the text's length (the offsets would not be the text's) or a token is not found in order."""
    seen = text.lower() if lowered else text
    if len(seen) != len(text):
        return None
    spans, cursor = [], 0
    for tok in tokens:
        at = seen.find(tok, cursor) if tok else -1
        if at < 0:
            return None
        spans.append((at, at + len(tok)))
        cursor = at + len(tok)
    return spans


def centred(first: int, last: int, window: int, n_tokens: int) -> Tuple[int, int]:
    """The [start, end) window of `window` tokens that centres the marks first .. last (inclusive) inside a run of
    n_tokens, clamped to the run."""
    pad = max(window - (last - first + 1), 0) // 2
    start = max(first - pad, 0)
    end = min(start + window, n_tokens)
    start = max(min(start, end - window), 0)
    return start, max(end, min(last + 1, n_tokens))


def build(table: SlotTable, spec: Highlight, win, score: float, slots, marks, status: int, text: Optional[str],
          tokens: Optional[Sequence[str]], lowered: bool, n_tokens: int) -> HitHighlight:
    """The HitHighlight of one pair from the kernel's outputs.  text / tokens: the chunk text and its re-cut tokens (None:
    no character mapping); n_tokens: the length of the chunk's resident token run."""
    w_start, w_end, w_count, n_all = (int(x) for x in win)
    kept = [(int(p), int(s)) for p, s in marks if p >= 0]
    if w_count > 0:
        last = kept[-1][0] if len(kept) == w_count else w_end - 1
        start, end = centred(w_start, last, spec.window, n_tokens)
    else:
        start, end = w_start, w_end
    spans = None
    if text is not None and tokens is not None and len(tokens) == n_tokens:
        spans = char_spans(text, tokens, lowered)
    chars = snippet = None
    if spans is not None:
        chars = (spans[start][0], spans[end - 1][1]) if end > start else (0, 0)
        snippet = text[chars[0]:chars[1]]
    out = [Mark(p, s, table.labels[s], spans[p][0] if spans else None, spans[p][1] if spans else None) for p, s in kept]
    in_chunk = int(slots[1])
    found = [lab for j, lab in enumerate(table.labels) if (in_chunk >> j) & 1]
    missing = [lab for j, lab in enumerate(table.labels) if not (in_chunk >> j) & 1] + list(table.missing)
    return HitHighlight((start, end), chars, snippet, float(score), out, found, missing, n_all, bool(status))

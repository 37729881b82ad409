"""Vocabulary patterns resolved on the GPU: which tokens a `Wildcard` or a `Fuzzy` (retrieval/terms.py) names.

No reference counterpart: legalrag looks a query token up exactly, so a misspelt word silently matches nothing.  A Prefix is
a contiguous range of the sorted vocabulary and is expanded by bisection on the host (terms.prefix_tokens); a wildcard or an
edit-distance pattern has no such range and is a scan of every token — here ONE native call for the distinct patterns of a
batch (amdr_vocab_match, csrc/vocab_match.hip) over a resident copy of the vocabulary.  This module is the host side: the
matcher over the native handle, `expand()`, whose result `terms.pack(expansions=)` and `highlight.slot_table(expansions=)`
take, and the "did you mean" ordering of `suggest`.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Mapping, Optional, Sequence, Tuple

from .. import _native
from .terms import FUZZY_MAX_EDITS, PREFIX_MAX_TERMS, Fuzzy, Wildcard


@dataclass(frozen=True)
class Suggestion:
    """One "did you mean" candidate: a vocabulary token, its distance from the word and its document frequency."""
    token: str
    distance: int
    doc_freq: int


def order_suggestions(matches: Sequence[Tuple[str, int]], doc_freq: Mapping[str, int], top: int) -> Tuple[Suggestion, ...]:
    """The first `top` of (token, distance) pairs by (distance ascending, document frequency descending, token ascending
    by code point): the word itself comes first, at distance 0, when the vocabulary holds it."""
    out = sorted((Suggestion(t, int(d), int(doc_freq.get(t, 0))) for t, d in matches),
                 key=lambda s: (s.distance, -s.doc_freq, s.token))
    return tuple(out[:max(int(top), 0)])


class VocabMatcher:
    """The tokens of one vocabulary, resident on `device`, and the patterns matched against them.  `vocab` is the token
    list in TERM-ID order (token i is term id i) or a token -> term id mapping such as BM25Okapi.vocab(), which is laid out
    by id here (ValueError unless its ids are exactly 0 .. n - 1)."""

    def __init__(self, vocab, *, device: int = 0):
        if isinstance(vocab, Mapping):
            by_id: list = [None] * len(vocab)
            for w, t in vocab.items():
                if not 0 <= int(t) < len(by_id) or by_id[int(t)] is not None:
                    raise ValueError(f"VocabMatcher: the term ids of the vocabulary are not 0 .. {len(by_id) - 1}, each once")
                by_id[int(t)] = w
            vocab = by_id
        self.tokens = list(vocab)
        self.device = int(device)
        self.native = _native.VocabIndex(self.tokens, device=self.device)

    def __len__(self) -> int:
        return len(self.tokens)

    def expand(self, members: Sequence[Any], item_cap: int = PREFIX_MAX_TERMS) -> Dict[Any, Tuple[Tuple[str, int], ...]]:
        """{member: ((token, distance), ...)} of the DISTINCT Wildcards and Fuzzys among `members`, each row ascending by
        term id, resolved in ONE native call (the distance of a Wildcard's token is 0).  A member that names more than
        `item_cap` tokens (PREFIX_MAX_TERMS) is a ValueError naming it, as an over-wide Prefix is."""
        distinct = list(dict.fromkeys(members))
        for m in distinct:
            if not isinstance(m, (Wildcard, Fuzzy)):
                raise TypeError(f"expand: a member is a Wildcard or a Fuzzy, got {type(m).__name__}")
        if not distinct:
            return {}
        ids, dist, n_match = self.native.match(*_native.VocabIndex.pack_patterns([m.native_pattern() for m in distinct]),
                                               int(item_cap))
        out: Dict[Any, Tuple[Tuple[str, int], ...]] = {}
        for p, m in enumerate(distinct):
            n = int(n_match[p])
            if n > item_cap:
                raise ValueError(f"{m!r} names {n} vocabulary tokens, more than {item_cap}: give a narrower pattern")
            out[m] = tuple((self.tokens[int(t)], int(d)) for t, d in zip(ids[p, :n].tolist(), dist[p, :n].tolist()))
        return out

    def suggest_batch(self, words: Sequence[str], doc_freq: Mapping[str, int], edits: int = 2,
                      top: int = 5) -> Tuple[Tuple[Suggestion, ...], ...]:
        """Per word the vocabulary tokens within `edits` (1 or 2) of it, ordered by order_suggestions; one native call for
        the batch.  A word no longer than `edits` takes the most edits a Fuzzy of it allows, len(word) - 1 — within its own
        length in edits a word names every short token, which is no suggestion — so a word of one character (or none) is
        suggested only itself, when the vocabulary holds it: a short word never fails the batch."""
        if isinstance(edits, bool) or not isinstance(edits, int) or not 1 <= edits <= FUZZY_MAX_EDITS:
            raise ValueError(f"suggest: edits of 1 or {FUZZY_MAX_EDITS}, got {edits!r}")
        pats = [Fuzzy(w, edits=min(edits, len(w) - 1)) if len(w) > 1 else None for w in words]
        got = self.expand([p for p in pats if p is not None])
        return tuple(order_suggestions(got[p] if p is not None else [(w, 0)] if w in doc_freq else [], doc_freq, top)
                     for w, p in zip(words, pats))


def collect_patterns(terms: Sequence[Optional[Any]]) -> list:
    """The distinct Wildcards and Fuzzys of a batch of Terms (None entries skipped), in order of appearance."""
    seen: Dict[Any, None] = {}
    for t in terms:
        if t is not None:
            for m in t.patterns():
                seen.setdefault(m)
    return list(seen)

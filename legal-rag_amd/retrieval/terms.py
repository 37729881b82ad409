"""Required and excluded terms: "articles that contain *seller* and *goods* but not *buyer*".

No reference counterpart: legalrag's BM25 channel only prefers a query's terms and HybridRetriever.search has no filter
argument; a caller who wants a term of art to stand in every hit over-fetches and filters on the host — fewer than top_k
hits, and a fusion normalised over rows the user excluded (the failure retrieval/scope.py describes).  Here a `Terms`
names what a chunk's text must contain, `pack()` turns the (Scope, Terms) pairs of a batch into the operand arrays of
amdr_term_scope (csrc/term_scope.hip), and the GPU resolves them on the resident BM25 postings into the scope table the
scoped channels take: every channel then ranks only the qualifying chunks, with the scores and the order of the unscoped
channels (idf and avgdl stay those of the whole index).

A `Phrase` is an exact token SEQUENCE: Phrase("security", "interest") names the chunks that hold the two words next to
each other in that order.  It stands wherever a token stands.  The GPU resolves each phrase of a batch from the resident
token stream into an ascending document list of its own (amdr_phrase_lists, csrc/phrase_scope.hip), and the term step
reads that list as one more term.

A `Near` is PROXIMITY: Near("buyer", "seller", distance=5) names the chunks that hold the two words within five tokens of
each other, in either order (ordered=True: in the order given) — looser than a phrase, stricter than a conjunction.  It
stands wherever a token or a Phrase stands, and the GPU resolves the phrases and the Nears of a batch in one step into one
array of document lists (amdr_span_lists).

A `Prefix` is the ROOT EXPANDER (sell! in a Boolean legal search): Prefix("sell") names every vocabulary token that starts
with "sell" — the index has no stemmer — and a `OneOf` is ALTERNATIVES as one term: OneOf("buyer", "purchaser").  Either
stands wherever a token stands, also inside a tuple group: (OneOf("buyer", "purchaser"), OneOf("goods", "merchandise")) is
(buyer OR purchaser) AND (goods OR merchandise).  `pack()` expands both into the term ids they name and the GPU merges the
posting lists of each into one ascending, de-duplicated document list (amdr_union_lists, csrc/union_lists.hip) behind the
lists of the phrases and the Nears.

A `PhraseOf` and a `NearOf` are a phrase and a Near of token CLASSES: a member is a token, a Prefix or a OneOf, so
PhraseOf(Prefix("secur"), "interest") is "secur! interest" and NearOf(Prefix("sell"), Prefix("good"), distance=5) is
sell! /5 good!.  They are classes of their own — Phrase, Near and OneOf keep their constructors and their errors — and stand
wherever a Phrase or a Near stands.  `pack()` resolves each member as it resolves a Prefix or a OneOf; an item of plain
ids IS the plain Phrase / Near, every other one is a class span that the GPU resolves from the token stream and the
unions' lists (amdr_class_spans, csrc/class_span.hip) behind the unions.

A `Wildcard` and a `Fuzzy` are vocabulary PATTERNS: Wildcard("s?ll*") names every vocabulary token the pattern fits ('?' one
character, '*' any run) and Fuzzy("warrenty", edits=1) every token within one edit of the word, transpositions included.
Either stands wherever a Prefix stands.  Which tokens a pattern names is found by a scan of the resident vocabulary on the
GPU (amdr_vocab_match, csrc/vocab_match.hip; retrieval/vocab_match.py VocabMatcher.expand) and handed to `pack()` as
`expansions`; from there on a pattern resolves exactly as a Prefix does.

A `Within` is the SAME-SENTENCE / SAME-PARAGRAPH connector (buyer /s seller, buyer +p seller): Within("buyer", "seller",
unit="sentence") names the chunks in which one sentence holds both words — "one provision speaks of both", which no
distance expresses.  Its members are those of a NearOf and it stands wherever a Near stands.  Where a sentence or a
paragraph begins is the rule of retrieval/units.py, resident beside the token stream as one break byte per token
(amdr_bm25_set_breaks); the GPU resolves the Withins of a batch from the stream and the flags (amdr_unit_spans,
csrc/unit_span.hip) behind the class spans.
"""
from __future__ import annotations

from bisect import bisect_left
from dataclasses import dataclass
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np

from .scope import Scope

MUST, ANY, NOT = 0, 1, 2  # the group kinds of the ABI (term_scope_rule.hpp TsKind)

PHRASE_MAX_LEN = 16  # tokens of a phrase (phrase_rule.hpp kPhMaxLen)
NEAR_MAX_TERMS = 8   # tokens of a Near (near_rule.hpp kNearMaxTerms)
NEAR_MAX_DIST = 255  # the largest distance of a Near (near_rule.hpp kNearMaxDist)
PREFIX_MAX_TERMS = 4096  # vocabulary tokens one Prefix or OneOf may name (pack)


class Phrase:
    """An exact token sequence: a chunk holds Phrase(t0, t1, ...) when its text, as the index's tokeniser cuts it, has
    t0 t1 ... at consecutive positions (never across two chunks).  1 to 16 tokens (ValueError otherwise); one token is
    the plain term.  Accepted wherever a token is: as an entry of a Terms field or as a member of a tuple group.  Tokens
    are compared exactly, as a Terms' are (HybridRetriever.phrase cuts a string with the index's own tokeniser).
    Frozen and hashable: equal phrases are equal and hash alike."""
    __slots__ = ("tokens",)

    def __init__(self, *tokens: str) -> None:
        if not 1 <= len(tokens) <= PHRASE_MAX_LEN:
            raise ValueError(f"Phrase: 1 to {PHRASE_MAX_LEN} tokens, got {len(tokens)}")
        for t in tokens:
            if not isinstance(t, str):
                raise TypeError(f"Phrase: a token is a str, got {type(t).__name__}")
        object.__setattr__(self, "tokens", tuple(tokens))

    def __setattr__(self, name, value) -> None:
        raise AttributeError("Phrase is frozen")

    def __delattr__(self, name) -> None:
        raise AttributeError("Phrase is frozen")

    def __eq__(self, other) -> bool:
        return isinstance(other, Phrase) and self.tokens == other.tokens

    def __hash__(self) -> int:
        return hash(("Phrase", self.tokens))

    def __len__(self) -> int:
        return len(self.tokens)

    def __repr__(self) -> str:
        return "Phrase(" + ", ".join(repr(t) for t in self.tokens) + ")"

    def __reduce__(self):
        return (Phrase, self.tokens)

    def within(self, tokens: Sequence[str]) -> bool:
        """Whether the token sequence `tokens` holds this phrase (the plain window scan)."""
        L, want = len(self.tokens), self.tokens
        return any(tuple(tokens[p:p + L]) == want for p in range(len(tokens) - L + 1))


class Near:
    """Proximity: a chunk holds Near(t0, t1, ..., distance=n) when its text, as the index's tokeniser cuts it, has the
    tokens close together (never across two chunks).
      ordered=False  some run of at most n + 1 consecutive tokens contains every distinct token at least as many times as
                     the Near names it: Near("a", "a", "b", distance=5) needs two a and one b inside one window; for two
                     different tokens at positions p and q this is |q - p| <= n.
      ordered=True   there are positions p0 < p1 < ... with the tokens in the order given and the last at most n behind
                     the first.
    2 to 8 tokens and 1 <= distance <= 255 (ValueError otherwise); repeats are allowed and are meaningful.  Accepted
    wherever a token or a Phrase is: as an entry of a Terms field or as a member of a tuple group; its members are tokens,
    not phrases.  Near(a, b, distance=1, ordered=True) names the chunks Phrase(a, b) names.  Tokens are compared exactly,
    as a Terms' are (HybridRetriever.near cuts a string with the index's own tokeniser).  Frozen and hashable: equal Nears
    are equal and hash alike."""
    __slots__ = ("tokens", "distance", "ordered")

    def __init__(self, *tokens: str, distance: int, ordered: bool = False) -> None:
        if not 2 <= len(tokens) <= NEAR_MAX_TERMS:
            raise ValueError(f"Near: 2 to {NEAR_MAX_TERMS} tokens, got {len(tokens)}")
        for t in tokens:
            if not isinstance(t, str):
                raise TypeError(f"Near: a token is a str, got {type(t).__name__}")
        if isinstance(distance, bool) or not isinstance(distance, (int, np.integer)):
            raise TypeError(f"Near: distance is an int, got {type(distance).__name__}")
        if not 1 <= int(distance) <= NEAR_MAX_DIST:
            raise ValueError(f"Near: a distance of 1 to {NEAR_MAX_DIST}, got {int(distance)}")
        object.__setattr__(self, "tokens", tuple(tokens))
        object.__setattr__(self, "distance", int(distance))
        object.__setattr__(self, "ordered", bool(ordered))

    def __setattr__(self, name, value) -> None:
        raise AttributeError("Near is frozen")

    def __delattr__(self, name) -> None:
        raise AttributeError("Near is frozen")

    def _key(self):
        return (self.tokens, self.distance, self.ordered)

    def __eq__(self, other) -> bool:
        return isinstance(other, Near) and self._key() == other._key()

    def __hash__(self) -> int:
        return hash(("Near",) + self._key())

    def __len__(self) -> int:
        return len(self.tokens)

    def __repr__(self) -> str:
        return ("Near(" + ", ".join(repr(t) for t in self.tokens) + f", distance={self.distance}"
                + (", ordered=True" if self.ordered else "") + ")")

    def __reduce__(self):
        return (_make_near, (self.tokens, self.distance, self.ordered))

    def within(self, tokens: Sequence[str]) -> bool:
        """Whether the token sequence `tokens` holds this Near (the plain scan of every window)."""
        n, want = self.distance, self.tokens
        if not set(want) <= set(tokens):  # (a sequence that lacks a token has no such window)
            return False
        for s in range(len(tokens)):
            win = tokens[s:s + n + 1]
            if self.ordered:
                if win[0] != want[0]:  # (the span is measured from the first token's position)
                    continue
                j = 0
                for t in win:
                    if t == want[j]:
                        j += 1
                        if j == len(want):
                            return True
            else:
                have: Dict[str, int] = {}
                for t in win:
                    have[t] = have.get(t, 0) + 1
                if all(have.get(t, 0) >= want.count(t) for t in want):
                    return True
        return False


def _make_near(tokens, distance, ordered) -> Near:
    return Near(*tokens, distance=distance, ordered=ordered)


class Prefix:
    """The root expander: Prefix("sell") names every vocabulary token that starts with "sell" (sell, seller, seller's,
    selling, sells), and a chunk holds it when it holds at least one of them.  The stem is a non-empty str (TypeError /
    ValueError otherwise), compared exactly as every token is (HybridRetriever.prefix cuts a string with the index's own
    tokeniser).  Accepted wherever a token is: as an entry of a Terms field, as a member of a tuple group or of a OneOf —
    not inside a Phrase or a Near.  A stem that no token starts with is a token the vocabulary does not hold.  Frozen and
    hashable: equal prefixes are equal and hash alike."""
    __slots__ = ("stem",)

    def __init__(self, stem: str) -> None:
        if not isinstance(stem, str):
            raise TypeError(f"Prefix: the stem is a str, got {type(stem).__name__}")
        if not stem:
            raise ValueError("Prefix: an empty stem names every token")
        object.__setattr__(self, "stem", stem)

    def __setattr__(self, name, value) -> None:
        raise AttributeError("Prefix is frozen")

    def __delattr__(self, name) -> None:
        raise AttributeError("Prefix is frozen")

    def __eq__(self, other) -> bool:
        return isinstance(other, Prefix) and self.stem == other.stem

    def __hash__(self) -> int:
        return hash(("Prefix", self.stem))

    def __repr__(self) -> str:
        return f"Prefix({self.stem!r})"

    def __reduce__(self):
        return (Prefix, (self.stem,))

    def within(self, tokens) -> bool:
        """Whether one of `tokens` (a set or a sequence) starts with the stem."""
        return any(t.startswith(self.stem) for t in tokens)

WILDCARD_MAX_LEN = 64  # code points of a Wildcard's pattern or a Fuzzy's token (vocab_match_rule.hpp kVmMaxLen)
FUZZY_MAX_EDITS = 2    # kVmMaxEdits
_ANY_ONE, _ANY_RUN = 0x110000, 0x110001  # '?' and '*' among a Wildcard's code points (kVmAnyOne, kVmAnyRun)


def wildcard_fits(pattern: str, token: str) -> bool:
    """Whether `token` fits `pattern` ('?' exactly one character, '*' any run, the empty one included), character by
    character — code points, as Python's str is: greedy, with the last '*' as the one backtrack point.  The empty token
    fits nothing."""
    if not token:
        return False
    p = t = 0
    star_p, star_t = -1, 0
    while t < len(token):
        if p < len(pattern) and pattern[p] == "*":
            star_p, star_t = p, t
            p += 1
        elif p < len(pattern) and (pattern[p] == "?" or pattern[p] == token[t]):
            p, t = p + 1, t + 1
        elif star_p >= 0:
            star_t += 1
            p, t = star_p + 1, star_t
        else:
            return False
    return all(c == "*" for c in pattern[p:])


def osa_distance(a: str, b: str) -> int:
    """The optimal-string-alignment distance of two strings over code points: insertion, deletion, substitution and the
    transposition of two adjacent characters cost 1 each, and no character is edited twice (osa("ca", "abc") is 3)."""
    before2: List[int] = []
    before = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        row = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            v = min(before[j] + 1, row[j - 1] + 1, before[j - 1] + (a[i - 1] != b[j - 1]))
            if i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                v = min(v, before2[j - 2] + 1)
            row[j] = v
        before2, before = before, row
    return before[len(b)]


class Wildcard:
    """The universal characters: Wildcard("s?ll*") names every vocabulary token that fits the pattern, and a chunk holds
    it when it holds at least one of them.  '?' stands for exactly one character, '*' for any run of characters, the empty
    one included, every other character for itself; characters are Unicode code points, never bytes.  The pattern has 1
    to 64 code points, at least one of them a literal, and holds a '?' or a '*' (ValueError otherwise: write the plain
    token).  There is NO escape: a vocabulary token that is literally "?" or holds a '*' cannot be named by a Wildcard (a
    plain str names it).  Westlaw's wom*n is Wildcard("wom?n"); its sell! stays Prefix("sell").  Accepted wherever a
    Prefix is: as an entry of a Terms field, in a tuple group, as a member of a OneOf, a PhraseOf or a NearOf — not inside
    a plain Phrase or Near.  The pattern is compared as it is given (an English index is lower-cased: write it so); no
    retriever method cuts one, because a tokeniser would cut at '?'.  Frozen and hashable."""
    __slots__ = ("pattern",)

    def __init__(self, pattern: str) -> None:
        if not isinstance(pattern, str):
            raise TypeError(f"Wildcard: the pattern is a str, got {type(pattern).__name__}")
        if not 1 <= len(pattern) <= WILDCARD_MAX_LEN:
            raise ValueError(f"Wildcard: 1 to {WILDCARD_MAX_LEN} characters, got {len(pattern)}")
        if all(c in "?*" for c in pattern):
            raise ValueError(f"Wildcard: {pattern!r} holds no literal character and names every token of its length")
        if "?" not in pattern and "*" not in pattern:
            raise ValueError(f"Wildcard: {pattern!r} holds neither '?' nor '*': write the plain token")
        object.__setattr__(self, "pattern", pattern)

    def __setattr__(self, name, value) -> None:
        raise AttributeError("Wildcard is frozen")

    def __delattr__(self, name) -> None:
        raise AttributeError("Wildcard is frozen")

    def __eq__(self, other) -> bool:
        return isinstance(other, Wildcard) and self.pattern == other.pattern

    def __hash__(self) -> int:
        return hash(("Wildcard", self.pattern))

    def __repr__(self) -> str:
        return f"Wildcard({self.pattern!r})"

    def __reduce__(self):
        return (Wildcard, (self.pattern,))

    def fits(self, token: str) -> bool:
        """Whether the one token fits the pattern."""
        return wildcard_fits(self.pattern, token)

    def within(self, tokens) -> bool:
        """Whether one of `tokens` (a set or a sequence) fits the pattern."""
        return any(wildcard_fits(self.pattern, t) for t in tokens)

    def native_pattern(self) -> Tuple[int, int, List[int]]:
        """(kind 0, arg 0, code points) as amdr_vocab_match takes it: '?' and '*' as the two values above U+10FFFF."""
        return 0, 0, [_ANY_ONE if c == "?" else _ANY_RUN if c == "*" else ord(c) for c in self.pattern]


class Fuzzy:
    """A word and its misspellings: Fuzzy("warrenty", edits=1) names every vocabulary token within `edits` (1 or 2) of the
    token under the optimal-string-alignment distance over code points — insertion, deletion, substitution and the
    transposition of two adjacent characters cost 1 each, no character is edited twice — the token itself included, and a
    chunk holds it when it holds at least one of them.  With the transposition Fuzzy("recieve") finds "receive"; plain
    Levenshtein would not.  The token has 1 to 64 code points and more than `edits` of them (ValueError).  Accepted
    wherever a Prefix is; compared as given (HybridRetriever.fuzzy cuts a string with the index's own tokeniser).  Frozen
    and hashable."""
    __slots__ = ("token", "edits")

    def __init__(self, token: str, edits: int = 1) -> None:
        if not isinstance(token, str):
            raise TypeError(f"Fuzzy: the token is a str, got {type(token).__name__}")
        if isinstance(edits, bool) or not isinstance(edits, (int, np.integer)):
            raise TypeError(f"Fuzzy: edits is an int, got {type(edits).__name__}")
        if not 1 <= int(edits) <= FUZZY_MAX_EDITS:
            raise ValueError(f"Fuzzy: edits of 1 or {FUZZY_MAX_EDITS}, got {int(edits)}")
        if not 1 <= len(token) <= WILDCARD_MAX_LEN:
            raise ValueError(f"Fuzzy: a token of 1 to {WILDCARD_MAX_LEN} characters, got {len(token)}")
        if len(token) <= int(edits):
            raise ValueError(f"Fuzzy: {token!r} within {int(edits)} edits names every token of up to {len(token) + int(edits)} "
                             f"characters; the token must be longer than the edits")
        object.__setattr__(self, "token", token)
        object.__setattr__(self, "edits", int(edits))

    def __setattr__(self, name, value) -> None:
        raise AttributeError("Fuzzy is frozen")

    def __delattr__(self, name) -> None:
        raise AttributeError("Fuzzy is frozen")

    def __eq__(self, other) -> bool:
        return isinstance(other, Fuzzy) and (self.token, self.edits) == (other.token, other.edits)

    def __hash__(self) -> int:
        return hash(("Fuzzy", self.token, self.edits))

    def __repr__(self) -> str:
        return f"Fuzzy({self.token!r}, edits={self.edits})"

    def __reduce__(self):
        return (Fuzzy, (self.token, self.edits))

    def fits(self, token: str) -> bool:
        """Whether the one token lies within the edits (the empty token never does)."""
        return bool(token) and abs(len(token) - len(self.token)) <= self.edits and osa_distance(self.token, token) <= self.edits

    def within(self, tokens) -> bool:
        """Whether one of `tokens` (a set or a sequence) lies within the edits."""
        return any(self.fits(t) for t in tokens)

    def native_pattern(self) -> Tuple[int, int, List[int]]:
        """(kind 1, edits, code points) as amdr_vocab_match takes it."""
        return 1, self.edits, [ord(c) for c in self.token]


_PATTERNS = (Wildcard, Fuzzy)  # what names vocabulary tokens by a scan (pack: `expansions`)


class OneOf:
    """Alternatives as ONE term: a chunk holds OneOf(m0, m1, ...) when it holds at least one member.  A member is a token
    (str), a Prefix, a Wildcard or a Fuzzy, at least one (ValueError); a Phrase, a Near or a OneOf as a member is a TypeError — alternatives
    between token sequences are not resolved yet.  OneOf("x") is the plain term, as a one-token Phrase is.  Accepted
    wherever a token is: as an entry of a Terms field or as a member of a tuple group — not inside a Phrase or a Near.
    Frozen and hashable: equal OneOfs (the same members in the same order) are equal and hash alike."""
    __slots__ = ("members",)

    def __init__(self, *members) -> None:
        if not members:
            raise ValueError("OneOf: at least one member")
        for m in members:
            if not isinstance(m, (str, Prefix) + _PATTERNS):
                raise TypeError(f"OneOf: a member is a str, a Prefix, a Wildcard or a Fuzzy, got {type(m).__name__}")
        object.__setattr__(self, "members", tuple(members))

    def __setattr__(self, name, value) -> None:
        raise AttributeError("OneOf is frozen")

    def __delattr__(self, name) -> None:
        raise AttributeError("OneOf is frozen")

    def __eq__(self, other) -> bool:
        return isinstance(other, OneOf) and self.members == other.members

    def __hash__(self) -> int:
        return hash(("OneOf", self.members))

    def __len__(self) -> int:
        return len(self.members)

    def __repr__(self) -> str:
        return "OneOf(" + ", ".join(repr(m) for m in self.members) + ")"

    def __reduce__(self):
        return (OneOf, self.members)

    def within(self, tokens) -> bool:
        """Whether `tokens` (a set or a sequence) holds one of the members."""
        return any(m in tokens if isinstance(m, str) else m.within(tokens) for m in self.members)


def fills(slot, token: str) -> bool:
    """Whether `token` FILLS `slot`, a member of a PhraseOf or a NearOf: it equals the str, starts with the Prefix's stem,
    fits the Wildcard, lies within the Fuzzy's edits, or fills a member of the OneOf."""
    if isinstance(slot, str):
        return token == slot
    if isinstance(slot, Prefix):
        return token.startswith(slot.stem)
    if isinstance(slot, _PATTERNS):
        return slot.fits(token)
    return any(fills(m, token) for m in slot.members)


def _slots(who: str, members, most: int) -> tuple:
    if not 2 <= len(members) <= most:
        raise ValueError(f"{who}: 2 to {most} members, got {len(members)}")
    for m in members:
        if not isinstance(m, (str, Prefix, OneOf) + _PATTERNS):
            # (the first three as the message has always named them: callers match on it)
            raise TypeError(f"{who}: a member is a str, a Prefix or a OneOf, a Wildcard or a Fuzzy, got {type(m).__name__}")
    return tuple(members)


class PhraseOf:
    """A phrase of token CLASSES ("secur! interest"): a chunk holds PhraseOf(m0, m1, ...) when its text has, at consecutive
    positions (never across two chunks), a token that FILLS m0, one that fills m1, ...  A member — a slot — is a token
    (str), a Prefix or a OneOf, and a token fills it when it equals the str, starts with the stem, or fills a member of the
    OneOf.  2 to 16 members (ValueError); a Phrase, a Near, a PhraseOf or a NearOf as a member is a TypeError.
    PhraseOf("a", "b") names the chunks Phrase("a", "b") names.  Accepted wherever a Phrase is.  Frozen and hashable."""
    __slots__ = ("members",)

    def __init__(self, *members) -> None:
        object.__setattr__(self, "members", _slots("PhraseOf", members, PHRASE_MAX_LEN))

    def __setattr__(self, name, value) -> None:
        raise AttributeError("PhraseOf is frozen")

    def __delattr__(self, name) -> None:
        raise AttributeError("PhraseOf is frozen")

    def __eq__(self, other) -> bool:
        return isinstance(other, PhraseOf) and self.members == other.members

    def __hash__(self) -> int:
        return hash(("PhraseOf", self.members))

    def __len__(self) -> int:
        return len(self.members)

    def __repr__(self) -> str:
        return "PhraseOf(" + ", ".join(repr(m) for m in self.members) + ")"

    def __reduce__(self):
        return (PhraseOf, self.members)

    def within(self, tokens: Sequence[str]) -> bool:
        """Whether the token sequence `tokens` holds this phrase (the plain window scan)."""
        L, want = len(self.members), self.members
        return any(all(fills(want[j], tokens[p + j]) for j in range(L)) for p in range(len(tokens) - L + 1))


class NearOf:
    """Proximity of token CLASSES (sell! /5 good!): NearOf(m0, m1, ..., distance=n) with members as PhraseOf's.
      ordered=False  some run of at most n + 1 consecutive tokens admits an assignment of the members to DISTINCT positions
                     of the run, each token filling its member — a bipartite matching: NearOf(P, P, distance=n) needs two
                     positions.
      ordered=True   there are positions p0 < p1 < ... with token p_i filling member i and the last at most n behind the
                     first.
    2 to 8 members and 1 <= distance <= 255 (ValueError); a Phrase, a Near, a PhraseOf or a NearOf as a member is a
    TypeError.  NearOf("a", "b", distance=5) names the chunks Near("a", "b", distance=5) names.  The GPU resolves the
    unordered form only when the members' token sets are pairwise equal or disjoint: pack() raises ValueError for
    NearOf("seller", Prefix("sell"), distance=3).  Accepted wherever a Near is.  Frozen and hashable."""
    __slots__ = ("members", "distance", "ordered")

    def __init__(self, *members, distance: int, ordered: bool = False) -> None:
        members = _slots("NearOf", members, NEAR_MAX_TERMS)
        if isinstance(distance, bool) or not isinstance(distance, (int, np.integer)):
            raise TypeError(f"NearOf: distance is an int, got {type(distance).__name__}")
        if not 1 <= int(distance) <= NEAR_MAX_DIST:
            raise ValueError(f"NearOf: a distance of 1 to {NEAR_MAX_DIST}, got {int(distance)}")
        object.__setattr__(self, "members", members)
        object.__setattr__(self, "distance", int(distance))
        object.__setattr__(self, "ordered", bool(ordered))

    def __setattr__(self, name, value) -> None:
        raise AttributeError("NearOf is frozen")

    def __delattr__(self, name) -> None:
        raise AttributeError("NearOf is frozen")

    def _key(self):
        return (self.members, self.distance, self.ordered)

    def __eq__(self, other) -> bool:
        return isinstance(other, NearOf) and self._key() == other._key()

    def __hash__(self) -> int:
        return hash(("NearOf",) + self._key())

    def __len__(self) -> int:
        return len(self.members)

    def __repr__(self) -> str:
        return ("NearOf(" + ", ".join(repr(m) for m in self.members) + f", distance={self.distance}"
                + (", ordered=True" if self.ordered else "") + ")")

    def __reduce__(self):
        return (_make_near_of, (self.members, self.distance, self.ordered))

    def within(self, tokens: Sequence[str]) -> bool:
        """Whether the token sequence `tokens` holds this NearOf: every anchor with the earliest next match per member
        (ordered), a bipartite matching by augmenting paths in every window (unordered)."""
        n, want, M = self.distance, self.members, len(self.members)
        if self.ordered:
            for s in range(len(tokens)):
                if not fills(want[0], tokens[s]):
                    continue
                j = 1
                for t in tokens[s + 1:s + n + 1]:
                    if fills(want[j], t):
                        j += 1
                        if j == M:
                            return True
            return False
        for s in range(len(tokens)):
            win = tokens[s:s + n + 1]
            if len(win) < M:
                break  # (every later window is no longer)
            may = [[q for q, t in enumerate(win) if fills(m, t)] for m in want]  # the positions each member may take
            taken: Dict[int, int] = {}  # position -> the member it is assigned to

            def place(j: int, seen: set) -> bool:
                for q in may[j]:
                    if q in seen:
                        continue
                    seen.add(q)
                    if q not in taken or place(taken[q], seen):
                        taken[q] = j
                        return True
                return False
            if all(place(j, set()) for j in range(M)):
                return True
        return False


def _make_near_of(members, distance, ordered) -> NearOf:
    return NearOf(*members, distance=distance, ordered=ordered)


WITHIN_MAX_TERMS = 8  # members of a Within (unit_span_rule.hpp kUsMaxSlots)
UNITS = ("sentence", "paragraph")
BREAK_SENTENCE, BREAK_PARAGRAPH = 1, 2  # the bits of a break byte (retrieval/units.py)


class Within:
    """The same-sentence and same-paragraph connectors (/s and +s, /p and +p of a Boolean legal search): a chunk holds
    Within(m0, m1, ..., unit="sentence") when ONE sentence of its text holds every member, and unit="paragraph" when one
    paragraph does.  A chunk's tokens are partitioned into units at the tokens whose break flag says so (retrieval/units.py:
    a sentence begins behind . ? ! 。 ！ ？, a paragraph behind a line break, a paragraph start is a sentence start, the
    first token begins both).  Members are a NearOf's: a token (str), a Prefix, a OneOf, a Wildcard or a Fuzzy.
      ordered=False  some unit admits an assignment of the members to DISTINCT positions of that unit, each token filling
                     its member — a bipartite matching: Within("goods", "goods") needs two in one sentence.
      ordered=True   there are positions p0 < p1 < ... inside one unit with token p_i filling member i.
    2 to 8 members, unit "sentence" or "paragraph" (ValueError); a Phrase, a Near, a PhraseOf, a NearOf or a Within as a
    member is a TypeError.  The GPU resolves the unordered form only when the members' token sets are pairwise equal or
    disjoint: pack() raises ValueError for Within("seller", Prefix("sell")).  Accepted wherever a Near is.  Frozen and
    hashable."""
    __slots__ = ("members", "unit", "ordered")

    def __init__(self, *members, unit: str = "sentence", ordered: bool = False) -> None:
        members = _slots("Within", members, WITHIN_MAX_TERMS)
        if not isinstance(unit, str):
            raise TypeError(f"Within: unit is a str, got {type(unit).__name__}")
        if unit not in UNITS:
            raise ValueError(f"Within: unit is 'sentence' or 'paragraph', got {unit!r}")
        object.__setattr__(self, "members", members)
        object.__setattr__(self, "unit", unit)
        object.__setattr__(self, "ordered", bool(ordered))

    def __setattr__(self, name, value) -> None:
        raise AttributeError("Within is frozen")

    def __delattr__(self, name) -> None:
        raise AttributeError("Within is frozen")

    def _key(self):
        return (self.members, self.unit, self.ordered)

    def __eq__(self, other) -> bool:
        return isinstance(other, Within) and self._key() == other._key()

    def __hash__(self) -> int:
        return hash(("Within",) + self._key())

    def __len__(self) -> int:
        return len(self.members)

    def __repr__(self) -> str:
        return ("Within(" + ", ".join(repr(m) for m in self.members) + f", unit={self.unit!r}"
                + (", ordered=True" if self.ordered else "") + ")")

    def __reduce__(self):
        return (_make_within, (self.members, self.unit, self.ordered))

    @property
    def kind(self) -> int:
        """The item kind of the ABI: bit 0 ordered, bit 1 paragraph."""
        return (1 if self.ordered else 0) | (2 if self.unit == "paragraph" else 0)

    def within(self, tokens: Sequence[str], breaks: Sequence[int]) -> bool:
        """Whether the token sequence `tokens` with the break flags `breaks` (one per token) holds this Within: the plain
        scan of every unit — the earliest next match per member (ordered), a bipartite matching by augmenting paths
        (unordered)."""
        if len(breaks) != len(tokens):
            raise ValueError(f"Within.within: {len(tokens)} tokens, {len(breaks)} break flags")
        bit = BREAK_PARAGRAPH if self.unit == "paragraph" else BREAK_SENTENCE
        want, M = self.members, len(self.members)
        begin = 0
        for end in range(1, len(tokens) + 1):
            if end < len(tokens) and not (int(breaks[end]) & bit):
                continue
            unit, begin = tokens[begin:end], end
            if len(unit) < M:
                continue
            if self.ordered:
                j = 0
                for t in unit:
                    if fills(want[j], t):
                        j += 1
                        if j == M:
                            return True
                continue
            may = [[q for q, t in enumerate(unit) if fills(m, t)] for m in want]  # the positions each member may take
            taken: Dict[int, int] = {}  # position -> the member it is assigned to

            def place(j: int, seen: set) -> bool:
                for q in may[j]:
                    if q in seen:
                        continue
                    seen.add(q)
                    if q not in taken or place(taken[q], seen):
                        taken[q] = j
                        return True
                return False
            if all(place(j, set()) for j in range(M)):
                return True
        return False


def _make_within(members, unit, ordered) -> Within:
    return Within(*members, unit=unit, ordered=ordered)


Member = Union[str, Phrase, Near, Prefix, OneOf, PhraseOf, NearOf, Wildcard, Fuzzy, Within]
Group = Tuple[Member, ...]
_MEMBERS = (str, Phrase, Near, Prefix, OneOf, PhraseOf, NearOf, Wildcard, Fuzzy, Within)
_SPANS = (Phrase, Near, PhraseOf, NearOf)  # what needs the token SEQUENCE


def _member(t) -> Member:
    if isinstance(t, (Near, Prefix, PhraseOf, NearOf, Within) + _PATTERNS):
        return t
    if isinstance(t, OneOf):
        return t.members[0] if len(t) == 1 else t  # one member is that member
    if isinstance(t, Phrase):
        return t.tokens[0] if len(t) == 1 else t  # one token is the plain term
    return str(t)


def _groups(x, field: str) -> Optional[Tuple[Group, ...]]:
    if x is None:
        return None
    if isinstance(x, _MEMBERS):
        x = (x,)
    out: List[Group] = []
    for e in x:
        g = (_member(e),) if isinstance(e, _MEMBERS) else tuple(_member(t) for t in e)
        if not g:
            raise ValueError(f"Terms.{field}: an empty group names no token")
        out.append(g)
    return tuple(out) or None


@dataclass(frozen=True)
class Terms:
    """What a chunk's text must contain.  An entry is one vocabulary token (`str`) or a tuple of tokens, one GROUP: a
    chunk satisfies a group when it holds EVERY token of it, anywhere — a conjunction.  The tokens next to each other
    in order are a `Phrase`, the tokens within a distance of each other a `Near`; either stands wherever a token stands:
    as an entry, or inside a tuple group.  So do a `Prefix` (every token with that stem) and a `OneOf` (alternatives as
    one term): all_of=[(OneOf("buyer", "purchaser"), Prefix("sell"))] is (buyer OR purchaser) AND sell!.  For a
    char-cut Han index a word is the phrase of its characters, Phrase("合", "同") (the group ("合", "同") also names
    every chunk that holds 同 … 合).
      all_of   every entry must be satisfied (each entry is a MUST group);
      any_of   at least one entry must be satisfied;
      none_of  no entry may be satisfied (a tuple excludes only the chunks that hold ALL its tokens).
    Tokens are compared exactly with the live index's vocabulary (`BM25Okapi.vocab()`): pass them as the index's
    tokeniser cuts them — the reference's English index is lower-cased while its queries are not, so
    "Seller" names no chunk of it.  A token the vocabulary does not hold is present in no chunk: it empties all_of,
    is ignored in any_of unless every entry is unknown, and is ignored in none_of.  A field left at None does not
    restrict; a Terms with nothing given is unrestricted and behaves like None.  Frozen and hashable: equal Terms are
    equal and hash alike (fields are stored as tuples of tuples)."""
    all_of: Optional[Tuple[Group, ...]] = None
    any_of: Optional[Tuple[Group, ...]] = None
    none_of: Optional[Tuple[Group, ...]] = None

    def __post_init__(self) -> None:
        for f in ("all_of", "any_of", "none_of"):
            object.__setattr__(self, f, _groups(getattr(self, f), f))

    @property
    def unrestricted(self) -> bool:
        return self.all_of is None and self.any_of is None and self.none_of is None

    def groups(self) -> List[Tuple[int, Group]]:
        """[(kind, tokens)] in the order the operands hold them: all_of, any_of, none_of."""
        return ([(MUST, g) for g in self.all_of or ()] + [(ANY, g) for g in self.any_of or ()]
                + [(NOT, g) for g in self.none_of or ()])

    @property
    def has_phrase(self) -> bool:
        return any(isinstance(t, Phrase) for _, g in self.groups() for t in g)

    @property
    def has_near(self) -> bool:
        return any(isinstance(t, Near) for _, g in self.groups() for t in g)

    @property
    def has_union(self) -> bool:
        return any(isinstance(t, (Prefix, OneOf)) for _, g in self.groups() for t in g)

    @property
    def has_class_span(self) -> bool:
        return any(isinstance(t, (PhraseOf, NearOf)) for _, g in self.groups() for t in g)

    @property
    def has_within(self) -> bool:
        return any(isinstance(t, Within) for _, g in self.groups() for t in g)

    def patterns(self) -> List[Any]:
        """The distinct Wildcards and Fuzzys of this Terms in order of appearance, wherever they stand: as an entry, in a
        tuple group, or as a member of a OneOf, a PhraseOf, a NearOf or a Within (also inside a OneOf of those)."""
        seen: Dict[Any, None] = {}

        def walk(t) -> None:
            if isinstance(t, _PATTERNS):
                seen.setdefault(t)
            elif isinstance(t, (OneOf, PhraseOf, NearOf, Within)):
                for m in t.members:
                    walk(m)
        for _, g in self.groups():
            for t in g:
                walk(t)
        return list(seen)

    @property
    def has_pattern(self) -> bool:
        """Whether a Wildcard or a Fuzzy stands anywhere in this Terms: pack() then needs their `expansions`."""
        return bool(self.patterns())

    def matches(self, tokens, breaks=None) -> bool:
        """The rule on one document's tokens (host check; the kernels apply term_scope_rule.hpp, phrase_rule.hpp,
        union_rule.hpp, class_span_rule.hpp and unit_span_rule.hpp): a token set or sequence — with a Phrase, a Near, a
        PhraseOf, a NearOf or a Within present, the token SEQUENCE in text order (TypeError for a set); a Prefix, a
        Wildcard, a Fuzzy or a OneOf takes either.  breaks: the document's break flags, one per token (retrieval/units.py
        break_flags); a Terms that holds a Within raises TypeError without them."""
        if self.has_within and breaks is None:
            raise TypeError("Terms.matches: a Terms with a Within needs the document's break flags (breaks=)")
        if self.has_phrase or self.has_near or self.has_class_span or self.has_within:
            if isinstance(tokens, (set, frozenset, dict)) or not isinstance(tokens, Sequence):
                what = ("Phrase" if self.has_phrase else "Near" if self.has_near else
                        "PhraseOf or a NearOf" if self.has_class_span else "Within")
                raise TypeError(f"Terms.matches: a Terms with a {what} needs the document's token sequence, not a set")
            have = set(tokens)
        else:
            have = tokens if isinstance(tokens, (set, frozenset, dict)) else set(tokens)
        sat = lambda g: all(t.within(tokens, breaks) if isinstance(t, Within) else  # noqa: E731
                            t.within(tokens) if isinstance(t, _SPANS) else
                            t.within(have) if isinstance(t, (Prefix, OneOf) + _PATTERNS) else t in have for t in g)
        return (all(sat(g) for g in self.all_of or ()) and (self.any_of is None or any(sat(g) for g in self.any_of))
                and not any(sat(g) for g in self.none_of or ()))


def driver_length(groups: Sequence[Tuple[int, Sequence[int]]], df: Sequence[int], base_len: Optional[int], n_docs: int) -> int:
    """The candidate count of a constraint by the rule of term_scope_rule.hpp (ts_driver): the shortest of { the base
    scope, the posting list of each MUST term }; 0 with an unknown MUST term; n_docs with neither a MUST term nor a base.
    groups: (kind, term ids); df[t]: the document frequency of term t — for the id of a phrase (a virtual list, ids behind
    the vocabulary's: pack) the UPPER bound of its list's length, the smallest document frequency among its tokens.  The
    device's driver is the shortest of the true lengths, each <= its bound, so the result is an upper bound of it."""
    best = base_len
    for kind, ids in groups:
        if kind != MUST:
            continue
        for t in ids:
            if t < 0 or t >= len(df):
                return 0
            if best is None or df[t] < best:
                best = int(df[t])
    return int(n_docs) if best is None else int(best)


@dataclass
class TermTable:
    """The operands of one amdr_term_scope call (pack)."""
    ops: Tuple[np.ndarray, ...]   # _native.BM25Index.TERM_OPS order
    qscope: np.ndarray            # i32 [len(pairs)]: each question's constraint
    n_cons: int
    n_groups: int
    n_base: int
    driver_lens: np.ndarray       # i64 [n_cons]
    cand_max: int                 # the longest driver
    rows_cap: int                 # the sum of the drivers: no table is longer
    # the phrases of the batch, each stored once; phrase p is term id len(vocab) + p in `ops` (amdr_phrase_lists)
    phr_ops: Tuple[np.ndarray, ...] = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))  # phr_ptr, phr_terms
    phrases: Tuple[Phrase, ...] = ()
    phr_cand_max: int = 0         # the longest phrase driver: the largest of the phrases' upper bounds
    phr_rows_cap: int = 0         # the sum of the upper bounds

    # the Nears of the batch, each stored once; Near j is term id len(vocab) + n_phr + j in `ops`.  With a Near present
    # span_ops holds the items of the ONE span step (amdr_span_lists): the phrases as kind 0, then the Nears
    span_ops: Tuple[np.ndarray, ...] = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32),
                                        np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))  # ptr, terms, kind, dist
    nears: Tuple[Near, ...] = ()
    near_cand_max: int = 0        # the longest Near driver: the largest of the Nears' upper bounds
    near_rows_cap: int = 0        # the sum of the upper bounds

    # the unions of the batch (a Prefix or a OneOf that names two or more vocabulary tokens), equal sets of term ids stored
    # once; union u is term id len(vocab) + n_phr + n_near + u in `ops`, behind the Nears (amdr_union_lists).  Attributes
    # with class-level defaults, set per table by pack(), and NOT dataclass fields: the fields above stay the last ones
    union_ops = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))  # ptr i64 [n_union + 1], terms i32
    unions = ()          # per union the first Prefix / OneOf of the batch that names it
    union_rows_cap = 0   # the sum of the upper bounds min(n_docs, the sum of the tokens' document frequencies)

    # the class spans of the batch (a PhraseOf or a NearOf with at least one slot that is a union), equal ones — compared
    # after resolution — stored once; class span c is term id len(vocab) + n_phr + n_near + n_union + c, behind the unions
    # (amdr_class_spans).  A slot is a plain term id or the term id of a union.  Class-level defaults as the unions'
    cspan_ops = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32),
                 np.zeros(0, dtype=np.int32))  # ptr i64 [n_cspan + 1], slots i32, kind i32 (SpanKind), dist i32
    cspans = ()          # per class span the first PhraseOf / NearOf of the batch that names it
    cspan_cand_max = 0   # the largest of the upper bounds: the smallest slot bound of each item
    cspan_rows_cap = 0   # their sum

    # the unit items of the batch (a Within), equal ones — compared after resolution — stored once; unit item w is term id
    # len(vocab) + n_phr + n_near + n_union + n_cspan + w, behind the class spans (amdr_unit_spans).  A slot is a plain term
    # id or the term id of a union.  Class-level defaults as the unions'
    unit_ops = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))  # ptr, slots, kind
    units = ()           # per unit item the first Within of the batch that names it
    unit_cand_max = 0    # the largest of the upper bounds: the smallest slot bound of each item
    unit_rows_cap = 0    # their sum

    @property
    def n_unit(self) -> int:
        return len(self.units)

    @property
    def n_cspan(self) -> int:
        return len(self.cspans)

    @property
    def n_phr(self) -> int:
        return len(self.phrases)

    @property
    def n_near(self) -> int:
        return len(self.nears)

    @property
    def n_union(self) -> int:
        return len(self.unions)

    @property
    def span_cand_max(self) -> int:
        return max(self.phr_cand_max, self.near_cand_max)

    @property
    def span_rows_cap(self) -> int:
        return self.phr_rows_cap + self.near_rows_cap

    def span_item(self, i: int):
        """Item i of the span step: the Phrase or the Near."""
        return self.phrases[i] if i < self.n_phr else self.nears[i - self.n_phr]

    def list_item(self, i: int):
        """What virtual list i of the term step stands for: the Phrase, the Near, the union's Prefix / OneOf, the class
        span's PhraseOf / NearOf, or the unit item's Within."""
        n_span = self.n_phr + self.n_near
        if i < n_span:
            return self.span_item(i)
        if i < n_span + self.n_union:
            return self.unions[i - n_span]
        i -= n_span + self.n_union
        return self.cspans[i] if i < self.n_cspan else self.units[i - self.n_cspan]


def prefix_tokens(stem: str, sorted_vocab: Sequence[str]) -> List[str]:
    """The tokens of `sorted_vocab` (ascending by code point, BM25Okapi.sorted_vocab()) that start with `stem`: they stand
    next to each other, from the first token >= stem."""
    at = bisect_left(sorted_vocab, stem)
    end = at
    while end < len(sorted_vocab) and sorted_vocab[end].startswith(stem):
        end += 1
    return list(sorted_vocab[at:end])


def pack(pairs: Sequence[Tuple[Optional[Scope], Terms]], vocab: Mapping[str, int], doc_freq: Mapping[str, int], n_docs: int,
         base_rows=None, sorted_vocab: Optional[Sequence[str]] = None,
         expansions: Optional[Mapping[Any, Any]] = None) -> TermTable:
    """The operand arrays of a batch of (Scope | None, Terms) pairs.  Equal pairs are stored once (as ScopeResolver.table
    stores equal scopes once) and `qscope` names each pair's constraint; equal base scopes are stored once as well.
    vocab / doc_freq: the live host model's token -> term id and token -> document frequency (BM25Okapi.vocab(),
    _doc_frequencies()); base_rows(scope) -> the ascending int64 rows of a Scope (ScopeResolver.rows), needed only when a
    pair carries one.  The bounds come from the host model by the header's own rule: cand_max = the longest driver,
    rows_cap = the sum of the drivers.  Equal phrases are stored once as well and stand in the table as the term ids
    len(vocab) + p; the host knows only an upper bound of a phrase's list — the smallest document frequency among its
    tokens, 0 with an unknown one — which serves both steps: phr_cand_max / phr_rows_cap are the largest and the sum of
    these, and the drivers of the term step are computed with them (driver_length).  Equal Nears are stored once too and
    stand as the term ids len(vocab) + n_phr + j, behind the phrases, with the same upper bound (a chunk that holds a Near
    holds each of its tokens): near_cand_max / near_rows_cap; a table with a Near carries span_ops, the items of the one
    span step.  A table without one is field for field the table of the phrases alone.
    A Prefix is expanded by bisection over sorted_vocab (the vocabulary's tokens ascending by code point,
    BM25Okapi.sorted_vocab(); computed from `vocab` when not given) and a OneOf into its members' tokens; what either names
    is the sorted tuple of its DISTINCT KNOWN term ids.  None: the id -1, a token the vocabulary does not hold; one: that
    plain term; more than PREFIX_MAX_TERMS: ValueError.  Two or more are a union item (amdr_union_lists): equal tuples are
    stored once — Prefix("sell") and the OneOf of its tokens share a list — and union u stands as the term id
    len(vocab) + n_phr + n_near + u, behind the Nears, with the upper bound min(n_docs, the sum of the ids' document
    frequencies) of its list's length: union_rows_cap is the sum of these, and the drivers are computed with them.  A
    table without a union is field for field the table of the phrases and the Nears alone.
    A PhraseOf or a NearOf has each slot resolved as a Prefix or a OneOf is (a str: its term id or -1).  When every slot is
    a plain id the item IS the plain Phrase / Near of those tokens and is stored as that one: the same slot, the same list,
    the old step.  Otherwise it is a class span (amdr_class_spans): a union among its slots registers a union item even when
    nothing else in the batch uses it, equal class spans — compared after resolution — are stored once, and class span c
    stands as the term id len(vocab) + n_phr + n_near + n_union + c, behind the unions, with the smallest slot bound (df of
    a plain id, 0 of the id -1, the union's bound) as its upper bound: cspan_cand_max / cspan_rows_cap.  An unordered NearOf
    whose slots' id sets intersect without being equal is a ValueError: the device's first-unfilled-slot tally is the
    matching only for pairwise equal or disjoint slots.  A table without a class span is field for field the table without.
    A Wildcard or a Fuzzy names the tokens `expansions` holds for it — {pattern: the (token, distance) pairs, or the bare
    tokens, it names}, VocabMatcher.expand's result; this function stays plain host code and scans no vocabulary — and
    resolves from there on exactly as a Prefix does: none -> -1, one -> that plain term, two or more -> a union item that
    shares its slot with an equal OneOf or Prefix.  A pattern without an entry is a ValueError.  Without a pattern
    `expansions` is not looked at and the table is field for field what it was.
    A Within has each member resolved as a NearOf's slot is, and is ALWAYS a unit item (amdr_unit_spans), plain members or
    not: a union among its members registers a union item, equal Withins — compared after resolution: the same ids, unit and
    order — are stored once, and unit item w stands as the term id len(vocab) + n_phr + n_near + n_union + n_cspan + w,
    behind the class spans, with the smallest slot bound as its upper bound: unit_cand_max / unit_rows_cap.  An unordered
    Within whose members' id sets intersect without being equal is a ValueError (class_span_rule.hpp's reason).  A table
    without a Within is field for field the table without."""
    n_vocab = len(vocab)
    df_by_id = np.zeros(n_vocab, dtype=np.int64)
    for w, t in vocab.items():
        df_by_id[t] = doc_freq.get(w, 0)
    union_slot: Dict[Tuple[int, ...], int] = {}
    union_first: List[Any] = []
    union_bound: List[int] = []
    union_ids: List[Tuple[int, ...]] = []
    sorted_held = [sorted_vocab]

    def union_id(t):
        """The id a Prefix or a OneOf stands for: -1, a plain term's, or the placeholder ("u", u) of union u."""
        words: List[str] = []
        for m in (t.members if isinstance(t, OneOf) else (t,)):
            if isinstance(m, _PATTERNS):
                if expansions is None or m not in expansions:
                    raise ValueError(f"{m!r}: pack() was given no expansion of this pattern (expansions=: "
                                     f"VocabMatcher.expand resolves the patterns of a batch)")
                words.extend(e if isinstance(e, str) else e[0] for e in expansions[m])
            elif isinstance(m, Prefix):
                if sorted_held[0] is None:
                    sorted_held[0] = sorted(vocab)
                words.extend(prefix_tokens(m.stem, sorted_held[0]))
            else:
                words.append(m)
        ids = tuple(sorted({vocab[w] for w in words if w in vocab}))
        if len(ids) > PREFIX_MAX_TERMS:
            raise ValueError(f"{t!r} names {len(ids)} vocabulary tokens, more than {PREFIX_MAX_TERMS}: give a longer stem"
                             if not isinstance(t, _PATTERNS) else
                             f"{t!r} names {len(ids)} vocabulary tokens, more than {PREFIX_MAX_TERMS}: give a narrower pattern")
        if len(ids) < 2:
            return ids[0] if ids else -1
        u = union_slot.get(ids)
        if u is None:
            u = union_slot[ids] = len(union_bound)
            union_first.append(t)
            union_ids.append(ids)
            union_bound.append(min(int(n_docs), int(sum(df_by_id[i] for i in ids))))
        return ("u", u)

    phr_slot: Dict[Phrase, int] = {}
    phr_ptr, phr_terms, phr_bound = [0], [], []

    near_slot: Dict[Near, int] = {}
    near_ids: List[List[int]] = []
    near_bound: List[int] = []

    cspan_slot: Dict[Any, int] = {}
    cspan_first: List[Any] = []
    cspan_slots: List[list] = []
    cspan_bound: List[int] = []
    word_held: List[Optional[Dict[int, str]]] = [None]

    def class_span_id(t):
        """The id a PhraseOf or a NearOf stands for: that of the equal plain Phrase / Near, or the placeholder ("c", c)."""
        near = isinstance(t, NearOf)
        ids = [vocab.get(m, -1) if isinstance(m, str) else union_id(m) for m in t.members]
        if all(not isinstance(i, tuple) and (i >= 0 or isinstance(m, str)) for i, m in zip(ids, t.members)):
            if word_held[0] is None:
                word_held[0] = {i: w for w, i in vocab.items()}
            words = [m if isinstance(m, str) else word_held[0][i] for i, m in zip(ids, t.members)]
            return term_id(Near(*words, distance=t.distance, ordered=t.ordered) if near else Phrase(*words))
        sets = [frozenset(union_ids[i[1]]) if isinstance(i, tuple) else frozenset([i] if i >= 0 else []) for i in ids]
        if near and not t.ordered:
            for j in range(len(sets)):
                for k in range(j):
                    if sets[j] & sets[k] and sets[j] != sets[k]:
                        raise ValueError(f"{t!r}: members {k} and {j} name overlapping, unequal token sets "
                                         f"({t.members[k]!r}, {t.members[j]!r}); the unordered form is resolved only for "
                                         f"members that are pairwise equal or disjoint")
        key = (2 if near and t.ordered else 1 if near else 0, tuple(ids), t.distance if near else 0)
        c = cspan_slot.get(key)
        if c is None:
            c = cspan_slot[key] = len(cspan_bound)
            cspan_first.append(t)
            cspan_slots.append(ids)
            cspan_bound.append(min(union_bound[i[1]] if isinstance(i, tuple) else int(df_by_id[i]) if i >= 0 else 0 for i in ids))
        return ("c", c)

    unit_slot: Dict[Any, int] = {}
    unit_first: List[Any] = []
    unit_slots: List[list] = []
    unit_bound: List[int] = []

    def unit_id(t):
        """The placeholder ("w", w) of the unit item a Within stands for."""
        ids = [vocab.get(m, -1) if isinstance(m, str) else union_id(m) for m in t.members]
        sets = [frozenset(union_ids[i[1]]) if isinstance(i, tuple) else frozenset([i] if i >= 0 else []) for i in ids]
        if not t.ordered:
            for j in range(len(sets)):
                for k in range(j):
                    if sets[j] & sets[k] and sets[j] != sets[k]:
                        raise ValueError(f"{t!r}: members {k} and {j} name overlapping, unequal token sets "
                                         f"({t.members[k]!r}, {t.members[j]!r}); the unordered form is resolved only for "
                                         f"members that are pairwise equal or disjoint")
        key = (t.kind, tuple(ids))
        w = unit_slot.get(key)
        if w is None:
            w = unit_slot[key] = len(unit_bound)
            unit_first.append(t)
            unit_slots.append(ids)
            unit_bound.append(min(union_bound[i[1]] if isinstance(i, tuple) else int(df_by_id[i]) if i >= 0 else 0 for i in ids))
        return ("w", w)

    def term_id(t):
        if isinstance(t, Within):  # (numbered behind the class spans: a placeholder)
            return unit_id(t)
        if isinstance(t, (PhraseOf, NearOf)):  # (numbered behind the unions: a placeholder, or the plain form's id)
            return class_span_id(t)
        if isinstance(t, Near):  # (numbered behind the phrases once all of those are known: a placeholder until then)
            j = near_slot.get(t)
            if j is None:
                j = near_slot[t] = len(near_bound)
                ids = [vocab.get(w, -1) for w in t.tokens]
                near_ids.append(ids)
                near_bound.append(0 if min(ids) < 0 else int(min(df_by_id[i] for i in ids)))
            return ("n", j)
        if isinstance(t, (Prefix, OneOf) + _PATTERNS):  # (numbered behind the Nears: a placeholder as well)
            return union_id(t)
        if not isinstance(t, Phrase):
            return vocab.get(t, -1)
        p = phr_slot.get(t)
        if p is None:
            p = phr_slot[t] = len(phr_bound)
            ids = [vocab.get(w, -1) for w in t.tokens]
            phr_terms.extend(ids)
            phr_ptr.append(len(phr_terms))
            phr_bound.append(0 if min(ids) < 0 else int(min(df_by_id[i] for i in ids)))
        return n_vocab + p
    slot: Dict[Any, int] = {}
    base_slot: Dict[Scope, int] = {}
    bases: List[np.ndarray] = []
    grp_ptr, grp_kind, grp_term_ptr, grp_terms, cons_base, cons_groups = [0], [], [0], [], [], []
    qscope = np.empty(len(pairs), dtype=np.int32)
    for i, (scope, terms) in enumerate(pairs):
        if not isinstance(terms, Terms):
            raise TypeError(f"terms[{i}] is not a Terms")
        if scope is not None and scope.unrestricted:
            scope = None
        j = slot.get((scope, terms))
        if j is None:
            j = slot[(scope, terms)] = len(cons_base)
            b = -1
            if scope is not None:
                b = base_slot.get(scope)
                if b is None:
                    b = base_slot[scope] = len(bases)
                    bases.append(np.ascontiguousarray(base_rows(scope), dtype=np.int64))
            groups = [(kind, [term_id(t) for t in g]) for kind, g in terms.groups()]
            grp_ptr.append(grp_ptr[-1] + len(groups))
            cons_base.append(b)
            cons_groups.append(groups)
        qscope[i] = j
    n_phr = len(phr_bound)
    behind = {"n": n_vocab + n_phr, "u": n_vocab + n_phr + len(near_bound)}
    behind["c"] = behind["u"] + len(union_bound)
    behind["w"] = behind["c"] + len(cspan_bound)
    cons_groups = [[(kind, [behind[t[0]] + t[1] if isinstance(t, tuple) else t for t in ids]) for kind, ids in groups]
                   for groups in cons_groups]
    for groups in cons_groups:
        for kind, ids in groups:
            grp_kind.append(kind)
            grp_terms.extend(ids)
            grp_term_ptr.append(len(grp_terms))
    base_ptr = np.zeros(len(bases) + 1, dtype=np.int64)
    if bases:
        np.cumsum([b.size for b in bases], out=base_ptr[1:])
    ops = (np.asarray(grp_ptr, dtype=np.int64), np.asarray(grp_kind, dtype=np.int32), np.asarray(grp_term_ptr, dtype=np.int64),
           np.asarray(grp_terms, dtype=np.int32), base_ptr,
           np.concatenate(bases) if bases else np.zeros(0, dtype=np.int64), np.asarray(cons_base, dtype=np.int32))
    df_all = np.concatenate([df_by_id, np.asarray(phr_bound + near_bound + union_bound + cspan_bound + unit_bound, dtype=np.int64)])  # (all known by now)
    lens_a = np.asarray([driver_length(g, df_all, int(bases[b].size) if b >= 0 else None, n_docs)
                         for g, b in zip(cons_groups, cons_base)], dtype=np.int64)
    tt = TermTable(ops, qscope, len(cons_base), len(grp_kind), len(bases), lens_a,
                   int(lens_a.max()) if lens_a.size else 0, int(lens_a.sum()),
                   (np.asarray(phr_ptr, dtype=np.int64), np.asarray(phr_terms, dtype=np.int32)), tuple(phr_slot),
                   max(phr_bound, default=0), int(sum(phr_bound)))
    if near_slot:
        item_ptr, item_terms = list(phr_ptr), list(phr_terms)
        for ids in near_ids:
            item_terms.extend(ids)
            item_ptr.append(len(item_terms))
        nears = tuple(near_slot)
        tt.span_ops = (np.asarray(item_ptr, dtype=np.int64), np.asarray(item_terms, dtype=np.int32),
                       np.asarray([0] * n_phr + [2 if x.ordered else 1 for x in nears], dtype=np.int32),
                       np.asarray([0] * n_phr + [x.distance for x in nears], dtype=np.int32))
        tt.nears, tt.near_cand_max, tt.near_rows_cap = nears, max(near_bound), int(sum(near_bound))
    if union_slot:
        u_ptr = np.zeros(len(union_slot) + 1, dtype=np.int64)
        np.cumsum([len(ids) for ids in union_slot], out=u_ptr[1:])
        tt.union_ops = (u_ptr, np.asarray([i for ids in union_slot for i in ids], dtype=np.int32))
        tt.unions, tt.union_rows_cap = tuple(union_first), int(sum(union_bound))
    if cspan_slot:
        c_ptr = np.zeros(len(cspan_slot) + 1, dtype=np.int64)
        np.cumsum([len(ids) for ids in cspan_slots], out=c_ptr[1:])
        tt.cspan_ops = (c_ptr, np.asarray([behind["u"] + i[1] if isinstance(i, tuple) else i for ids in cspan_slots for i in ids],
                                          dtype=np.int32),
                        np.asarray([k[0] for k in cspan_slot], dtype=np.int32), np.asarray([k[2] for k in cspan_slot], dtype=np.int32))
        tt.cspans, tt.cspan_cand_max, tt.cspan_rows_cap = tuple(cspan_first), max(cspan_bound), int(sum(cspan_bound))
    if unit_slot:
        w_ptr = np.zeros(len(unit_slot) + 1, dtype=np.int64)
        np.cumsum([len(ids) for ids in unit_slots], out=w_ptr[1:])
        tt.unit_ops = (w_ptr, np.asarray([behind["u"] + i[1] if isinstance(i, tuple) else i for ids in unit_slots for i in ids],
                                         dtype=np.int32), np.asarray([k[0] for k in unit_slot], dtype=np.int32))
        tt.units, tt.unit_cand_max, tt.unit_rows_cap = tuple(unit_first), max(unit_bound), int(sum(unit_bound))
    return tt

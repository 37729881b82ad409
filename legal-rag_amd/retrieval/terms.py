"""Required and excluded terms: "articles that contain *seller* and *goods* but not *buyer*".

No reference counterpart: legalrag's BM25 channel only prefers a query's terms and HybridRetriever.search has no filter
argument; a caller who wants a term of art to stand in every hit over-fetches and filters on the host — fewer than top_k
hits, and a fusion normalised over rows the user excluded (the failure retrieval/scope.py describes).  Here a `Terms`
names what a chunk's text must contain, `pack()` turns the (Scope, Terms) pairs of a batch into the operand arrays of
amdr_term_scope (csrc/term_scope.hip), and the GPU resolves them on the resident BM25 postings into the scope table the
scoped channels take: every channel then ranks only the qualifying chunks, with the scores and the order of the unscoped
channels (idf and avgdl stay those of the whole index).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from .scope import Scope

MUST, ANY, NOT = 0, 1, 2  # the group kinds of the ABI (term_scope_rule.hpp TsKind)

Group = Tuple[str, ...]


def _groups(x, field: str) -> Optional[Tuple[Group, ...]]:
    if x is None:
        return None
    if isinstance(x, str):
        x = (x,)
    out: List[Group] = []
    for e in x:
        g = (e,) if isinstance(e, str) else tuple(str(t) for t in e)
        if not g:
            raise ValueError(f"Terms.{field}: an empty group names no token")
        out.append(g)
    return tuple(out) or None


@dataclass(frozen=True)
class Terms:
    """What a chunk's text must contain.  An entry is one vocabulary token (`str`) or a tuple of tokens, one GROUP: a
    chunk satisfies a group when it holds EVERY token of it, anywhere — a conjunction, not a phrase match: the postings
    hold no positions.  For a char-cut Han index a word is the group of its characters, ("合", "同").
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

    def matches(self, tokens) -> bool:
        """The rule on one document's token set (host check; the kernels apply term_scope_rule.hpp)."""
        have = tokens if isinstance(tokens, (set, frozenset, dict)) else set(tokens)
        sat = lambda g: all(t in have for t in g)  # noqa: E731
        return (all(sat(g) for g in self.all_of or ()) and (self.any_of is None or any(sat(g) for g in self.any_of))
                and not any(sat(g) for g in self.none_of or ()))


def driver_length(groups: Sequence[Tuple[int, Sequence[int]]], df: Sequence[int], base_len: Optional[int], n_docs: int) -> int:
    """The candidate count of a constraint by the rule of term_scope_rule.hpp (ts_driver): the shortest of { the base
    scope, the posting list of each MUST term }; 0 with an unknown MUST term; n_docs with neither a MUST term nor a base.
    groups: (kind, term ids); df[t]: the document frequency of term t."""
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


def pack(pairs: Sequence[Tuple[Optional[Scope], Terms]], vocab: Mapping[str, int], doc_freq: Mapping[str, int], n_docs: int,
         base_rows=None) -> TermTable:
    """The operand arrays of a batch of (Scope | None, Terms) pairs.  Equal pairs are stored once (as ScopeResolver.table
    stores equal scopes once) and `qscope` names each pair's constraint; equal base scopes are stored once as well.
    vocab / doc_freq: the live host model's token -> term id and token -> document frequency (BM25Okapi.vocab(),
    _doc_frequencies()); base_rows(scope) -> the ascending int64 rows of a Scope (ScopeResolver.rows), needed only when a
    pair carries one.  The bounds come from the host model by the header's own rule: cand_max = the longest driver,
    rows_cap = the sum of the drivers."""
    df_by_id = np.zeros(len(vocab), dtype=np.int64)
    for w, t in vocab.items():
        df_by_id[t] = doc_freq.get(w, 0)
    slot: Dict[Any, int] = {}
    base_slot: Dict[Scope, int] = {}
    bases: List[np.ndarray] = []
    grp_ptr, grp_kind, grp_term_ptr, grp_terms, cons_base, lens = [0], [], [0], [], [], []
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
            groups = [(kind, [vocab.get(t, -1) for t in g]) for kind, g in terms.groups()]
            for kind, ids in groups:
                grp_kind.append(kind)
                grp_terms.extend(ids)
                grp_term_ptr.append(len(grp_terms))
            grp_ptr.append(len(grp_kind))
            cons_base.append(b)
            lens.append(driver_length(groups, df_by_id, int(bases[b].size) if b >= 0 else None, n_docs))
        qscope[i] = j
    base_ptr = np.zeros(len(bases) + 1, dtype=np.int64)
    if bases:
        np.cumsum([b.size for b in bases], out=base_ptr[1:])
    ops = (np.asarray(grp_ptr, dtype=np.int64), np.asarray(grp_kind, dtype=np.int32), np.asarray(grp_term_ptr, dtype=np.int64),
           np.asarray(grp_terms, dtype=np.int32), base_ptr,
           np.concatenate(bases) if bases else np.zeros(0, dtype=np.int64), np.asarray(cons_base, dtype=np.int32))
    lens_a = np.asarray(lens, dtype=np.int64)
    return TermTable(ops, qscope, len(cons_base), len(grp_kind), len(bases), lens_a,
                     int(lens_a.max()) if lens_a.size else 0, int(lens_a.sum()))

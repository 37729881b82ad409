"""Search scopes: "within Book III", "within this section", "only these articles".

No reference counterpart: legalrag's HybridRetriever.search ranks the whole corpus; a caller who wants a part of it
over-fetches and filters, which returns fewer than top_k hits for a narrow scope and normalises the fusion over rows the
user excluded.  Here a `Scope` names a part of the corpus by the fields every LawChunk carries, a `ScopeResolver` turns
it into the ascending row list of ONE chunk list (dense rows, BM25 documents and ColBERT documents each have their own
list: one resolver per channel's list), and `table()` packs the scopes of a batch into the arrays the scoped kernels
take (csrc/scope.hip): the channels then rank only those rows, with the scores and the order of the unscoped channels.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

_FIELDS = ("law_name", "chapter", "section")
FACET_FIELDS = _FIELDS + ("article_id",)  # the fields ScopeResolver.codes() numbers (retrieval/facets.py)


def _as_set(x) -> Optional[frozenset]:
    if x is None:
        return None
    if isinstance(x, (str, bytes)):
        return frozenset((str(x),))
    return frozenset(str(v) for v in x)


@dataclass(frozen=True)
class Scope:
    """A part of the corpus.  Every given field must match (AND); a field left at None does not restrict.
    law_name / chapter / section: the chunk's field equals the value; article_ids / chunk_ids: the chunk's article_id /
    id is one of the values (any iterable; stored as a frozenset, so equal scopes are equal and hash alike)."""
    law_name: Optional[str] = None
    chapter: Optional[str] = None
    section: Optional[str] = None
    article_ids: Optional[frozenset] = None
    chunk_ids: Optional[frozenset] = None

    def __post_init__(self) -> None:
        object.__setattr__(self, "article_ids", _as_set(self.article_ids))
        object.__setattr__(self, "chunk_ids", _as_set(self.chunk_ids))

    @property
    def unrestricted(self) -> bool:
        return all(getattr(self, f) is None for f in _FIELDS + ("article_ids", "chunk_ids"))


class ScopeResolver:
    """Scope -> the ascending, unique int64 rows of `chunks` it names (cached per scope; the arrays are read-only).
    Built once per chunk list: one index per field, value -> rows."""

    def __init__(self, chunks: Sequence[Any]):
        self.n = len(chunks)
        self._by: Dict[str, Dict[str, List[int]]] = {f: {} for f in _FIELDS + ("article_id", "id")}
        for row, c in enumerate(chunks):
            for f, index in self._by.items():
                v = getattr(c, f, None)
                if v is not None:
                    index.setdefault(str(v), []).append(row)
        self._cache: Dict[Scope, np.ndarray] = {}
        self._codes: Dict[Any, Tuple[np.ndarray, Any]] = {}  # field -> codes(); ("columns", fields...) -> code_columns()

    def codes(self, field: str) -> Tuple[np.ndarray, List[str]]:
        """(codes i32 [n], values) of a facet field (FACET_FIELDS): row r's value is values[codes[r]], -1 where the chunk's
        field is None.  A value's code is its order of first appearance by row, so "code ascending" is "first in the
        statute".  Cached beside the row cache for the resolver's lifetime; the array is read-only."""
        got = self._codes.get(field)
        if got is not None:
            return got
        if field not in FACET_FIELDS:
            raise ValueError(f"codes(): {field!r} is not a facet field (one of {', '.join(FACET_FIELDS)})")
        index = self._by[field]
        firsts = sorted((rows[0], v) for v, rows in index.items())  # (dict order is first appearance already; said outright)
        codes = np.full(self.n, -1, dtype=np.int32)
        values: List[str] = []
        for c, (_, v) in enumerate(firsts):
            codes[np.asarray(index[v], dtype=np.int64)] = c
            values.append(v)
        codes.setflags(write=False)
        got = self._codes[field] = (codes, values)
        return got

    def code_columns(self, fields: Sequence[str]) -> Tuple[np.ndarray, List[List[str]]]:
        """(codes i32 [len(fields), n] field-major, the fields' value lists): the operand of the facet kernel
        (csrc/facet.hip).  One read-only array per tuple of fields, cached with the resolver, so that a device copy made of
        it can be kept as long."""
        key = ("columns",) + tuple(fields)
        got = self._codes.get(key)
        if got is None:
            per = [self.codes(f) for f in fields]
            cols = np.ascontiguousarray(np.stack([c for c, _ in per]), dtype=np.int32).reshape(len(per), self.n)
            cols.setflags(write=False)
            got = self._codes[key] = (cols, [v for _, v in per])
        return got

    def _rows_of(self, field: str, values: Iterable[str]) -> np.ndarray:
        index = self._by[field]
        parts = [index[v] for v in values if v in index]
        if not parts:
            return np.zeros(0, dtype=np.int64)
        return np.unique(np.concatenate([np.asarray(p, dtype=np.int64) for p in parts]))

    def row_of(self, chunk_id: Any) -> int:
        """The (first) row of the chunk with this id, -1 when the list holds none."""
        rows = self._by["id"].get(str(chunk_id))
        return int(rows[0]) if rows else -1

    def rows(self, scope: Scope) -> np.ndarray:
        got = self._cache.get(scope)
        if got is not None:
            return got
        out: Optional[np.ndarray] = None
        for f in _FIELDS:
            v = getattr(scope, f)
            if v is not None:
                r = self._rows_of(f, (str(v),))
                out = r if out is None else np.intersect1d(out, r, assume_unique=True)
        for f, key in (("article_ids", "article_id"), ("chunk_ids", "id")):
            v = getattr(scope, f)
            if v is not None:
                r = self._rows_of(key, v)
                out = r if out is None else np.intersect1d(out, r, assume_unique=True)
        if out is None:  # no field given: the whole list
            out = np.arange(self.n, dtype=np.int64)
        out = np.ascontiguousarray(out, dtype=np.int64)
        out.setflags(write=False)
        self._cache[scope] = out
        return out

    def table(self, scopes: Sequence[Scope]) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
        """(scope_ptr i64 [n_scopes + 1], rows i64, qscope i32 [len(scopes)], rows_max) of a batch: query i ranks rows
        [scope_ptr[qscope[i]], scope_ptr[qscope[i] + 1]); equal scopes of the batch are stored once."""
        slot: Dict[Scope, int] = {}
        parts: List[np.ndarray] = []
        qscope = np.empty(len(scopes), dtype=np.int32)
        for i, s in enumerate(scopes):
            j = slot.get(s)
            if j is None:
                j = slot[s] = len(parts)
                parts.append(self.rows(s))
            qscope[i] = j
        scope_ptr = np.zeros(len(parts) + 1, dtype=np.int64)
        if parts:
            np.cumsum([p.size for p in parts], out=scope_ptr[1:])
        rows = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
        rows_max = max((int(p.size) for p in parts), default=0)
        return scope_ptr, np.ascontiguousarray(rows, dtype=np.int64), qscope, rows_max


_RESOLVERS: Dict[int, Tuple[Any, ScopeResolver]] = {}


def resolver_for(chunks: Sequence[Any]) -> ScopeResolver:
    """The resolver of this chunk list object (one per list, kept while the list lives in a retriever)."""
    ent = _RESOLVERS.get(id(chunks))
    if ent is None or ent[0] is not chunks or ent[1].n != len(chunks):
        if len(_RESOLVERS) > 64:
            _RESOLVERS.clear()
        ent = _RESOLVERS[id(chunks)] = (chunks, ScopeResolver(chunks))
    return ent[1]

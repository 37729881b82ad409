"""Facets: how many chunks a query matches, and how they spread over the statute (csrc/facet.hip; the rule is in
include/amdretrieval.h).

    retriever.count(terms=Terms(all_of=[Prefix("sell")]))                              -> 109
    retriever.facets(terms=Terms(all_of=[Prefix("sell")]), spec=Facets(by=("chapter",), top=5))
        .fields["chapter"].values  -> [("Article 2 – Sales", 61), ("Article 9 – Secured Transactions", 22), ...]

The result set of a query is the scope table the term constraints resolve into on the GPU; its rows are counted there, by
the code columns of the chunk list (ScopeResolver.codes), and only the counts come back.  A field's values are listed by
count descending, then by first appearance in the statute; `missing` counts the matching chunks whose field is None.  The
reference has no such call."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

from .scope import FACET_FIELDS

MAX_TOP = 64  # AMDR_FACET_MAX_TOP


@dataclass(frozen=True)
class Facets:
    by: Tuple[str, ...] = ("chapter",)  # the fields to count by, each one of FACET_FIELDS
    top: int = 10                       # values listed per field, 1 .. 64

    def __post_init__(self) -> None:
        if isinstance(self.by, (str, bytes)) or not isinstance(self.by, (tuple, list)):
            raise TypeError(f"Facets.by must be a tuple of field names, got {self.by!r}")
        by = tuple(self.by)
        if not by:
            raise ValueError("Facets.by names no field")
        for f in by:
            if not isinstance(f, str):
                raise TypeError(f"Facets.by must hold field names, got {f!r}")
            if f not in FACET_FIELDS:
                raise ValueError(f"Facets.by: {f!r} is not a facet field (one of {', '.join(FACET_FIELDS)})")
        if len(set(by)) != len(by):
            raise ValueError(f"Facets.by names a field twice: {by!r}")
        if isinstance(self.top, bool) or not isinstance(self.top, int):
            raise TypeError(f"Facets.top must be an int, got {self.top!r}")
        if not 1 <= self.top <= MAX_TOP:
            raise ValueError(f"Facets.top must be in [1, {MAX_TOP}], got {self.top}")
        object.__setattr__(self, "by", by)


@dataclass(frozen=True)
class FieldCounts:
    values: List[Tuple[str, int]]  # (value, count): count descending, then first appearance; at most `top`
    distinct: int                  # the values with a count > 0, listed or not
    missing: int                   # matching chunks whose field is None


@dataclass(frozen=True)
class FacetCounts:
    total: int                      # matching chunks
    fields: Dict[str, FieldCounts]  # one entry per field of the spec, in its order


def build(spec: Facets, values: Sequence[Sequence[str]], total, missing, distinct, code, count) -> List[FacetCounts]:
    """The kernel's arrays (total [n], missing / distinct [n, F], code / count [n, F, top]) as one FacetCounts per
    constraint."""
    out = []
    for p in range(int(total.shape[0])):
        fields = {}
        for f, name in enumerate(spec.by):
            kept = min(int(distinct[p, f]), spec.top)
            fields[name] = FieldCounts([(values[f][int(code[p, f, j])], int(count[p, f, j])) for j in range(kept)],
                                       int(distinct[p, f]), int(missing[p, f]))
        out.append(FacetCounts(int(total[p]), fields))
    return out

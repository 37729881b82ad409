"""Diversified results: maximal-marginal-relevance (MMR) selection over the fused hits (csrc/mmr.hip; the definition is
in include/amdretrieval.h).

    retriever.search(question, top_k=10, diversity=Diversity(lam=0.7))

Each step picks the hit of the largest  lam * score - (1 - lam) * (largest cosine to a hit already picked), the cosine
taken between the hits' rows of the resident chunk matrix.  lam = 1 is the plain ranking, lam = 0 looks at similarity
alone.  The candidates are the first `pool` hits of the list the call would have returned without it.

cfg.retrieval.diversity_lambda / diversity_pool are the default of a call that passes nothing; diversity=False switches
a configured default off for one call.  The reference has no such stage."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Optional

MAX_POOL = 64  # AMDR_MMR_MAX_POOL: one wave of candidates


@dataclass(frozen=True)
class Diversity:
    lam: float = 0.7  # weight of the relevance, in [0, 1]
    pool: int = 0     # candidates per question, at most 64; 0: min(64, max(3 * top_k, 10))

    def __post_init__(self) -> None:
        if isinstance(self.lam, bool) or not isinstance(self.lam, (int, float)):
            raise TypeError(f"Diversity.lam must be a number, got {self.lam!r}")
        if math.isnan(self.lam) or not 0.0 <= self.lam <= 1.0:
            raise ValueError(f"Diversity.lam must be in [0, 1], got {self.lam!r}")
        if isinstance(self.pool, bool) or not isinstance(self.pool, int):
            raise TypeError(f"Diversity.pool must be an int, got {self.pool!r}")
        if not 0 <= self.pool <= MAX_POOL:
            raise ValueError(f"Diversity.pool must be 0 (automatic) or in [1, {MAX_POOL}], got {self.pool}")
        object.__setattr__(self, "lam", float(self.lam))

    def pool_for(self, top_k: int) -> int:
        """The pool of a call that returns top_k hits; a chosen pool below top_k could not fill the result."""
        top_k = int(top_k)
        if top_k > MAX_POOL:
            raise ValueError(f"diversity: MMR selection ranks at most {MAX_POOL} candidates per question, got top_k={top_k}")
        if self.pool == 0:
            return min(MAX_POOL, max(3 * top_k, 10))
        if self.pool < top_k:
            raise ValueError(f"diversity: pool={self.pool} is smaller than top_k={top_k}")
        return self.pool


def configured(rcfg: Any) -> Optional[Diversity]:
    """The default of cfg.retrieval: Diversity(diversity_lambda, diversity_pool), or None while diversity_lambda is None."""
    lam = getattr(rcfg, "diversity_lambda", None)
    if lam is None:
        return None
    return Diversity(lam=lam, pool=int(getattr(rcfg, "diversity_pool", 0) or 0))


def resolve(diversity: Any, rcfg: Any) -> Optional[Diversity]:
    """What a call's `diversity` argument means: None -> the configured default, False -> off, a Diversity -> itself."""
    if diversity is None:
        return configured(rcfg)
    if diversity is False:
        return None
    if not isinstance(diversity, Diversity):
        raise TypeError(f"diversity must be a Diversity, None or False, got {type(diversity).__name__}")
    return diversity

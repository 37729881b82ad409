"""Take chunks out of every channel of the hybrid (the reference has no removal: a withdrawn article takes the full
rebuild of legalrag/retrieval/builders/faiss_builder.py, bm25_builder.py and colbert_builder.py and a reload of each
retriever).  Each builder removes from its own files under its own lock, and a live retriever of this process takes the
removal in place in HBM: amdr_bm25_remove, amdr_dense_remove, amdr_maxsim_remove."""
from __future__ import annotations

import logging
from typing import Dict, Iterable

from .incremental_bm25_builder import IncrementalBM25Builder
from .incremental_dense_builder import IncrementalDenseBuilder

logger = logging.getLogger(__name__)


def remove_chunk_ids(cfg, chunk_ids: Iterable[str]) -> Dict[str, int]:
    """Remove the chunks with these ids from the BM25, dense and (when cfg.retrieval.enable_colbert) ColBERT indexes;
    returns how many each channel held: {"bm25": n, "dense": n, "colbert": n} (no "colbert" key when it is disabled).
    Ids a channel does not hold are skipped there.  A removal that would empty a channel raises ValueError from that
    channel's builder; BM25 goes first, so on one corpus shared by all channels nothing has been removed by then."""
    ids = [str(i) for i in chunk_ids]
    out = {"bm25": IncrementalBM25Builder(cfg).remove_ids(ids), "dense": IncrementalDenseBuilder(cfg).remove_ids(ids)}
    if bool(getattr(cfg.retrieval, "enable_colbert", False)):
        from .incremental_colbert_builder import IncrementalColBERTBuilder
        out["colbert"] = IncrementalColBERTBuilder(cfg).remove_ids(ids)
    logger.info("[remove] %s", out)
    return out

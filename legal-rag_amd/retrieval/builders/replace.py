"""Exchange chunks under their ids in every channel of the hybrid: an AMENDED article (the reference has no update: its
incremental builders skip a chunk id they have seen, so an amendment takes the full rebuild of
legalrag/retrieval/builders/faiss_builder.py, bm25_builder.py and colbert_builder.py and a reload of each retriever).
Each builder replaces in its own files under its own lock, and a live retriever of this process takes the replacement in
place in HBM: amdr_bm25_replace, amdr_dense_replace, amdr_maxsim_replace.  Every chunk keeps its row, so graph tables,
scope tables and row maps stay valid, and each channel is afterwards what a fresh build of the amended corpus, in its
original order, is."""
from __future__ import annotations

import logging
from typing import Dict

from .incremental_bm25_builder import IncrementalBM25Builder
from .incremental_dense_builder import IncrementalDenseBuilder

logger = logging.getLogger(__name__)


def replace_chunks(cfg, jsonl_path) -> Dict[str, int]:
    """Replace, in the BM25, dense and (when cfg.retrieval.enable_colbert) ColBERT indexes, the chunks whose ids the
    chunks of `jsonl_path` carry; returns how many each channel replaced: {"bm25": n, "dense": n, "colbert": n} (no
    "colbert" key when it is disabled).  Ids a channel does not hold are left alone there: adding is add_jsonl's job.
    BM25 goes first, as in remove_chunk_ids."""
    out = {"bm25": IncrementalBM25Builder(cfg).replace_jsonl(jsonl_path),
           "dense": IncrementalDenseBuilder(cfg).replace_jsonl(jsonl_path)}
    if bool(getattr(cfg.retrieval, "enable_colbert", False)):
        from .incremental_colbert_builder import IncrementalColBERTBuilder
        out["colbert"] = IncrementalColBERTBuilder(cfg).replace_jsonl(jsonl_path)
    logger.info("[replace] %s", out)
    return out

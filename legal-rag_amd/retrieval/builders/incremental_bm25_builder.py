"""Incremental BM25 rebuild (counterpart of
legalrag/retrieval/builders/incremental_bm25_builder.py:19-82).

BM25 statistics are corpus-global, so "incremental" is: chunks of the current
bm25.pkl (none if it is missing or unreadable) + the new ids -> full re-fit ->
atomic replace.  The reference tokenises EVERY chunk with jieba.cut on this path,
English included (build_bm25_index lower-cases English with a regex instead);
the quirk is kept so that a re-built index equals the reference's.

The file written is exactly that.  Afterwards a live BM25Retriever of this index file and device (BM25Retriever.live)
whose loaded state was the replaced file takes the new documents in place — BM25Okapi.add_documents and, for the
resident postings, amdr_bm25_add: one device pass instead of unpickling, to_csr() and a new handle — when the re-fit's
old documents and vocabulary are the live object's (BM25Retriever.append_in_place; an index built with the English regex
rule of build_bm25_index is tokenised differently here, fails that check and reloads: correct, not an error).  The
retriever's lock is held from the question "is the loaded state the file" until the append is done, so that no search
thread reloads the new file in between.  A row-sharded retriever (cfg.retrieval.shard = "rows") always reloads."""
from __future__ import annotations

import contextlib
import logging
from pathlib import Path
from typing import List

from ... import artifacts, text
from ...bm25_model import BM25Okapi
from ...schemas import LawChunk
from ._incremental import incoming_chunks

logger = logging.getLogger(__name__)


class IncrementalBM25Builder:
    def __init__(self, cfg):
        self.cfg = cfg

    def _current_chunks(self) -> List[LawChunk]:
        path = Path(self.cfg.retrieval.bm25_index_file)
        try:
            return artifacts.read_bm25_pickle(path)[1] if path.exists() else []
        except Exception:  # noqa: BLE001 - an unreadable index means start over, as the reference does
            return []

    def add_jsonl(self, jsonl_path) -> int:
        batch = incoming_chunks(jsonl_path, logger, "bm25")
        if not batch:
            return 0
        kept = self._current_chunks()
        fresh = [c for c in batch if c.id not in {k.id for k in kept}]
        if not fresh:
            logger.info("[bm25] no new chunks to add: incoming=%d", len(batch))
            return 0
        corpus = kept + fresh
        mode, dict_file = text.cfg_mode(self.cfg), text.cfg_dict_file(self.cfg)
        text.require_dict(mode, dict_file)
        path = Path(self.cfg.retrieval.bm25_index_file)
        tokens = [text.jieba_cut(c.text, mode, dict_file) for c in corpus]
        refit = BM25Okapi(tokens)
        from ..bm25_retriever import BM25Retriever
        live = BM25Retriever.live(path, int(getattr(self.cfg.retrieval, "device", 0)))
        with live._lock if live is not None else contextlib.nullcontext():
            in_place = live is not None and live.state_is_current()
            artifacts.write_bm25_pickle(path, refit, corpus, tokenizer=text.tokenizer_id(mode))
            if in_place:
                in_place = live.append_in_place(refit, corpus, tokens[len(kept):], text.tokenizer_id(mode))
        logger.info("[bm25] live retriever: %s", "appended in place" if in_place else
                    "none" if live is None else "reloads on its next load()")
        logger.info("[bm25] incremental add done: added=%d total=%d", len(fresh), len(corpus))
        return len(fresh)

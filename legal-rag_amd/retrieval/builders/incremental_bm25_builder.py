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
thread reloads the new file in between.  A row-sharded retriever (cfg.retrieval.shard = "rows") always reloads.

remove_ids takes chunks out again (the reference has no removal at all) — out of THIS channel.  A retriever that runs the
hybrid holds the chunk in its dense and ColBERT channels too: builders/remove.py `remove_chunk_ids(cfg, ids)` calls the
three builders' remove_ids.

replace_jsonl exchanges chunks under their ids — an AMENDED article: add_jsonl skips an id the index holds (and says how
many it skipped).  The chunk keeps its row, so every table that names rows stays valid and ties break as in a fresh
build of the amended corpus; builders/replace.py `replace_chunks(cfg, jsonl_path)` does it for every channel."""
from __future__ import annotations

import contextlib
import logging
from pathlib import Path
from typing import Iterable, List

from ... import artifacts, text
from ...bm25_model import BM25Okapi
from ...schemas import LawChunk
from ._incremental import amended, incoming_chunks

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
        if len(fresh) < len(batch):
            logger.info("[bm25] skipped %d incoming chunks whose id is in the index already; replace_jsonl ingests "
                        "amended chunks", len(batch) - len(fresh))
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

    def remove_ids(self, chunk_ids: Iterable[str]) -> int:
        """Remove the chunks with these ids from the index; returns how many were there.  No reference counterpart: the
        reference's builder only appends, so a corpus that shrinks is re-fitted from scratch there.  The model in the
        current pickle is brought to the re-fit of the surviving documents by BM25Okapi.remove_documents — no text is
        tokenised again: doc_freqs are in the file — and written back with the tokenizer id the file records.  None of the
        ids present: 0; all of them: ValueError (an index keeps a document); the file is untouched in both cases.  A live
        BM25Retriever whose loaded state was the replaced file then takes the removal in place (remove_in_place,
        amdr_bm25_remove), under the same lock discipline as add_jsonl; otherwise, and always when row-sharded, it
        reloads on its next load()."""
        wanted = {str(i) for i in chunk_ids}
        path = Path(self.cfg.retrieval.bm25_index_file)
        if not wanted or not path.exists():
            return 0
        bm25, chunks = artifacts.read_bm25_pickle(path)
        rows = [d for d, c in enumerate(chunks) if c.id in wanted]
        if not rows:
            logger.info("[bm25] none of %d ids is in the index", len(wanted))
            return 0
        if len(rows) >= len(chunks):
            raise ValueError("remove_ids: this would empty the index")
        if bm25.corpus_size != len(chunks):
            raise RuntimeError(f"[BM25] {path}: {bm25.corpus_size} documents but {len(chunks)} chunks")
        tokenizer = bm25.__dict__.get("_tokenizer_id")
        bm25.remove_documents(rows)
        gone = set(rows)
        corpus = [c for d, c in enumerate(chunks) if d not in gone]
        from ..bm25_retriever import BM25Retriever
        live = BM25Retriever.live(path, int(getattr(self.cfg.retrieval, "device", 0)))
        with live._lock if live is not None else contextlib.nullcontext():
            in_place = live is not None and live.state_is_current()
            artifacts.write_bm25_pickle(path, bm25, corpus, tokenizer=tokenizer)
            if in_place:
                in_place = live.remove_in_place(rows, corpus)
        logger.info("[bm25] live retriever: %s", "removed in place" if in_place else
                    "none" if live is None else "reloads on its next load()")
        logger.info("[bm25] incremental remove done: removed=%d total=%d", len(rows), len(corpus))
        return len(rows)

    def replace_jsonl(self, jsonl_path) -> int:
        """Incoming chunks whose id IS in the index replace that chunk at its row; returns how many.  Ids the index does
        not hold are left alone (add_jsonl adds them).  The model in the current pickle is brought to the re-fit of the
        amended corpus, in its original order, by BM25Okapi.replace_documents — only the incoming texts are tokenised,
        with add_jsonl's rule (jieba.cut); the other documents keep the tokens the file holds — and written back with the
        tokenizer id the file records, which must be this configuration's.  A live BM25Retriever whose loaded state was
        the replaced file then takes the replacement in place (replace_in_place, amdr_bm25_replace), under the same lock
        discipline as add_jsonl; otherwise it reloads on its next load()."""
        if getattr(self.cfg.retrieval, "shard", None):
            raise RuntimeError("replacement on a row-sharded index is not supported: rebuild and reload")
        batch = incoming_chunks(jsonl_path, logger, "bm25")
        path = Path(self.cfg.retrieval.bm25_index_file)
        if not batch or not path.exists():
            return 0
        bm25, chunks = artifacts.read_bm25_pickle(path)
        found = amended(batch, [c.id for c in chunks])
        if not found:
            logger.info("[bm25] none of %d incoming ids is in the index", len(batch))
            return 0
        if bm25.corpus_size != len(chunks):
            raise RuntimeError(f"[BM25] {path}: {bm25.corpus_size} documents but {len(chunks)} chunks")
        mode, dict_file = text.cfg_mode(self.cfg), text.cfg_dict_file(self.cfg)
        text.require_dict(mode, dict_file)
        tokenizer = bm25.__dict__.get("_tokenizer_id")
        if tokenizer != text.tokenizer_id(mode):
            raise RuntimeError(f"[BM25] {path} was tokenised by {tokenizer!r}, this configuration tokenises by "
                               f"{text.tokenizer_id(mode)!r}: an amended chunk would be cut differently from the rest. "
                               f"Rebuild the index.")
        rows = list(found)
        tokens = [text.jieba_cut(c.text, mode, dict_file) for c in found.values()]
        bm25.replace_documents(rows, tokens)
        corpus = list(chunks)
        for r, c in found.items():
            corpus[r] = c
        from ..bm25_retriever import BM25Retriever
        live = BM25Retriever.live(path, int(getattr(self.cfg.retrieval, "device", 0)))
        with live._lock if live is not None else contextlib.nullcontext():
            in_place = live is not None and live.state_is_current()
            artifacts.write_bm25_pickle(path, bm25, corpus, tokenizer=tokenizer)
            if in_place:
                in_place = live.replace_in_place(rows, tokens, corpus)
        logger.info("[bm25] live retriever: %s", "replaced in place" if in_place else
                    "none" if live is None else "reloads on its next load()")
        logger.info("[bm25] incremental replace done: replaced=%d total=%d", len(rows), len(corpus))
        return len(rows)

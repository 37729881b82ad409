"""Incremental ColBERT add: the sibling of IncrementalDenseBuilder for the token store (the reference has none — its
only way to index a new document is Indexer.index() over the whole collection,
legalrag/retrieval/builders/colbert_builder.py:131-132).

Under the lock build_colbert_index takes (`<index_path>/.colbert_build.lock`): read colbert_meta.jsonl, keep only ids
it does not hold yet, encode THOSE chunks, append their meta lines (pid = next row) BEFORE the token store is rewritten
(a reader must never see a pid without its chunk), then append the token rows to the store.  Before anything is
written the meta file and the store must agree (pids 0 .. n - 1, n documents); if they do not, it asks for a rebuild.
If a ColBERTRetriever of this index identity is live in the process and holds the store that was appended to, the same
rows go behind its resident store in HBM (`amdr_maxsim_add`) and it remembers the files' mtimes, so it does not reload
what this process wrote — under the retriever's registry lock from the check to the add, so that no search thread
reloads the file in between; any other reader finds the store changed and reloads it.

remove_ids takes chunks out again under the same lock and the same consistency check: the meta file is rewritten with
the pids renumbered 0 .. n - 1, the token store without the documents, and a live retriever that held the store takes
the removal in place (`amdr_maxsim_remove`, ColBERTRetriever.note_removed).

replace_jsonl exchanges chunks under their pids — an amended article, which add_jsonl skips — under the same lock and
check: the meta file is rewritten with the new chunks at their pids, the token store with their new token rows, and a
live retriever that held the store takes the replacement in place (`amdr_maxsim_replace`,
ColBERTRetriever.note_replaced)."""
from __future__ import annotations

import json
import logging
import os
from pathlib import Path
from typing import Iterable

import numpy as np
from filelock import FileLock

from ... import artifacts
from ..colbert_retriever import ColBERTRetriever, _identity, get_token_encoder
from ._incremental import amended, incoming_chunks, unseen

logger = logging.getLogger(__name__)


class IncrementalColBERTBuilder:
    def __init__(self, cfg):
        self.cfg = cfg

    def add_jsonl(self, jsonl_path) -> int:
        rcfg = self.cfg.retrieval
        if not bool(getattr(rcfg, "enable_colbert", False)):
            raise RuntimeError("ColBERT is disabled: set cfg.retrieval.enable_colbert=True")
        if getattr(rcfg, "shard", None):
            raise RuntimeError("incremental add on a row-sharded index is not supported: rebuild and reload")
        batch = incoming_chunks(jsonl_path, logger, "colbert")
        if not batch:
            return 0
        index_path, index_name, model_name, meta_file, experiment, _ = _identity(rcfg)
        meta_file = Path(meta_file)
        out_dir = artifacts.colbert_index_dir(index_path, experiment, index_name)
        if not meta_file.exists() or not ((out_dir / "amdr_tokens.npz").exists() or artifacts.is_plaid_index(out_dir)):
            raise RuntimeError(f"ColBERT index not found ({meta_file}, {out_dir}). Run build_colbert_index() first.")
        with FileLock(str(Path(index_path) / ".colbert_build.lock")):
            by_pid = artifacts.read_colbert_meta(meta_file)
            fresh = unseen(batch, {c.id for c in by_pid.values()})
            logger.info("[colbert] dedup done: incoming=%d added=%d", len(batch), len(fresh))
            if len(fresh) < len(batch):
                logger.info("[colbert] skipped %d incoming chunks whose id is in the index already; replace_jsonl "
                            "ingests amended chunks", len(batch) - len(fresh))
            if not fresh:
                return 0
            # pid == row of the token store: the meta file must hold pids 0 .. n - 1 and the store n documents (an add
            # that died between its two writes leaves ids without token rows, and every later pid would be off by them)
            first = len(by_pid)
            n_store = artifacts.token_store_ndocs(out_dir)
            if sorted(by_pid) != list(range(first)) or n_store != first:
                raise RuntimeError(f"ColBERT index is inconsistent: {meta_file} holds {first} chunks (pids up to "
                                   f"{max(by_pid) if by_pid else -1}), the token store in {out_dir} {n_store} documents. "
                                   f"Rebuild it: build_colbert_index(cfg, chunks, override=True).")
            enc = get_token_encoder(model_name, str(getattr(rcfg, "encoder_backend", "auto")),
                                    int(getattr(rcfg, "colbert_doc_maxlen", 220)),
                                    device=f"cuda:{int(getattr(rcfg, 'device', 0))}")
            mats = [np.asarray(enc.encode_doc((getattr(c, "text", "") or "").strip()), dtype=np.float32) for c in fresh]
            tokens = np.concatenate(mats, axis=0)
            doc_ptr = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
            live = ColBERTRetriever._instances_by_key.get(_identity(rcfg) + ("none",))
            # The retriever's lock is held from the question "is the resident store the one on disk" until the rows are
            # behind it: a search thread that sees the new mtime in between would otherwise reload the file — new rows
            # included — and the add below would put them there a second time.
            with ColBERTRetriever._registry_lock:
                in_place = live is not None and live.store_is_current()
                with meta_file.open("a", encoding="utf-8") as meta:
                    meta.writelines(json.dumps({"pid": first + i, "chunk": c.model_dump()}, ensure_ascii=False) + "\n"
                                    for i, c in enumerate(fresh))
                artifacts.append_token_store(out_dir, tokens, doc_ptr)
                if in_place:
                    live.note_appended(tokens, doc_ptr, first)
        logger.info("[colbert] incremental add done: added=%d jsonl=%s", len(fresh), jsonl_path)
        return len(fresh)

    def remove_ids(self, chunk_ids: Iterable[str]) -> int:
        """Remove the chunks with these ids; returns how many were there.  None of the ids present: 0; all of them:
        ValueError (a store keeps a document); the files are untouched in both cases.  The meta file (pids renumbered
        0 .. n - 1, through a temporary and os.replace) is written BEFORE the token store, as in add_jsonl."""
        rcfg = self.cfg.retrieval
        if not bool(getattr(rcfg, "enable_colbert", False)):
            raise RuntimeError("ColBERT is disabled: set cfg.retrieval.enable_colbert=True")
        if getattr(rcfg, "shard", None):
            raise RuntimeError("removal on a row-sharded index is not supported: rebuild and reload")
        wanted = {str(i) for i in chunk_ids}
        if not wanted:
            return 0
        index_path, index_name, _model, meta_file, experiment, _ = _identity(rcfg)
        meta_file = Path(meta_file)
        out_dir = artifacts.colbert_index_dir(index_path, experiment, index_name)
        if not meta_file.exists() or not ((out_dir / "amdr_tokens.npz").exists() or artifacts.is_plaid_index(out_dir)):
            raise RuntimeError(f"ColBERT index not found ({meta_file}, {out_dir}). Run build_colbert_index() first.")
        with FileLock(str(Path(index_path) / ".colbert_build.lock")):
            by_pid = artifacts.read_colbert_meta(meta_file)
            rows = sorted(pid for pid, c in by_pid.items() if c.id in wanted)
            if not rows:
                logger.info("[colbert] none of %d ids is in the index", len(wanted))
                return 0
            n = len(by_pid)
            n_store = artifacts.token_store_ndocs(out_dir)
            if sorted(by_pid) != list(range(n)) or n_store != n:
                raise RuntimeError(f"ColBERT index is inconsistent: {meta_file} holds {n} chunks (pids up to "
                                   f"{max(by_pid) if by_pid else -1}), the token store in {out_dir} {n_store} documents. "
                                   f"Rebuild it: build_colbert_index(cfg, chunks, override=True).")
            if len(rows) >= n:
                raise ValueError("remove_ids: this would empty the index")
            gone = set(rows)
            kept = [by_pid[pid] for pid in range(n) if pid not in gone]
            live = ColBERTRetriever._instances_by_key.get(_identity(rcfg) + ("none",))
            # the retriever's lock from the question "is the resident store the one on disk" until the documents have
            # left it: see add_jsonl
            with ColBERTRetriever._registry_lock:
                in_place = live is not None and live.store_is_current()
                tmp = meta_file.with_suffix(meta_file.suffix + ".tmp")
                artifacts.write_colbert_meta(tmp, kept)
                os.replace(tmp, meta_file)
                artifacts.remove_from_token_store(out_dir, rows)
                if in_place:
                    live.note_removed(rows)
        logger.info("[colbert] incremental remove done: removed=%d total=%d", len(rows), len(kept))
        return len(rows)

    def replace_jsonl(self, jsonl_path) -> int:
        """Incoming chunks whose id IS in the index replace that chunk at its pid; returns how many.  Ids the index does
        not hold are left alone (add_jsonl adds them).  Only the incoming chunks are encoded.  The meta file (through a
        temporary and os.replace) is written BEFORE the token store, as in add_jsonl."""
        rcfg = self.cfg.retrieval
        if not bool(getattr(rcfg, "enable_colbert", False)):
            raise RuntimeError("ColBERT is disabled: set cfg.retrieval.enable_colbert=True")
        if getattr(rcfg, "shard", None):
            raise RuntimeError("replacement on a row-sharded index is not supported: rebuild and reload")
        batch = incoming_chunks(jsonl_path, logger, "colbert")
        if not batch:
            return 0
        index_path, index_name, model_name, meta_file, experiment, _ = _identity(rcfg)
        meta_file = Path(meta_file)
        out_dir = artifacts.colbert_index_dir(index_path, experiment, index_name)
        if not meta_file.exists() or not ((out_dir / "amdr_tokens.npz").exists() or artifacts.is_plaid_index(out_dir)):
            raise RuntimeError(f"ColBERT index not found ({meta_file}, {out_dir}). Run build_colbert_index() first.")
        with FileLock(str(Path(index_path) / ".colbert_build.lock")):
            by_pid = artifacts.read_colbert_meta(meta_file)
            n = len(by_pid)
            n_store = artifacts.token_store_ndocs(out_dir)
            if sorted(by_pid) != list(range(n)) or n_store != n:
                raise RuntimeError(f"ColBERT index is inconsistent: {meta_file} holds {n} chunks (pids up to "
                                   f"{max(by_pid) if by_pid else -1}), the token store in {out_dir} {n_store} documents. "
                                   f"Rebuild it: build_colbert_index(cfg, chunks, override=True).")
            found = amended(batch, [by_pid[pid].id for pid in range(n)])
            if not found:
                logger.info("[colbert] none of %d incoming ids is in the index", len(batch))
                return 0
            enc = get_token_encoder(model_name, str(getattr(rcfg, "encoder_backend", "auto")),
                                    int(getattr(rcfg, "colbert_doc_maxlen", 220)),
                                    device=f"cuda:{int(getattr(rcfg, 'device', 0))}")
            mats = [np.asarray(enc.encode_doc((getattr(c, "text", "") or "").strip()), dtype=np.float32)
                    for c in found.values()]
            tokens = np.concatenate(mats, axis=0)
            doc_ptr = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
            rows = list(found)
            chunks = [found.get(pid, by_pid[pid]) for pid in range(n)]
            live = ColBERTRetriever._instances_by_key.get(_identity(rcfg) + ("none",))
            # the retriever's lock from the question "is the resident store the one on disk" until the documents are
            # exchanged in it: see add_jsonl
            with ColBERTRetriever._registry_lock:
                in_place = live is not None and live.store_is_current()
                tmp = meta_file.with_suffix(meta_file.suffix + ".tmp")
                artifacts.write_colbert_meta(tmp, chunks)
                os.replace(tmp, meta_file)
                artifacts.replace_in_token_store(out_dir, rows, tokens, doc_ptr)
                if in_place:
                    live.note_replaced(rows, tokens, doc_ptr)
        logger.info("[colbert] incremental replace done: replaced=%d total=%d", len(rows), n)
        return len(rows)

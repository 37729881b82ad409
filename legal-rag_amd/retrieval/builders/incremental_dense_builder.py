"""Incremental dense add (counterpart of
legalrag/retrieval/builders/incremental_dense_builder.py:18-78).

Under the index file lock (`faiss.index` with the suffix replaced by `.lock`,
the reference's name): reload the store, keep only ids it does not hold yet,
embed them as passages, append the rows to the matrix resident in HBM
(`amdr_dense_add` is serialised against concurrent searches inside the library),
append the meta lines BEFORE rewriting the index file (a reader must never see
an index row without its chunk), then persist the index.

remove_ids takes chunks out again (the reference has no removal: a corpus that shrinks takes `index.add` over everything,
faiss_builder.py:91, and the reload of vector_store.py): the rows leave the resident matrix in place (`amdr_dense_remove`)
and both files are rewritten.  builders/remove.py does it for every channel of the hybrid.

replace_jsonl exchanges chunks under their ids — an amended article, which add_jsonl skips: the new embeddings are
written over the chunks' rows of the resident matrix (`amdr_dense_replace`), no row moves, and both files are rewritten.
builders/replace.py does it for every channel."""
from __future__ import annotations

import logging
import os
from pathlib import Path
from typing import Iterable

from filelock import FileLock

from ... import artifacts
from ..vector_store import VectorStore
from ._incremental import amended, incoming_chunks, unseen

logger = logging.getLogger(__name__)


class IncrementalDenseBuilder:
    def __init__(self, cfg):
        self.cfg = cfg
        self.vs = VectorStore.from_config(cfg)

    def add_jsonl(self, jsonl_path) -> int:
        batch = incoming_chunks(jsonl_path, logger, "index")
        if not batch:
            return 0
        vs = self.vs
        with FileLock(str(Path(self.cfg.retrieval.faiss_index_file).with_suffix(".lock"))):
            vs.load()
            fresh = unseen(batch, {c.id for c in vs.chunks})
            logger.info("[index] dedup done: incoming=%d added=%d", len(batch), len(fresh))
            if len(fresh) < len(batch):
                logger.info("[index] skipped %d incoming chunks whose id is in the index already; replace_jsonl ingests "
                            "amended chunks", len(batch) - len(fresh))
            if not fresh:
                return 0
            vs.index.add(vs._embed([c.text for c in fresh]).astype("float32"))
            vs.meta_path.parent.mkdir(parents=True, exist_ok=True)
            with vs.meta_path.open("a", encoding="utf-8") as meta:
                meta.writelines(c.model_dump_json() + "\n" for c in fresh)
            vs.chunks.extend(fresh)
            artifacts.write_faiss_flat_ip(vs.index_path, vs.index.reconstruct_n(0, vs.index.ntotal))
            # what this process just wrote IS the resident state: no mtime-triggered reload
            vs._index_mtime = vs.index_path.stat().st_mtime
            vs._meta_mtime = vs.meta_path.stat().st_mtime
        logger.info("[index] incremental add done: added=%d jsonl=%s", len(fresh), jsonl_path)
        return len(fresh)

    def remove_ids(self, chunk_ids: Iterable[str]) -> int:
        """Remove the chunks with these ids; returns how many were there.  Under the index file lock: reload the store,
        find their rows, take the rows out of the matrix resident in HBM (FlatIPIndex.remove_ids: the survivors close up
        in their old order, faiss's convention), then rewrite the meta file and the index file, each through a temporary
        and os.replace, in add_jsonl's order and with its stamping of the mtimes, so that this process does not reload
        what it wrote.  None of the ids present: 0, all of them: ValueError (an index keeps a chunk); the files are
        untouched in both cases.  Row ids held elsewhere name the old rows: a GraphRetriever of this store finds
        `rows_epoch` changed and binds its row map, norms and device tables again."""
        wanted = {str(i) for i in chunk_ids}
        if not wanted:
            return 0
        vs = self.vs
        with FileLock(str(Path(self.cfg.retrieval.faiss_index_file).with_suffix(".lock"))):
            vs.load()
            rows = [r for r, c in enumerate(vs.chunks) if c.id in wanted]
            if not rows:
                logger.info("[index] none of %d ids is in the index", len(wanted))
                return 0
            if len(rows) >= len(vs.chunks):
                raise ValueError("remove_ids: this would empty the index")
            if vs.index.ntotal != len(vs.chunks):
                raise RuntimeError(f"[index] {vs.index_path}: {vs.index.ntotal} rows but {len(vs.chunks)} chunks")
            vs.index.remove_ids(rows)
            gone = set(rows)
            kept = [c for r, c in enumerate(vs.chunks) if r not in gone]
            tmp = vs.meta_path.with_suffix(vs.meta_path.suffix + ".tmp")
            artifacts.write_faiss_meta(tmp, kept)
            os.replace(tmp, vs.meta_path)
            vs.chunks = kept
            artifacts.write_faiss_flat_ip(vs.index_path, vs.index.reconstruct_n(0, vs.index.ntotal))
            # what this process just wrote IS the resident state: no mtime-triggered reload
            vs._index_mtime = vs.index_path.stat().st_mtime
            vs._meta_mtime = vs.meta_path.stat().st_mtime
        logger.info("[index] incremental remove done: removed=%d total=%d", len(rows), len(kept))
        return len(rows)

    def replace_jsonl(self, jsonl_path) -> int:
        """Incoming chunks whose id IS in the index replace that chunk at its row; returns how many.  Ids the index does
        not hold are left alone (add_jsonl adds them).  Under the index file lock: reload the store, embed the incoming
        texts as passages, write them over their rows of the matrix resident in HBM (FlatIPIndex.replace_rows: no row
        moves), then rewrite the meta file and the index file as remove_ids does: each through a temporary and
        os.replace, the mtimes stamped so that this process does not reload what it wrote.  A GraphRetriever of this
        store finds `rows_epoch` changed and binds its norms and device tables again."""
        batch = incoming_chunks(jsonl_path, logger, "index")
        if not batch:
            return 0
        vs = self.vs
        with FileLock(str(Path(self.cfg.retrieval.faiss_index_file).with_suffix(".lock"))):
            vs.load()
            found = amended(batch, [c.id for c in vs.chunks])
            if not found:
                logger.info("[index] none of %d incoming ids is in the index", len(batch))
                return 0
            if vs.index.ntotal != len(vs.chunks):
                raise RuntimeError(f"[index] {vs.index_path}: {vs.index.ntotal} rows but {len(vs.chunks)} chunks")
            vs.index.replace_rows(list(found), vs._embed([c.text for c in found.values()]).astype("float32"))
            chunks = list(vs.chunks)
            for r, c in found.items():
                chunks[r] = c
            tmp = vs.meta_path.with_suffix(vs.meta_path.suffix + ".tmp")
            artifacts.write_faiss_meta(tmp, chunks)
            os.replace(tmp, vs.meta_path)
            vs.chunks = chunks
            artifacts.write_faiss_flat_ip(vs.index_path, vs.index.reconstruct_n(0, vs.index.ntotal))
            # what this process just wrote IS the resident state: no mtime-triggered reload
            vs._index_mtime = vs.index_path.stat().st_mtime
            vs._meta_mtime = vs.meta_path.stat().st_mtime
        logger.info("[index] incremental replace done: replaced=%d total=%d", len(found), len(chunks))
        return len(found)

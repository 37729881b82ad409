"""Sparse channel (legalrag/retrieval/bm25_retriever.py:19-76).

`load()` unpickles {"bm25", "chunks"} (RuntimeError when the file is missing or
has no "bm25", mtime-guarded reload); `search()` tokenises the query with
jieba.cut WITHOUT lower-casing (:73), scores every document with Okapi BM25 and
returns the first top_k of a stable descending sort — zero-score documents
included, ties in ascending document order (:74-76).  Scoring and ranking run in
the HIP kernel (csrc/bm25.hip), bit-identical to rank_bm25's float64 numpy
expression.

Tokenisation is never silently inexact (text.py): a Han query without a
segmenter raises `text.ZhTokenizerUnavailable` unless cfg.retrieval.zh_tokenizer
= "char" (or "dict", with zh_dict_file) opts in (then `zh_exact` is False and the
hybrid layer stamps it into score_breakdown); `search(..., tokens=)` takes the
caller's own tokens; an index whose recorded tokenizer is "char" or "dict" is
queried in the same mode so that index and query tokens stay consistent — and,
when neither jieba nor a registered segmenter exists, its Han queries are cut by
the native batched tokenisers (host and device) in that mode.

Loaded retrievers are kept in a process-wide weak registry, keyed by resolved index file and device
(`BM25Retriever.live`): IncrementalBM25Builder finds the live retriever of the file it has rewritten there and appends
the new documents behind its resident postings (`append_in_place`, amdr_bm25_add) instead of leaving it to reload the
whole index, and takes removed documents out of them the same way (`remove_in_place`, amdr_bm25_remove).  Not on a
row-sharded index (cfg.retrieval.shard = "rows"): that one reloads as before."""
from __future__ import annotations

import threading
import weakref
from itertools import islice
from pathlib import Path
import logging
from typing import ClassVar, List, Optional, Sequence, Tuple

from .. import artifacts, text
from ..bm25_model import BM25Okapi
from ..config import token_stream_mode
from ..schemas import LawChunk


logger = logging.getLogger(__name__)

STAND_INS = ("char", "dict")  # recorded tokenizer ids of the declared inexact Han segmenters (text.py)


class BM25Retriever:
    # loaded instances by (resolved index file, device); weak: a retriever nobody holds any more is not kept alive
    _live: ClassVar["weakref.WeakValueDictionary"] = weakref.WeakValueDictionary()
    _live_lock: ClassVar[threading.Lock] = threading.Lock()

    def __init__(self, cfg):
        self.cfg = cfg
        rcfg = cfg.retrieval
        self.bm25_path = Path(rcfg.bm25_index_file)
        self.device_index = int(getattr(rcfg, "device", 0))
        self._loaded = False
        self._bm25_mtime: float | None = None
        self.bm25: BM25Okapi | None = None
        self.chunks: List[LawChunk] = []
        self._lock = threading.Lock()
        self._tokens_lock = threading.Lock()          # one thread makes the token stream (ensure_token_stream)
        self.index_tokenizer: Optional[str] = None  # id recorded in bm25.pkl (None: reference-built)
        self._tls = threading.local()                 # per-thread: did the last query use the stand-in?
        self.shard = None                             # sharding.ShardSpec in a row-sharded deployment
        self.appends = 0                              # in-place mutations (appends, removals, replacements) so far: part of the
                                                      # hybrid stage's key

    @staticmethod
    def _live_key(path, device: int) -> tuple:
        return str(Path(path).resolve()), int(device)

    @classmethod
    def live(cls, path, device: int) -> Optional["BM25Retriever"]:
        """The loaded retriever of this index file on this device in the process, if one is alive."""
        with cls._live_lock:
            return cls._live.get(cls._live_key(path, device))

    def load(self) -> None:
        if not self.bm25_path.exists():
            raise RuntimeError(
                f"[BM25] index not found: {self.bm25_path}. "
                f"Run: python build_index.py (or python build_index.py --only-bm25)")
        current_mtime = self.bm25_path.stat().st_mtime
        if self._loaded and self._bm25_mtime == current_mtime:
            return
        with self._lock:
            if self._loaded and self._bm25_mtime == current_mtime:
                return
            bm25, chunks = artifacts.read_bm25_pickle(self.bm25_path)
            from . import sharding
            self.shard = sharding.active_shard(self.cfg.retrieval)  # row-sharded deployment: this rank's block only
            # upload CSR postings now, not on the first query
            bm25.gpu(self.device_index, rows=self.shard.bounds(bm25.corpus_size) if self.shard else None)
            self.bm25 = bm25
            self.chunks = chunks
            self.index_tokenizer = bm25.__dict__.get("_tokenizer_id")
            if self.index_tokenizer in STAND_INS:
                logger.warning("[BM25] %s was built with the %s stand-in tokenizer: results differ "
                               "from a jieba-built index (zh_exact=False)", self.bm25_path,
                               "one-character" if self.index_tokenizer == "char" else "dictionary")
            self._loaded = True
            self._bm25_mtime = current_mtime
            with type(self)._live_lock:
                type(self)._live[self._live_key(self.bm25_path, self.device_index)] = self

    def state_is_current(self) -> bool:
        """The loaded state is the index file on disk, and the index is unsharded — asked by the builder BEFORE it
        replaces the file, under `_lock`, which it keeps until append_in_place has returned: a search thread that sees the
        new mtime in between waits in load() and then finds the state current."""
        try:
            return (self._loaded and self.shard is None and self.bm25 is not None
                    and self.bm25_path.stat().st_mtime == self._bm25_mtime)
        except OSError:
            return False

    def _carry_tokens(self) -> dict:
        """The keyword of the in-place updates under cfg.retrieval.token_stream = "carry": they keep the resident token
        stream current (BM25Okapi.*_documents(carry_tokens=True)) instead of dropping it for ensure_token_stream to
        rebuild.  Nothing under "rebuild": the calls are the ones they were."""
        return {"carry_tokens": True} if token_stream_mode(self.cfg) == "carry" else {}

    def append_in_place(self, refit: BM25Okapi, corpus: Sequence[LawChunk], new_tokens: Sequence[Sequence[str]],
                        tokenizer: Optional[str]) -> bool:
        """IncrementalBM25Builder, after it has replaced a file that was current (state_is_current, the caller holds
        `_lock`) by `refit` over `corpus` = the old chunks + len(new_tokens) new ones: when the re-fit's first n documents
        and first V vocabulary keys are the live object's — the old chunks were tokenised as the live index was; an index
        built with the English regex rule is not — the new documents go behind the live object and its resident postings
        (BM25Okapi.add_documents, amdr_bm25_add), the file's mtime is remembered and True is returned: what this process
        wrote IS the resident state.  Otherwise nothing is touched and the next load() reloads the file.
        The append is a mutation of the native handle (include/amdretrieval.h): device work already enqueued is waited
        for here; searches on the device-resident stage must not be STARTED from other threads while an ingest runs."""
        live = self.bm25
        n, v = live.corpus_size, len(live.idf)
        if (tokenizer != self.index_tokenizer or refit.corpus_size != n + len(new_tokens) or len(corpus) != refit.corpus_size
                or len(self.chunks) != n or refit.doc_freqs[:n] != live.doc_freqs
                or list(islice(refit.idf, v)) != list(live.idf)):
            return False
        stamp = self.bm25_path.stat().st_mtime
        if live.__dict__.get("_gpu") is not None:
            import torch
            if torch.cuda.is_available():
                torch.cuda.synchronize(self.device_index)
        try:
            live.add_documents(new_tokens, **self._carry_tokens())
        except Exception as exc:  # noqa: BLE001 - e.g. no room for the transient second copy: the file is reloaded instead
            logger.warning("[BM25] in-place append failed (%s): %s is reloaded on the next load()", exc, self.bm25_path)
            return False
        self.chunks = list(corpus)
        # the native tokenisers hold the vocabulary table: rebuilt for the grown one on their next use
        self.__dict__.pop("_native_tok", None)
        self.__dict__.pop("_device_tok", None)
        self.appends += 1
        self._bm25_mtime = stamp
        return True

    def remove_in_place(self, rows: Sequence[int], corpus_after: Sequence[LawChunk]) -> bool:
        """IncrementalBM25Builder.remove_ids, after it has replaced a file that was current (state_is_current, the caller
        holds `_lock`) by the same index without the documents at `rows` (positions in the replaced file's chunk list),
        whose chunks are now `corpus_after`: when the live chunks' ids and corpus_size are the replaced file's — the live
        chunks without `rows` are corpus_after, id for id — the documents leave the live object and its resident postings
        (BM25Okapi.remove_documents, amdr_bm25_remove), the file's mtime is remembered and True is returned.  Otherwise,
        or when the removal fails, False: the next load() reloads the file.  A mutation of the native handle, as
        append_in_place: device work already enqueued is waited for here; searches on the device-resident stage must not
        be STARTED from other threads meanwhile."""
        live = self.bm25
        gone = {int(r) for r in rows}
        n = live.corpus_size
        if (not gone or min(gone) < 0 or max(gone) >= n or len(self.chunks) != n or len(corpus_after) != n - len(gone)
                or [c.id for d, c in enumerate(self.chunks) if d not in gone] != [c.id for c in corpus_after]):
            return False
        stamp = self.bm25_path.stat().st_mtime
        if live.__dict__.get("_gpu") is not None:
            import torch
            if torch.cuda.is_available():
                torch.cuda.synchronize(self.device_index)
        try:
            live.remove_documents(sorted(gone), **self._carry_tokens())
        except Exception as exc:  # noqa: BLE001 - e.g. no room for the transient second copy: the file is reloaded instead
            logger.warning("[BM25] in-place removal failed (%s): %s is reloaded on the next load()", exc, self.bm25_path)
            return False
        self.chunks = list(corpus_after)
        # the native tokenisers hold the vocabulary table: rebuilt for the renumbered one on their next use
        self.__dict__.pop("_native_tok", None)
        self.__dict__.pop("_device_tok", None)
        self.appends += 1
        self._bm25_mtime = stamp
        return True

    def replace_in_place(self, rows: Sequence[int], new_tokens: Sequence[Sequence[str]],
                         corpus_after: Sequence[LawChunk]) -> bool:
        """IncrementalBM25Builder.replace_jsonl, after it has replaced a file that was current (state_is_current, the
        caller holds `_lock`) by the same index with the documents at `rows` (positions in the chunk list) re-fitted from
        `new_tokens`, whose chunks are now `corpus_after`: when the live chunks are the replaced file's — as many, and
        id for id corpus_after, a replaced chunk keeps its id — the documents are replaced in the live object and its
        resident postings (BM25Okapi.replace_documents, amdr_bm25_replace), the file's mtime is remembered and True is
        returned.  Otherwise, or when the replacement fails, False: the next load() reloads the file.  A mutation of the
        native handle, as append_in_place: device work already enqueued is waited for here; searches on the
        device-resident stage must not be STARTED from other threads meanwhile."""
        live = self.bm25
        rows = [int(r) for r in rows]
        n = live.corpus_size
        if (not rows or len(rows) != len(new_tokens) or len(set(rows)) != len(rows) or min(rows) < 0 or max(rows) >= n
                or len(self.chunks) != n or len(corpus_after) != n
                or [c.id for c in self.chunks] != [c.id for c in corpus_after]):
            return False
        stamp = self.bm25_path.stat().st_mtime
        if live.__dict__.get("_gpu") is not None:
            import torch
            if torch.cuda.is_available():
                torch.cuda.synchronize(self.device_index)
        try:
            live.replace_documents(rows, new_tokens, **self._carry_tokens())
        except Exception as exc:  # noqa: BLE001 - e.g. no room for the transient second copy: the file is reloaded instead
            logger.warning("[BM25] in-place replacement failed (%s): %s is reloaded on the next load()", exc, self.bm25_path)
            return False
        self.chunks = list(corpus_after)
        # the native tokenisers hold the vocabulary table: rebuilt for the renumbered one on their next use
        self.__dict__.pop("_native_tok", None)
        self.__dict__.pop("_device_tok", None)
        self.appends += 1
        self._bm25_mtime = stamp
        return True

    def gpu_index(self):
        """The _native.BM25Index this retriever scores with (this rank's row block in a sharded deployment)."""
        self.load()
        return self.bm25.gpu(self.device_index, rows=self.shard.bounds(self.bm25.corpus_size) if self.shard else None)

    def vocab_matcher(self):
        """The VocabMatcher (retrieval/vocab_match.py) over the live model's vocabulary, resident on this retriever's
        device: what a Wildcard or a Fuzzy is matched against.  Cached, and made again under the validity rule of
        BM25Okapi.sorted_vocab(): the same vocab() object AND the same length — add_documents extends the vocabulary in
        place, a removal or a replacement makes a new one.  The matcher lays the tokens out by term id.  Two threads that
        both find the cache stale each make a matcher and the later one is kept: a handle is wasted, nothing is wrong."""
        from .vocab_match import VocabMatcher
        self.load()
        v = self.bm25.vocab()
        held = self.__dict__.get("_vocab_matcher")
        if held is None or held[0] is not v or held[1] != len(v) or held[2].device != self.device_index:
            held = self.__dict__["_vocab_matcher"] = (v, len(v), VocabMatcher(v, device=self.device_index))
        return held[2]

    def document_tokens(self, s: str) -> List[str]:
        """A string cut as the index cut its documents (builders/bm25_builder.tokenize_corpus): the English regex rule on
        lower-cased text for an index recorded as "en_regex", else text.jieba_cut in the configured mode — when that is
        the segmenter the index records.  ValueError on an index that records no tokeniser (a reference rank_bm25 pickle),
        caller-made tokens ("pretokenized") or a segmenter this process does not have: the text cannot be cut again as
        the index's documents were, and a phrase needs exactly that."""
        self.load()
        tid = self.index_tokenizer
        if tid == "en_regex":
            return text.tokenize_en(s)
        mode = text.cfg_mode(self.cfg)
        if tid is None or tid != text.tokenizer_id(mode):
            raise ValueError(
                f"[BM25] {self.bm25_path} records "
                + ("no tokenizer (an index built by the reference)" if tid is None else f"the tokenizer {tid!r}")
                + f", this process cuts documents with {text.tokenizer_id(mode)!r}: the chunk texts cannot be cut again as "
                  f"the index's documents were, which a phrase constraint needs (the token order is not in the index). "
                  f"Rebuild the index here, or register the segmenter it was built with.")
        return text.jieba_cut(s, mode, text.cfg_dict_file(self.cfg))

    def ensure_token_stream(self) -> None:
        """The resident token stream of the native index (BM25Index.set_tokens), made on the first phrase constraint and
        again after a live add / remove / replace (the native handle drops it with every update and reports none; under
        cfg.retrieval.token_stream = "carry" the update keeps it and this returns at once): the
        chunk texts cut by document_tokens, each document checked against the model's doc_len and doc_freqs
        (BM25Okapi.token_stream: RuntimeError on a mismatch).  Not on a row shard."""
        self.load()
        if self.shard is not None:
            raise ValueError("phrase constraints do not run on a row-sharded index")
        g = self.gpu_index()
        with self._tokens_lock:
            if g.tokens_info()[0]:
                return
            doc_ptr, tokens = self.bm25.token_stream([self.document_tokens(c.text) for c in self.chunks])
            g.set_tokens(doc_ptr, tokens)

    def ensure_breaks(self) -> None:
        """The resident break flags of the native index (BM25Index.set_breaks; retrieval/units.py is the rule), made on the
        first Within and again after whatever dropped them: set_tokens and every live add / remove / replace, carrying or
        not.  The stream is made resident first (ensure_token_stream).  The flags come from a PER-CHUNK CACHE keyed by the
        chunk's id AND its text — a replaced chunk has another text, so its old entry cannot be reused — and only chunks
        without an entry are cut; entries of chunks that are gone are dropped.  The cached flags are concatenated in chunk
        order, each document's length is checked against the resident stream's doc_ptr (RuntimeError on a mismatch) and
        the flags go up, 1 B per token.  After a live update under cfg.retrieval.token_stream = "carry" the next Within
        therefore costs a cut of the NEW texts, one concatenation and that upload, not a re-cut of the corpus.  Not on a row
        shard (ValueError)."""
        import numpy as np
        from .units import PARAGRAPH, SENTENCE, break_flags
        self.load()
        if self.shard is not None:
            raise ValueError("sentence and paragraph constraints do not run on a row-sharded index")
        self.ensure_token_stream()
        g = self.gpu_index()
        with self._tokens_lock:
            if g.breaks_info()[0]:
                return
            lowered = self.index_tokenizer == "en_regex"
            old = self.__dict__.get("_break_cache", {})
            cache, cut, parts, unmapped = {}, [], [], 0
            for c in self.chunks:
                key = (c.id, c.text)
                ent = cache.get(key) or old.get(key)
                if ent is None:
                    ent = break_flags(c.text, self.document_tokens(c.text), lowered)
                    cut.append(c.id)
                cache[key] = ent
                parts.append(ent[0])
                unmapped += 0 if ent[1] else 1
            self._break_cache = cache
            self.breaks_cut = cut  # the ids of the chunks the last call had to cut
            doc_ptr = g.token_doc_ptr()
            lens = np.diff(doc_ptr)
            if len(parts) != lens.size:
                raise RuntimeError(f"[BM25] {len(parts)} chunks, a token stream of {lens.size} documents")
            for d, (fl, n) in enumerate(zip(parts, lens)):
                if fl.size != int(n):
                    raise RuntimeError(f"[BM25] chunk {self.chunks[d].id!r}: {fl.size} break flags for the {int(n)} tokens of its "
                                       f"resident run (the chunk text and the token stream disagree)")
            flags = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
            g.set_breaks(flags)
            n_docs = int(np.count_nonzero(lens))
            self._units_info = (int(flags.size), n_docs + int(np.count_nonzero(flags & SENTENCE)),
                                n_docs + int(np.count_nonzero(flags & PARAGRAPH)), unmapped)

    def units_info(self):
        """(tokens, sentences, paragraphs, unmapped documents) of the resident break flags (ensure_breaks makes them): a
        document's first token opens a sentence and a paragraph, every flagged token one more; an unmapped document — its
        tokens could not be mapped back to its text — counts as one of each."""
        self.ensure_breaks()
        return self._units_info

    def tokenize_query(self, query: str) -> List[str]:
        """bm25_retriever.py:73 — jieba.cut, not lower-cased.  Mode "char" / "dict" when the index was built
        that way or the config opts in; otherwise a Han query without a segmenter raises."""
        standin = self.index_tokenizer in STAND_INS
        mode = self.index_tokenizer if standin else text.cfg_mode(self.cfg)
        if standin and text.contains_han(query):
            # same stand-in as the index, whatever is installed
            toks = text.han_cut(query, mode, self._han_dict() if mode == "dict" else None)
        else:
            toks = text.jieba_cut(query, mode, text.cfg_dict_file(self.cfg))
        self._tls.exact = not (text.contains_han(query) and (standin or not text.zh_exact()))
        return toks

    def _han_dict(self):
        """The dictionary of cfg.retrieval.zh_dict_file (ValueError without one)."""
        return text.han_dict_for(text.cfg_dict_file(self.cfg))

    def han_mode(self):
        """What the native tokenisers do with a query that holds a Han character (_native.Tokenizer(han=)): "char" or
        the text.HanDict on an index recorded as built that way, when neither a registered segmenter nor jieba exists —
        tokenize_query's own result for such a query; "flag" otherwise (the query takes tokenize_query)."""
        if text._custom_cut is not None or text.HAVE_JIEBA or self.index_tokenizer not in STAND_INS:
            return "flag"
        return "char" if self.index_tokenizer == "char" else self._han_dict()

    def term_ids_batch(self, questions: Sequence[str]):
        """Tokenise + look up a whole batch: (q_terms i32, q_ptr i64 [n+1], exact bool [n]) — the query CSR of
        amdr_bm25_search.  Text without Han characters goes through the native batched tokeniser (one call, GIL
        released: amdr_tokenizer_encode, token for token what text.jieba_cut returns for it); a query holding Han
        characters takes tokenize_query() — unless han_mode() names a stand-in: the native call then cuts it too and
        exact is False for exactly those queries — and so does every query when a registered segmenter is present."""
        import numpy as np
        from .. import _native
        self.load()
        n = len(questions)
        # A registered segmenter sees every query.  With jieba installed — every real deployment of the reference — text
        # without Han characters still takes the native tokeniser (jieba decides it without its dictionary, text.py),
        # EXCEPT a query that holds one of the ASCII entries of jieba's dictionary (text._ASCII_DICT_WORDS: the one place
        # where the dictionary reaches into ASCII text): that query, like a Han one, goes to jieba itself.  The fallback is
        # per query, not per process (round 3 sent every English query through per-query Python once jieba was importable).
        native_ok = text._custom_cut is None
        if native_ok:
            qs = questions  # (None counts as the empty query inside the native call)
            terms, q_ptr, hard = self.native_tokenizer().encode(qs)
            if text.HAVE_JIEBA:
                qs = [q or "" for q in questions]
                joined = "\0".join(qs)
                if any(w in joined for w in text._ASCII_DICT_WORDS):  # rare: find the queries concerned
                    hard = hard | np.fromiter((any(w in q for w in text._ASCII_DICT_WORDS) for q in qs), dtype=bool, count=n)
            # text without Han characters is tokenised exactly whatever the index was built with (tokenize_query's rule:
            # only a Han query on a char-built index, or without jieba, is a stand-in result)
            exact = np.ones(n, dtype=bool)
            if self.han_mode() != "flag":  # a stand-in cut the Han queries natively: those, and only those, are inexact
                exact = self._not_han(questions, _native.utf8_views(questions)[3])
            if not hard.any():
                return terms, q_ptr, exact
        else:
            hard = np.ones(n, dtype=bool)
            terms, q_ptr = np.zeros(0, np.int32), np.zeros(n + 1, np.int64)
            exact = np.ones(n, dtype=bool)
        # the remaining queries one by one, spliced into the CSR
        parts, lens = [], np.diff(q_ptr)
        for i in range(n):
            if hard[i]:
                ids = np.asarray(self.bm25.term_ids(self.tokenize_query(questions[i])), dtype=np.int32)
                exact[i] = self.zh_exact
                lens[i] = len(ids)
                parts.append(ids)
            else:
                parts.append(terms[q_ptr[i]:q_ptr[i + 1]])
        out_ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=out_ptr[1:])
        return (np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)), out_ptr, exact

    def native_tokenizer(self):
        """The batched native tokeniser (_native.Tokenizer) over this index's vocabulary, built once per loaded index."""
        from .. import _native
        han = self.han_mode()
        tok = self.__dict__.get("_native_tok")
        if tok is None or tok[0] is not self.bm25 or tok[2] != han:  # (han: a str, or the cached HanDict itself)
            tok = (self.bm25, _native.Tokenizer(list(self.bm25.vocab().keys()), han=han), han)
            self.__dict__["_native_tok"] = tok
        return tok[1]

    def han_key(self):
        """Hashable identity of han_mode() (part of the hybrid stage's compatibility key)."""
        han = self.han_mode()
        return han if isinstance(han, str) else ("dict", id(han))

    @staticmethod
    def _not_han(questions, maybe_han):
        """bool [n]: True where the query holds no Han character (maybe_han: utf8_views' O(1) pre-test)."""
        import numpy as np
        exact = np.ones(len(questions), dtype=bool)
        idx = np.flatnonzero(maybe_han).tolist()
        if idx:
            search = text._RE_HAN_ANY.search  # (contains_han's test)
            exact[idx] = [search(questions[i] or "") is None for i in idx]
        return exact

    def device_tokenizer(self):
        """The same tokeniser on this retriever's GPU (_native.DeviceTokenizer: a copy of native_tokenizer()'s table)."""
        from .. import _native
        self.load()
        ent = self.__dict__.get("_device_tok")
        host = self.native_tokenizer()
        if ent is None or ent[0] is not host or ent[1] != self.device_index:
            ent = (host, self.device_index, _native.DeviceTokenizer(host, device=self.device_index))
            self.__dict__["_device_tok"] = ent
        return ent[2]

    def device_text_batch(self, questions: Sequence[str]):
        """The batch's UTF-8 views and exactness (_native.utf8_views: ptrs, lens, total bytes, keepalive; then exact
        bool [n]) when the device tokeniser decides EVERY query as term_ids_batch would, else None (the caller takes
        term_ids_batch): no registered segmenter, no Han character (an O(1) test of each string's storage kind first;
        only strings that could hold one are searched) unless han_mode() names a stand-in the device copy cuts them by
        and, when jieba is importable, none of its ASCII dictionary entries — term_ids_batch's routing.  exact is False
        for exactly the queries a stand-in cut (zh_exact)."""
        import numpy as np
        from .. import _native
        if text._custom_cut is not None:
            return None
        ptrs, lens, total, maybe_han, keep = _native.utf8_views(questions)
        exact = np.ones(len(questions), dtype=bool)
        if maybe_han.any():
            exact = self._not_han(questions, maybe_han)
            if not exact.all() and self.han_mode() == "flag":
                return None
        if text.HAVE_JIEBA and any(w in "\0".join(q or "" for q in questions) for w in text._ASCII_DICT_WORDS):
            return None
        return ptrs, lens, total, keep, exact

    @property
    def zh_exact(self) -> bool:
        """False when this thread's last query (or the index itself) went through the
        one-character stand-in instead of jieba."""
        return self.index_tokenizer not in STAND_INS and getattr(self._tls, "exact", True)

    def search(self, query: str, top_k: int, tokens: Optional[Sequence[str]] = None) -> List[Tuple[LawChunk, float]]:
        self.load()
        assert self.bm25 is not None
        if tokens is not None:
            tokens = list(tokens)
            self._tls.exact = True
        else:
            tokens = self.tokenize_query(query)
        k = int(top_k)
        if k <= 0:
            return []
        out: List[Tuple[LawChunk, float]] = []
        n = len(self.chunks)
        # the kernel ranks at most MAX_K per call; deeper requests take the dense score vector
        from .._native import MAX_K
        if k <= MAX_K:
            scores, ids = self.bm25.top_k(tokens, min(k, MAX_K), device=self.device_index, shard=self.shard)
            for s, i in zip(scores.tolist(), ids.tolist()):
                if i < 0:
                    break
                out.append((self.chunks[i], float(s)))
            return out
        if self.shard is not None:
            raise ValueError(f"sharded BM25 search: depth {k} exceeds the kernels' limit of {MAX_K}")
        scores = self.bm25.get_scores(tokens, device=self.device_index)
        idxs = sorted(range(n), key=lambda i: scores[i], reverse=True)[:k]
        return [(self.chunks[i], float(scores[i])) for i in idxs]

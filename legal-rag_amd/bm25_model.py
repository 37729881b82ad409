"""Host-side BM25 index object: vocabulary, statistics and the CSR postings that
are uploaded to the GPU.  Stands where `rank_bm25.BM25Okapi` stands in the
reference (`BM25Retriever.bm25`, bm25_retriever.py:30,63), exposing the same
attribute names (k1, b, epsilon, corpus_size, avgdl, doc_freqs, idf, doc_len,
average_idf) so an index pickled by the reference loads into it and an index
built here unpickles under rank_bm25 (artifacts.py).

Statistics follow rank_bm25 0.2.2 exactly (see oracle/bm25.py for the cited
restatement): vocabulary in first-seen order, idf = log(N-df+0.5)-log(df+0.5)
with negative values floored to epsilon*mean(idf), avgdl = total tokens / N.
Scoring runs on the GPU (csrc/bm25.hip) — there is no host scoring path.
"""
from __future__ import annotations

import math
from itertools import chain, islice
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _native


def shard_csr(term_ptr, post_doc, post_tf, doc_len, lo: int, hi: int):
    """Doc-partitioned postings of the row block [lo, hi): every term keeps the postings of those documents only,
    renumbered to local ids 0 .. hi-lo-1 (ascending per term, as the whole index); the term table — and with it the
    caller's idf vector — keeps its full length, so term ids mean the same on every shard."""
    lo, hi = int(lo), int(hi)
    keep = (post_doc >= lo) & (post_doc < hi)
    cnt = np.zeros(len(term_ptr), dtype=np.int64)
    term_of = np.repeat(np.arange(len(term_ptr) - 1), np.diff(term_ptr))
    np.add.at(cnt, term_of[keep] + 1, 1)
    return (np.cumsum(cnt).astype(np.int64), (post_doc[keep] - lo).astype(np.int32), np.ascontiguousarray(post_tf[keep]),
            np.ascontiguousarray(doc_len[lo:hi]))


def docs_csr(doc_freqs: Sequence[Dict[str, int]], vocab: Dict[str, int]):
    """Term-major CSR (term_ptr [V + 1], post_doc, post_tf) of documents given as {word: tf} dicts, local ids from 0,
    ascending per term — to_csr()'s arrays for these documents, built by numpy (a stable sort by term of the
    document-major postings) without a per-posting interpreter loop."""
    V = len(vocab)
    nnz = sum(map(len, doc_freqs))
    terms = np.fromiter(map(vocab.__getitem__, chain.from_iterable(doc_freqs)), dtype=np.int64, count=nnz)
    tfs = np.fromiter(chain.from_iterable(map(dict.values, doc_freqs)), dtype=np.int32, count=nnz)
    docs = np.repeat(np.arange(len(doc_freqs), dtype=np.int32), np.fromiter(map(len, doc_freqs), dtype=np.int64,
                                                                          count=len(doc_freqs)))
    order = np.argsort(terms, kind="stable")
    term_ptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(terms, minlength=V), out=term_ptr[1:])
    return term_ptr, np.ascontiguousarray(docs[order]), np.ascontiguousarray(tfs[order])


def concat_term_ptr(old_ptr, add_ptr):
    """term_ptr of the concatenated index: both tables are prefix sums over the same term ids, the old one extended by
    its last value over the new terms (csrc/bm25_add_rule.hpp computes the same on the device)."""
    old_ptr, add_ptr = np.asarray(old_ptr, dtype=np.int64), np.asarray(add_ptr, dtype=np.int64)
    return old_ptr[np.minimum(np.arange(len(add_ptr)), len(old_ptr) - 1)] + add_ptr


class BM25Okapi:
    def __init__(self, corpus: Optional[Sequence[Sequence[str]]] = None, tokenizer=None, k1: float = 1.5,
                 b: float = 0.75, epsilon: float = 0.25):
        self.k1 = k1
        self.b = b
        self.epsilon = epsilon
        self.corpus_size = 0
        self.avgdl = 0.0
        self.doc_freqs: List[Dict[str, int]] = []
        self.idf: Dict[str, float] = {}
        self.doc_len: List[int] = []
        self.tokenizer = tokenizer
        self.average_idf = 0.0
        if corpus is not None:
            nd: Dict[str, int] = {}
            total = 0
            for document in corpus:
                self.doc_len.append(len(document))
                total += len(document)
                freqs: Dict[str, int] = {}
                for word in document:
                    freqs[word] = freqs.get(word, 0) + 1
                self.doc_freqs.append(freqs)
                for word in freqs:
                    nd[word] = nd.get(word, 0) + 1
                self.corpus_size += 1
            self.avgdl = total / self.corpus_size
            idf_sum = 0
            negative = []
            for word, freq in nd.items():
                v = math.log(self.corpus_size - freq + 0.5) - math.log(freq + 0.5)
                self.idf[word] = v
                idf_sum += v
                if v < 0:
                    negative.append(word)
            self.average_idf = idf_sum / len(self.idf)
            eps = self.epsilon * self.average_idf
            for word in negative:
                self.idf[word] = eps

    # -- device side --------------------------------------------------------
    def __getstate__(self):
        st = dict(self.__dict__)
        for k in ("_vocab", "_sorted_vocab", "_gpu", "_gpu_device", "_tokenizer_id", "_nd", "_total"):
            st.pop(k, None)
        return st

    def vocab(self) -> Dict[str, int]:
        v = self.__dict__.get("_vocab")
        if v is None:
            v = {w: t for t, w in enumerate(self.idf.keys())}
            self.__dict__["_vocab"] = v
        return v

    def sorted_vocab(self) -> List[str]:
        """The vocabulary's tokens ascending by code point (a Prefix is expanded by bisection over it, retrieval/terms.py
        pack); cached next to the vocabulary, not pickled.  add_documents extends vocab() IN PLACE, so the cache holds
        only while vocab() is the same object AND as long as it was; a remove or a replace makes a new vocabulary."""
        v = self.vocab()
        held = self.__dict__.get("_sorted_vocab")
        if held is None or held[0] is not v or held[1] != len(v):
            held = self.__dict__["_sorted_vocab"] = (v, len(v), sorted(v))
        return held[2]

    def _doc_frequencies(self) -> Dict[str, int]:
        """{word: number of documents holding it} in vocabulary order — __init__'s `nd`, rebuilt once from doc_freqs
        (one pass over the postings) and then kept up to date by add_documents; not pickled."""
        nd = self.__dict__.get("_nd")
        if nd is None:
            nd = dict.fromkeys(self.idf, 0)
            for freqs in self.doc_freqs:
                for word in freqs:
                    nd[word] += 1
            self.__dict__["_nd"] = nd
            self.__dict__["_total"] = sum(self.doc_len)
        return nd

    @staticmethod
    def _carried_tokens(g, corpus: Sequence[Sequence[str]], vocab: Dict[str, int]):
        """The `tokens` operand of a carrying update (BM25Index.add / replace): the new documents' sequences as term ids
        over the NEW vocabulary, in text order — or None when the resident index holds no stream to carry."""
        if not g.tokens_info()[0]:
            return None
        tok_ptr = np.zeros(len(corpus) + 1, dtype=np.int64)
        np.cumsum([len(d) for d in corpus], out=tok_ptr[1:])
        return tok_ptr, np.fromiter((vocab[w] for d in corpus for w in d), dtype=np.int32, count=int(tok_ptr[-1]))

    def add_documents(self, corpus: Sequence[Sequence[str]], carry_tokens: bool = False) -> int:
        """Append tokenised documents; afterwards this object equals BM25Okapi(old corpus + corpus): the idf dict in the
        same key order with the same bits (math.log per term and a sequential sum in vocabulary order, as __init__),
        avgdl, average_idf, doc_len, doc_freqs, corpus_size.  O(V + added tokens) after the one-time document-frequency
        cache.  A resident unsharded index (gpu()) takes the same documents in place (BM25Index.add: the added documents'
        CSR, the new idf vector and avgdl); a row shard is dropped and uploaded again on its next use — the in-place
        append on a row-sharded index is not supported.  The resident token stream is dropped by that, unless
        carry_tokens is true: the resident unsharded index then keeps its stream current (BM25Index.add with the added
        documents' sequences; host work proportional to the added tokens)."""
        corpus = list(corpus)
        if not corpus:
            return 0
        if self.corpus_size == 0:
            raise ValueError("add_documents: fit the index on a corpus first")
        nd = self._doc_frequencies()
        n_terms_old = len(nd)
        total = self.__dict__["_total"]
        added: List[Dict[str, int]] = []
        for document in corpus:
            self.doc_len.append(len(document))
            total += len(document)
            freqs: Dict[str, int] = {}
            for word in document:
                freqs[word] = freqs.get(word, 0) + 1
            added.append(freqs)
            for word in freqs:
                nd[word] = nd.get(word, 0) + 1
        self.doc_freqs.extend(added)
        self.corpus_size += len(corpus)
        self.__dict__["_total"] = total
        self.avgdl = total / self.corpus_size
        idf: Dict[str, float] = {}
        idf_sum = 0
        negative = []
        for word, freq in nd.items():
            v = math.log(self.corpus_size - freq + 0.5) - math.log(freq + 0.5)
            idf[word] = v
            idf_sum += v
            if v < 0:
                negative.append(word)
        self.average_idf = idf_sum / len(idf)
        eps = self.epsilon * self.average_idf
        for word in negative:
            idf[word] = eps
        self.idf = idf
        vocab = self.__dict__.get("_vocab")
        if vocab is not None and len(vocab) == n_terms_old:  # new terms take the ids behind the old ones
            for word in islice(nd, n_terms_old, None):
                vocab[word] = len(vocab)
        else:
            self.__dict__.pop("_vocab", None)
        g = self.__dict__.get("_gpu")
        if g is not None:
            if self.__dict__.get("_gpu_device", (None, None))[1] is None:
                term_ptr, post_doc, post_tf = docs_csr(added, self.vocab())
                try:
                    carried = {"tokens": self._carried_tokens(g, corpus, self.vocab())} if carry_tokens else {}
                    g.add(term_ptr, post_doc, post_tf, np.fromiter(idf.values(), dtype=np.float64, count=len(idf)),
                          np.asarray(self.doc_len[-len(corpus):], dtype=np.int32), float(self.avgdl), **carried)
                except Exception:  # the resident index is unchanged and now behind this object: upload again on next use
                    self.__dict__.pop("_gpu", None)
                    self.__dict__.pop("_gpu_device", None)
                    raise
            else:
                self.__dict__.pop("_gpu", None)
                self.__dict__.pop("_gpu_device", None)
        return len(corpus)

    def remove_documents(self, doc_ids: Sequence[int], carry_tokens: bool = False) -> int:
        """Remove documents by id (duplicates and order do not matter); afterwards this object equals
        BM25Okapi(the surviving documents' tokens), the survivors renumbered 0 .. n-1 in their old order: the idf dict in
        the re-fit's key order — the first-seen order of the SURVIVORS, which drops the terms whose documents are all gone
        and can order the rest differently — with the same bits (math.log per term and a sequential sum in that order, as
        __init__), avgdl, average_idf, doc_len, doc_freqs, corpus_size.  O(V + the survivors' postings, at C speed) after
        the one-time document-frequency cache.  ValueError for an id out of range and for removing every document; the
        object is unchanged then.  A resident unsharded index (gpu()) takes the removal in place (BM25Index.remove: the
        ids, the map old term id -> new term id, the new idf vector and avgdl); a row shard is dropped and uploaded
        again on its next use.  The resident token stream is dropped by that, unless carry_tokens is true: the resident
        unsharded index then keeps the survivors' part of its stream (BM25Index.remove with carry=True).  Returns the
        number of documents removed."""
        ids = sorted({int(i) for i in doc_ids})
        if not ids:
            return 0
        if ids[0] < 0 or ids[-1] >= self.corpus_size:
            raise ValueError(f"remove_documents: ids must lie in [0, {self.corpus_size})")
        if len(ids) >= self.corpus_size:
            raise ValueError("remove_documents: an index keeps at least one document")
        nd_old = self._doc_frequencies()
        total = self.__dict__["_total"]
        gone = set(ids)
        doc_freqs = [f for d, f in enumerate(self.doc_freqs) if d not in gone]
        doc_len = [n for d, n in enumerate(self.doc_len) if d not in gone]
        lost: Dict[str, int] = {}
        for d in ids:
            total -= self.doc_len[d]
            for word in self.doc_freqs[d]:
                lost[word] = lost.get(word, 0) + 1
        # the re-fit's vocabulary order: a word's place is its first appearance in the surviving documents
        nd = dict.fromkeys(chain.from_iterable(doc_freqs))
        for word in nd:
            nd[word] = nd_old[word] - lost.get(word, 0)
        corpus_size = len(doc_freqs)
        idf: Dict[str, float] = {}
        idf_sum = 0
        negative = []
        for word, freq in nd.items():
            v = math.log(corpus_size - freq + 0.5) - math.log(freq + 0.5)
            idf[word] = v
            idf_sum += v
            if v < 0:
                negative.append(word)
        average_idf = idf_sum / len(idf)
        eps = self.epsilon * average_idf
        for word in negative:
            idf[word] = eps
        g = self.__dict__.get("_gpu")
        in_place = g is not None and self.__dict__.get("_gpu_device", (None, None))[1] is None
        if in_place:  # old term id -> new term id, -1 for a term that is gone
            old_vocab = self.vocab()
            term_map = np.full(len(old_vocab), -1, dtype=np.int32)
            term_map[np.fromiter(map(old_vocab.__getitem__, nd), dtype=np.int64, count=len(nd))] = np.arange(len(nd), dtype=np.int32)
        self.doc_freqs, self.doc_len, self.corpus_size = doc_freqs, doc_len, corpus_size
        self.avgdl = total / corpus_size
        self.idf, self.average_idf = idf, average_idf
        self.__dict__["_nd"], self.__dict__["_total"] = nd, total
        self.__dict__.pop("_vocab", None)
        if in_place:
            try:
                g.remove(np.asarray(ids, dtype=np.int64), np.fromiter(idf.values(), dtype=np.float64, count=len(idf)),
                         float(self.avgdl), term_map=term_map, **({"carry": True} if carry_tokens else {}))
            except Exception:  # the resident index is unchanged and now ahead of this object: upload again on next use
                self.__dict__.pop("_gpu", None)
                self.__dict__.pop("_gpu_device", None)
                raise
        elif g is not None:
            self.__dict__.pop("_gpu", None)
            self.__dict__.pop("_gpu_device", None)
        return len(ids)

    def replace_documents(self, doc_ids: Sequence[int], corpus: Sequence[Sequence[str]], carry_tokens: bool = False) -> int:
        """Replace documents under their ids: document doc_ids[i] takes the tokens corpus[i] (any order; an id given twice
        is a ValueError) and no document moves.  Afterwards this object equals BM25Okapi(the edited corpus in its original
        order): the idf dict in the re-fit's key order — the first-seen order of the EDITED corpus, which drops a term
        whose last document lost it, takes in new terms where they first appear and moves a word whose first appearance
        moved — with the same bits (math.log per term and a sequential sum in that order, as __init__), avgdl,
        average_idf, doc_len, doc_freqs.  O(V + the postings, at C speed) after the one-time document-frequency cache.
        ValueError for an id out of range or a length mismatch; the object is unchanged then.  A resident unsharded index
        (gpu()) takes the replacement in place (BM25Index.replace: the ids, the new documents' CSR over the new term
        table, the map old term id -> new term id, the new idf vector and avgdl); a row shard is dropped and uploaded
        again on its next use.  The resident token stream is dropped by that, unless carry_tokens is true: the resident
        unsharded index then keeps its stream current (BM25Index.replace with the new documents' sequences).  Returns the
        number of documents replaced."""
        corpus = list(corpus)
        ids = [int(i) for i in doc_ids]
        if len(ids) != len(corpus):
            raise ValueError(f"replace_documents: {len(ids)} ids for {len(corpus)} documents")
        if not ids:
            return 0
        order = sorted(range(len(ids)), key=ids.__getitem__)
        ids = [ids[i] for i in order]
        corpus = [corpus[i] for i in order]
        if ids[0] < 0 or ids[-1] >= self.corpus_size:
            raise ValueError(f"replace_documents: ids must lie in [0, {self.corpus_size})")
        if any(a == b for a, b in zip(ids, ids[1:])):
            raise ValueError("replace_documents: an id is given twice")
        nd_old = self._doc_frequencies()
        total = self.__dict__["_total"]
        change: Dict[str, int] = {}  # document frequency: lost by the old documents, gained by the new ones
        added: List[Dict[str, int]] = []
        for d, document in zip(ids, corpus):
            total += len(document) - self.doc_len[d]
            for word in self.doc_freqs[d]:
                change[word] = change.get(word, 0) - 1
            freqs: Dict[str, int] = {}
            for word in document:
                freqs[word] = freqs.get(word, 0) + 1
            added.append(freqs)
            for word in freqs:
                change[word] = change.get(word, 0) + 1
        doc_freqs = list(self.doc_freqs)
        doc_len = list(self.doc_len)
        for d, document, freqs in zip(ids, corpus, added):
            doc_freqs[d] = freqs
            doc_len[d] = len(document)
        # the re-fit's vocabulary order: a word's place is its first appearance in the edited corpus
        nd = dict.fromkeys(chain.from_iterable(doc_freqs))
        for word in nd:
            nd[word] = nd_old.get(word, 0) + change.get(word, 0)
        corpus_size = self.corpus_size
        idf: Dict[str, float] = {}
        idf_sum = 0
        negative = []
        for word, freq in nd.items():
            v = math.log(corpus_size - freq + 0.5) - math.log(freq + 0.5)
            idf[word] = v
            idf_sum += v
            if v < 0:
                negative.append(word)
        average_idf = idf_sum / len(idf)
        eps = self.epsilon * average_idf
        for word in negative:
            idf[word] = eps
        g = self.__dict__.get("_gpu")
        in_place = g is not None and self.__dict__.get("_gpu_device", (None, None))[1] is None
        if in_place:  # old term id -> new term id, -1 for a term that is gone; the new documents over the new term table
            new_vocab = {w: t for t, w in enumerate(nd)}
            term_map = np.fromiter((new_vocab.get(w, -1) for w in self.vocab()), dtype=np.int32, count=len(self.vocab()))
            add_csr = docs_csr(added, new_vocab)
        self.doc_freqs, self.doc_len = doc_freqs, doc_len
        self.avgdl = total / corpus_size
        self.idf, self.average_idf = idf, average_idf
        self.__dict__["_nd"], self.__dict__["_total"] = nd, total
        self.__dict__.pop("_vocab", None)
        if in_place:
            self.__dict__["_vocab"] = new_vocab
            try:
                carried = {"tokens": self._carried_tokens(g, corpus, new_vocab)} if carry_tokens else {}
                g.replace(np.asarray(ids, dtype=np.int64), *add_csr, np.asarray([doc_len[d] for d in ids], dtype=np.int32),
                          np.fromiter(idf.values(), dtype=np.float64, count=len(idf)), float(self.avgdl), term_map=term_map,
                          **carried)
            except Exception:  # the resident index is unchanged and now behind this object: upload again on next use
                self.__dict__.pop("_gpu", None)
                self.__dict__.pop("_gpu_device", None)
                raise
        elif g is not None:
            self.__dict__.pop("_gpu", None)
            self.__dict__.pop("_gpu_device", None)
        return len(ids)

    def to_csr(self):
        vocab = self.vocab()
        V = len(vocab)
        counts = np.zeros(V + 1, dtype=np.int64)
        for doc in self.doc_freqs:
            for w in doc:
                counts[vocab[w] + 1] += 1
        term_ptr = np.cumsum(counts).astype(np.int64)
        fill = term_ptr[:-1].copy()
        nnz = int(term_ptr[-1])
        post_doc = np.empty(nnz, dtype=np.int32)
        post_tf = np.empty(nnz, dtype=np.int32)
        for d, doc in enumerate(self.doc_freqs):
            for w, tf in doc.items():
                t = vocab[w]
                post_doc[fill[t]] = d
                post_tf[fill[t]] = tf
                fill[t] += 1
        idf = np.fromiter((self.idf[w] for w in vocab), dtype=np.float64, count=V)
        return term_ptr, post_doc, post_tf, idf, np.asarray(self.doc_len, dtype=np.int32)

    def gpu(self, device: int = 0, rows: Optional[tuple] = None) -> "_native.BM25Index":
        """The postings in HBM.  rows = (lo, hi): only the documents of that block (doc-partitioned postings at
        local ids 0 .. hi-lo-1) with the corpus-GLOBAL idf and avgdl — a row shard of a multi-GPU deployment
        (retrieval/sharding.py); per-document scores are then bit-identical to the unsharded index's."""
        key = (device, tuple(rows) if rows is not None else None)
        g = self.__dict__.get("_gpu")
        if g is None or self.__dict__.get("_gpu_device") != key:
            term_ptr, post_doc, post_tf, idf, doc_len = self.to_csr()
            if rows is not None:
                term_ptr, post_doc, post_tf, doc_len = shard_csr(term_ptr, post_doc, post_tf, doc_len, *rows)
            g = _native.BM25Index(term_ptr, post_doc, post_tf, idf, doc_len, float(self.avgdl), float(self.k1),
                                  float(self.b), device=device)
            self.__dict__["_gpu"] = g
            self.__dict__["_gpu_device"] = key
        return g

    def token_stream(self, docs: Sequence[Sequence[str]]):
        """(doc_ptr i64 [n + 1], tokens i32) of the corpus given as one token SEQUENCE per document, in text order — the
        operands of BM25Index.set_tokens (the forward index phrase constraints read).  The index keeps counts, not order,
        so the sequences come from the caller, cut again from the texts; each is checked against what the index holds of
        its document: as many tokens as doc_len says and the term counts of doc_freqs.  RuntimeError names the first
        document that differs (texts or a tokeniser that are not the index's)."""
        if len(docs) != self.corpus_size:
            raise RuntimeError(f"token_stream: {len(docs)} documents for an index of {self.corpus_size}")
        vocab = self.vocab()
        doc_ptr = np.zeros(len(docs) + 1, dtype=np.int64)
        np.cumsum([len(d) for d in docs], out=doc_ptr[1:])
        tokens = np.empty(int(doc_ptr[-1]), dtype=np.int32)
        for d, doc in enumerate(docs):
            if len(doc) != self.doc_len[d]:
                raise RuntimeError(f"token_stream: document {d} has {len(doc)} tokens, the index holds {self.doc_len[d]}")
            freqs: Dict[str, int] = {}
            for word in doc:
                freqs[word] = freqs.get(word, 0) + 1
            if freqs != self.doc_freqs[d]:
                raise RuntimeError(f"token_stream: the tokens of document {d} are not the ones the index counted")
            tokens[doc_ptr[d]:doc_ptr[d + 1]] = [vocab[w] for w in doc]
        return doc_ptr, tokens

    def term_ids(self, tokens: Sequence[str]) -> List[int]:
        v = self.vocab()
        return [v.get(t, -1) for t in tokens]

    def get_scores(self, query: Sequence[str], device: int = 0) -> np.ndarray:
        """Same contract as rank_bm25's get_scores, computed by the HIP kernel."""
        return self.gpu(device).get_scores([self.term_ids(query)])[0]

    def top_k(self, query: Sequence[str], k: int, device: int = 0, shard=None):
        """(scores, doc ids) of the k best documents.  shard = sharding.ShardSpec: this rank scores its row block,
        the per-shard lists are all-gathered and merged; ids are global and identical on every rank."""
        if shard is None:
            s, i = self.gpu(device).search([self.term_ids(query)], k)
            return s[0], i[0]
        from .retrieval import sharding
        lo, hi = shard.bounds(self.corpus_size)
        s, i = self.gpu(device, rows=(lo, hi)).search([self.term_ids(query)], k)
        (gs, gi), = sharding.exchange_topk_numpy([(s, i)], lo, device, group=shard.group)
        return gs[0], gi[0]

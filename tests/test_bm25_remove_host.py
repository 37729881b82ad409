"""Host side of the BM25 removal (no GPU): BM25Okapi.remove_documents against a re-fit of the survivors, bit for bit in
every statistic and in to_csr(); what remove_documents sends to a resident index; and IncrementalBM25Builder.remove_ids'
decision between the in-place removal and the reload, with _native.BM25Index stubbed."""
import json
import random
import struct

import numpy as np
import pytest

from conftest import GOLDEN
from legal_rag_amd import bm25_model
from legal_rag_amd.bm25_model import BM25Okapi

WORDS = [f"w{i}" for i in range(300)]


def corpus(rng, n, extra=None):
    """n documents over a Zipfian vocabulary; "all" is in every document (its idf takes the epsilon floor), lengths
    from 1 token up; extra(i) -> further tokens of document i."""
    out = []
    for i in range(n):
        doc = ["all"] + [WORDS[min(int(rng.paretovariate(1.1)) - 1, 299)] for _ in range(rng.choice([0, 1, 4, 16, 39, 89]))]
        out.append(doc + list(extra(i) if extra else ()))
    return out


def bits(x):
    return struct.pack("<d", x)


def assert_equals_refit(a, docs):
    b = BM25Okapi(docs)
    assert list(a.idf) == list(b.idf)  # key order
    assert [bits(x) for x in a.idf.values()] == [bits(x) for x in b.idf.values()]
    assert bits(a.avgdl) == bits(b.avgdl) and bits(a.average_idf) == bits(b.average_idf)
    assert a.doc_len == b.doc_len and a.doc_freqs == b.doc_freqs and a.corpus_size == b.corpus_size
    assert [list(f) for f in a.doc_freqs] == [list(f) for f in b.doc_freqs]
    assert a.vocab() == b.vocab() and list(a.vocab()) == list(b.vocab())
    for x, y in zip(a.to_csr(), b.to_csr()):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    return b


def survivors(docs, ids):
    gone = set(ids)
    return [d for i, d in enumerate(docs) if i not in gone]


@pytest.fixture(scope="module")
def docs1500():
    # "rare<j>" lives in documents 10j .. 10j+2 only; "early" words come first in the low documents, so that removing
    # those moves their first appearance behind words that used to follow them
    return corpus(random.Random(1500), 1500, extra=lambda i: ([f"rare{i // 10}"] if i % 10 < 3 and i < 600 else []))


@pytest.mark.parametrize("n_remove", [1, 37, 600])
def test_remove_documents_equals_a_refit(docs1500, n_remove):
    ids = random.Random(n_remove).sample(range(1500), n_remove)
    a = BM25Okapi(docs1500)
    if n_remove == 37:
        a.vocab()  # a vocabulary table made before the removal is not kept
    assert a.remove_documents(ids + ids[:1]) == n_remove  # a duplicate, unsorted
    b = assert_equals_refit(a, survivors(docs1500, ids))
    floor = b.epsilon * b.average_idf
    assert bits(a.idf["all"]) == bits(floor) and floor > 0  # df = N still: log(0.5) - log(N + 0.5) < 0 -> the floor


@pytest.mark.parametrize("ids", [[0], [1499], [0, 1499]], ids=["first", "last", "both"])
def test_first_and_last_document(docs1500, ids):
    a = BM25Okapi(docs1500)
    assert a.remove_documents(ids) == len(ids)
    assert_equals_refit(a, survivors(docs1500, ids))


def term_map_of(old, new):
    ov = old.vocab()
    tm = np.full(len(ov), -1, dtype=np.int32)
    for w, t in new.vocab().items():
        tm[ov[w]] = t
    return tm


def test_dropped_terms_and_a_changed_first_seen_order(docs1500):
    ids = list(range(0, 120))  # rare0 .. rare11 disappear; the words first seen in documents 0 .. 119 move back
    old = BM25Okapi(docs1500)
    a = BM25Okapi(docs1500)
    a.remove_documents(ids)
    b = assert_equals_refit(a, survivors(docs1500, ids))
    assert "rare0" in old.idf and "rare11" in old.idf and "rare0" not in a.idf and "rare11" not in a.idf and "rare12" in a.idf
    tm = term_map_of(old, b)
    assert (tm == -1).sum() == len(old.idf) - len(b.idf) >= 12
    kept = tm[tm >= 0]
    assert sorted(kept.tolist()) == list(range(len(b.idf)))
    assert not np.all(np.diff(kept) > 0), "the map old term id -> new term id is monotone: the case shows nothing"


def test_add_then_remove_and_remove_then_add():
    rng = random.Random(11)
    base, more = corpus(rng, 400, extra=lambda i: [f"b{i % 9}"]), corpus(rng, 60, extra=lambda i: ["fresh", f"m{i}"])
    a = BM25Okapi(base)
    a.add_documents(more)
    ids = [3, 17, 399, 400, 401, 459]
    a.remove_documents(ids)
    assert_equals_refit(a, survivors(base + more, ids))
    c = BM25Okapi(base)
    c.remove_documents([0, 5, 6, 7, 399])
    c.add_documents(more)
    assert_equals_refit(c, survivors(base, [0, 5, 6, 7, 399]) + more)
    assert set(c.__getstate__()) == set(BM25Okapi(base).__getstate__())  # the caches are still not pickled


def test_value_errors_leave_the_object_unchanged(docs1500):
    a = BM25Okapi(docs1500[:50])
    for bad in ([50], [-1], [0, 49, 50], list(range(50))):
        with pytest.raises(ValueError):
            a.remove_documents(bad)
    assert a.remove_documents([]) == 0
    assert_equals_refit(a, docs1500[:50])


class StubIndex:
    """Stands where _native.BM25Index stands: keeps what it is given."""
    made = []

    def __init__(self, term_ptr, post_doc, post_tf, idf, doc_len, avgdl, k1=1.5, b=0.75, *, device=0):
        self.n_docs, self.n_terms, self.device, self.adds, self.removes = len(doc_len), len(term_ptr) - 1, device, [], []
        StubIndex.made.append(self)

    def add(self, term_ptr_add, post_doc_add, post_tf_add, idf, doc_len_add, avgdl):
        self.adds.append((term_ptr_add, post_doc_add, post_tf_add, idf, doc_len_add, avgdl))
        self.n_docs += len(doc_len_add)
        self.n_terms = len(term_ptr_add) - 1

    def remove(self, remove_ids, idf, avgdl, term_map=None):
        self.removes.append((remove_ids, idf, avgdl, term_map))
        self.n_docs -= len(remove_ids)
        self.n_terms = len(idf)


@pytest.fixture()
def stub(monkeypatch):
    StubIndex.made = []
    monkeypatch.setattr(bm25_model._native, "BM25Index", StubIndex)
    return StubIndex


def test_a_resident_index_takes_the_removal(stub, docs1500):
    docs = docs1500[:300]
    ids = [299, 0, 1, 2, 57, 57]
    old = BM25Okapi(docs)
    a = BM25Okapi(docs)
    g = a.gpu(0)
    assert a.remove_documents(ids) == 5
    assert a.gpu(0) is g and len(stub.made) == 1 and len(g.removes) == 1
    remove_ids, idf, avgdl, term_map = g.removes[0]
    whole = BM25Okapi(survivors(docs, ids))
    assert remove_ids.dtype == np.int64 and remove_ids.tolist() == [0, 1, 2, 57, 299]
    assert term_map.dtype == np.int32 and np.array_equal(term_map, term_map_of(old, whole))
    assert idf.tobytes() == whole.to_csr()[3].tobytes() and bits(avgdl) == bits(whole.avgdl)
    # a row shard is not removed from: it is dropped and uploaded again on its next use
    b = BM25Okapi(docs)
    s = b.gpu(0, rows=(0, 150))
    b.remove_documents(ids)
    assert s.removes == [] and "_gpu" not in b.__dict__
    assert_equals_refit(b, survivors(docs, ids))


def _cfg(root):
    from legal_rag_amd.config import AppConfig
    return AppConfig.for_data_dir(str(root), "en")


def _jsonl(path, chunks):
    path.write_text("".join(json.dumps(c.model_dump(), ensure_ascii=False) + "\n" for c in chunks), encoding="utf-8")
    return path


@pytest.fixture(scope="module")
def chunks():
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    return load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")[:50]


def _same_model(a, b):
    assert list(a.idf) == list(b.idf) and [bits(x) for x in a.idf.values()] == [bits(x) for x in b.idf.values()]
    assert a.doc_freqs == b.doc_freqs and a.doc_len == b.doc_len and bits(a.avgdl) == bits(b.avgdl)
    assert bits(a.average_idf) == bits(b.average_idf) and a.corpus_size == b.corpus_size


def test_builder_removes_in_place(stub, tmp_path, chunks):
    from legal_rag_amd import artifacts, text
    from legal_rag_amd.retrieval.bm25_retriever import BM25Retriever
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    cfg = _cfg(tmp_path)
    assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "a.jsonl", chunks[:40])) == 40
    recorded = artifacts.read_bm25_pickle(cfg.retrieval.bm25_index_file)[0].__dict__["_tokenizer_id"]
    r = BM25Retriever(cfg)
    r.load()
    live, g = r.bm25, r.bm25.gpu(0)
    gone = [chunks[0].id, chunks[7].id, chunks[39].id, "no-such-id"]
    assert IncrementalBM25Builder(cfg).remove_ids(gone) == 3
    r.load()
    assert r.bm25 is live and r.bm25.gpu(0) is g and len(g.removes) == 1 and r.appends == 1 and len(stub.made) == 1
    assert g.removes[0][0].tolist() == [0, 7, 39] and g.n_docs == 37
    left = [c for c in chunks[:40] if c.id not in set(gone)]
    assert [c.id for c in r.chunks] == [c.id for c in left]
    # the file on disk equals the live object, and both the re-fit of the surviving texts; the tokenizer id is kept
    on_disk, disk_chunks = artifacts.read_bm25_pickle(cfg.retrieval.bm25_index_file)
    assert [c.id for c in disk_chunks] == [c.id for c in r.chunks]
    assert on_disk.__dict__["_tokenizer_id"] == recorded
    _same_model(live, on_disk)
    mode = text.cfg_mode(cfg)
    _same_model(live, BM25Okapi([text.jieba_cut(c.text, mode, text.cfg_dict_file(cfg)) for c in left]))
    # a replace: remove + add, both in place
    assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "b.jsonl", [chunks[7]] + chunks[40:45])) == 6
    r.load()
    assert r.bm25 is live and len(g.adds) == 1 and r.appends == 2 and g.n_docs == 43 and len(stub.made) == 1
    assert IncrementalBM25Builder(cfg).remove_ids([chunks[44].id]) == 1
    r.load()
    assert r.bm25 is live and len(g.removes) == 2 and r.appends == 3 and g.n_docs == 42 and len(stub.made) == 1
    _same_model(live, artifacts.read_bm25_pickle(cfg.retrieval.bm25_index_file)[0])


def test_builder_leaves_a_file_changed_underneath_to_reload(stub, tmp_path, chunks):
    import os
    from legal_rag_amd.retrieval.bm25_retriever import BM25Retriever
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    cfg = _cfg(tmp_path)
    IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "a.jsonl", chunks[:30]))
    r = BM25Retriever(cfg)
    r.load()
    live, g = r.bm25, r.bm25.gpu(0)
    st = os.stat(cfg.retrieval.bm25_index_file)
    os.utime(cfg.retrieval.bm25_index_file, ns=(st.st_atime_ns, st.st_mtime_ns + 10_000_000_000))  # another writer
    assert not r.state_is_current()
    assert IncrementalBM25Builder(cfg).remove_ids([chunks[3].id, chunks[4].id]) == 2
    assert g.removes == [] and r.appends == 0 and r.bm25 is live and live.corpus_size == 30
    r.load()
    assert r.bm25 is not live and r.bm25.corpus_size == 28 and len(r.chunks) == 28 and len(stub.made) == 2


def test_builder_with_nothing_to_remove_or_everything(stub, tmp_path, chunks):
    from legal_rag_amd.retrieval.bm25_retriever import BM25Retriever
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    cfg = _cfg(tmp_path)
    assert IncrementalBM25Builder(cfg).remove_ids(["x"]) == 0  # no index file yet
    IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "a.jsonl", chunks[:10]))
    r = BM25Retriever(cfg)
    r.load()
    g = r.bm25.gpu(0)
    before = (open(cfg.retrieval.bm25_index_file, "rb").read(), r._bm25_mtime)
    assert IncrementalBM25Builder(cfg).remove_ids(["no-such-id"]) == 0
    assert IncrementalBM25Builder(cfg).remove_ids([]) == 0
    with pytest.raises(ValueError):
        IncrementalBM25Builder(cfg).remove_ids([c.id for c in chunks[:10]])
    import os
    assert (open(cfg.retrieval.bm25_index_file, "rb").read(), os.stat(cfg.retrieval.bm25_index_file).st_mtime) == before
    assert g.removes == [] and r.appends == 0 and r.state_is_current()

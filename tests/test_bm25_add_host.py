"""Host side of the BM25 append (no GPU): BM25Okapi.add_documents against a re-fit, bit for bit in every statistic; the
numpy CSR of the added documents and the elementwise term_ptr identity against to_csr() of the re-fit; what
add_documents sends to a resident index; and IncrementalBM25Builder's decision between the in-place append and the
reload, with _native.BM25Index stubbed."""
import json
import random
import struct

import numpy as np
import pytest

from conftest import GOLDEN
from legal_rag_amd import bm25_model
from legal_rag_amd.bm25_model import BM25Okapi, concat_term_ptr, docs_csr, shard_csr

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
    assert a.vocab() == b.vocab() and list(a.vocab()) == list(b.vocab())
    for x, y in zip(a.to_csr(), b.to_csr()):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    return b


@pytest.mark.parametrize("n_add", [1, 37, 600])
def test_add_documents_equals_a_refit(n_add):
    rng = random.Random(n_add)
    old = corpus(rng, 1500)
    new = corpus(rng, n_add, extra=lambda i: [f"new{i % 16}"] + (["once"] if i == 0 else []))
    if n_add > 1:
        new[-1] = ["all"]  # a document of one token
    a = BM25Okapi(old)
    if n_add == 37:
        a.vocab()  # a vocabulary table made before the add is extended, not rebuilt
    assert a.add_documents(new) == n_add
    b = assert_equals_refit(a, old + new)
    floor = b.epsilon * b.average_idf
    assert bits(a.idf["all"]) == bits(floor) and floor > 0  # df = N: log(0.5) - log(N + 0.5) < 0 -> the floor
    assert "once" in a.idf and list(a.idf).index("new0") >= len(BM25Okapi(old).idf)


def test_two_adds_in_a_row_and_the_pickled_state():
    rng = random.Random(5)
    parts = [corpus(rng, 200), corpus(rng, 8, extra=lambda i: ["x"]), corpus(rng, 37, extra=lambda i: ["x", f"y{i}"])]
    a = BM25Okapi(parts[0])
    a.add_documents(parts[1])
    a.add_documents(parts[2])
    assert a.add_documents([]) == 0
    assert_equals_refit(a, parts[0] + parts[1] + parts[2])
    assert set(a.__getstate__()) == set(BM25Okapi(parts[0]).__getstate__())  # the caches are not pickled
    with pytest.raises(ValueError):
        BM25Okapi().add_documents([["a"]])


def test_numpy_csr_and_term_ptr_identity():
    rng = random.Random(9)
    old, new = corpus(rng, 700), corpus(rng, 90, extra=lambda i: [f"n{i % 7}"] * (1 + i % 3))
    whole = BM25Okapi(old + new)
    term_ptr, post_doc, post_tf, _, doc_len = whole.to_csr()
    for x, y in zip(docs_csr(whole.doc_freqs, whole.vocab()), (term_ptr, post_doc, post_tf)):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    add = docs_csr(whole.doc_freqs[700:], whole.vocab())
    exp = shard_csr(term_ptr, post_doc, post_tf, doc_len, 700, 790)  # the re-fit's postings of the added documents
    for x, y in zip(add, exp[:3]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    old_ptr = BM25Okapi(old).to_csr()[0]
    assert len(old_ptr) < len(term_ptr)  # new terms
    assert np.array_equal(concat_term_ptr(old_ptr, add[0]), term_ptr)
    assert np.array_equal(old_ptr[np.minimum(np.arange(len(term_ptr)), len(old_ptr) - 1)] + add[0], term_ptr)


class StubIndex:
    """Stands where _native.BM25Index stands: keeps what it is given."""
    made = []

    def __init__(self, term_ptr, post_doc, post_tf, idf, doc_len, avgdl, k1=1.5, b=0.75, *, device=0):
        self.n_docs, self.n_terms, self.device, self.adds = len(doc_len), len(term_ptr) - 1, device, []
        StubIndex.made.append(self)

    def add(self, term_ptr_add, post_doc_add, post_tf_add, idf, doc_len_add, avgdl):
        self.adds.append((term_ptr_add, post_doc_add, post_tf_add, idf, doc_len_add, avgdl))
        self.n_docs += len(doc_len_add)
        self.n_terms = len(term_ptr_add) - 1


@pytest.fixture()
def stub(monkeypatch):
    StubIndex.made = []
    monkeypatch.setattr(bm25_model._native, "BM25Index", StubIndex)
    return StubIndex


def test_a_resident_index_takes_the_added_documents(stub):
    rng = random.Random(3)
    old, new = corpus(rng, 300), corpus(rng, 30, extra=lambda i: ["fresh"])
    a = BM25Okapi(old)
    g = a.gpu(0)
    a.add_documents(new)
    assert a.gpu(0) is g and len(stub.made) == 1 and len(g.adds) == 1
    term_ptr_add, post_doc_add, post_tf_add, idf, doc_len_add, avgdl = g.adds[0]
    whole = BM25Okapi(old + new)
    term_ptr, post_doc, post_tf, idf_w, doc_len = whole.to_csr()
    exp = shard_csr(term_ptr, post_doc, post_tf, doc_len, 300, 330)
    assert np.array_equal(term_ptr_add, exp[0]) and np.array_equal(post_doc_add, exp[1]) and np.array_equal(post_tf_add, exp[2])
    assert idf.tobytes() == idf_w.tobytes() and np.array_equal(doc_len_add, exp[3]) and bits(avgdl) == bits(whole.avgdl)
    # a row shard is not appended to: it is dropped and uploaded again on its next use
    b = BM25Okapi(old)
    s = b.gpu(0, rows=(0, 150))
    b.add_documents(new)
    assert s.adds == [] and "_gpu" not in b.__dict__


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


def test_builder_appends_in_place_when_the_old_tokens_agree(stub, tmp_path, chunks):
    from legal_rag_amd import artifacts
    from legal_rag_amd.retrieval.bm25_retriever import BM25Retriever
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    cfg = _cfg(tmp_path)
    assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "a.jsonl", chunks[:30])) == 30
    r = BM25Retriever(cfg)
    r.load()
    assert BM25Retriever.live(cfg.retrieval.bm25_index_file, 0) is r
    live, g = r.bm25, r.bm25.gpu(0)
    r.bm25.vocab()
    assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "b.jsonl", chunks[25:42])) == 12  # 5 ids are there already
    r.load()
    assert r.bm25 is live and r.bm25.gpu(0) is g and len(g.adds) == 1 and r.appends == 1 and len(stub.made) == 1
    assert [c.id for c in r.chunks] == [c.id for c in chunks[:42]] and g.n_docs == 42
    on_disk, disk_chunks = artifacts.read_bm25_pickle(cfg.retrieval.bm25_index_file)
    assert [c.id for c in disk_chunks] == [c.id for c in r.chunks]
    assert list(live.idf) == list(on_disk.idf) and [bits(x) for x in live.idf.values()] == [bits(x) for x in on_disk.idf.values()]
    assert live.doc_freqs == on_disk.doc_freqs and bits(live.avgdl) == bits(on_disk.avgdl)
    # and once more: two appends in a row
    assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "c.jsonl", chunks[42:50])) == 8
    r.load()
    assert r.bm25 is live and len(g.adds) == 2 and r.appends == 2 and g.n_docs == 50 and len(stub.made) == 1


def test_builder_leaves_a_regex_built_index_to_reload(stub, tmp_path, chunks):
    from legal_rag_amd.retrieval.bm25_retriever import BM25Retriever
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    cfg = _cfg(tmp_path)
    build_bm25_index(cfg, chunks[:30])  # English through the lower-casing regex: other tokens than the incremental path's
    r = BM25Retriever(cfg)
    r.load()
    live, g = r.bm25, r.bm25.gpu(0)
    assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "b.jsonl", chunks[30:42])) == 12
    assert g.adds == [] and r.bm25 is live and r.appends == 0  # untouched ...
    r.load()                                                   # ... and reloaded on the next load()
    assert r.bm25 is not live and r.bm25.corpus_size == 42 and len(r.chunks) == 42 and len(stub.made) == 2


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
    assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "b.jsonl", chunks[30:42])) == 12
    assert g.adds == [] and r.appends == 0
    r.load()
    assert r.bm25 is not live and r.bm25.corpus_size == 42

"""Host side of the BM25 replacement (no GPU): BM25Okapi.replace_documents against a re-fit of the edited corpus in its
original order, bit for bit in every statistic and in to_csr(); what replace_documents sends to a resident index; and
IncrementalBM25Builder.replace_jsonl's decision between the in-place replacement and the reload, with _native.BM25Index
stubbed."""
import json
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN
from legal_rag_amd import bm25_model
from legal_rag_amd.bm25_model import BM25Okapi, docs_csr
from test_bm25_remove_host import StubIndex, _cfg, _jsonl, _same_model, assert_equals_refit, bits, corpus


def term_map_of(old, new):
    """old term id -> new term id, -1 for a term that is gone (a new term has no old id)."""
    nv = new.vocab()
    return np.asarray([nv.get(w, -1) for w in old.vocab()], dtype=np.int32)


def edited(docs, ids, new):
    out = list(docs)
    for i, d in zip(ids, new):
        out[i] = d
    return out


@pytest.fixture(scope="module")
def docs1500():
    # "rare<j>" lives in documents 10j .. 10j+2 only; "solo<i>" in document i alone, for i < 40; the words first seen in
    # the low documents move back when those documents lose them
    return corpus(random.Random(1500), 1500, extra=lambda i: ([f"rare{i // 10}"] if i % 10 < 3 and i < 600 else []) +
                  ([f"solo{i}"] if i < 40 else []))


@pytest.mark.parametrize("n_rep", [1, 37, 1500])
def test_replace_documents_equals_a_refit(docs1500, n_rep):
    rng = random.Random(n_rep)
    ids = rng.sample(range(1500), n_rep)
    new = corpus(rng, n_rep, extra=lambda i: [f"new{i % 5}"] if i % 3 == 0 else [])
    a = BM25Okapi(docs1500)
    if n_rep == 37:
        a.vocab()  # a vocabulary table made before the replacement is not kept
    assert a.replace_documents(ids, new) == n_rep  # unsorted ids
    b = assert_equals_refit(a, edited(docs1500, ids, new))
    floor = b.epsilon * b.average_idf
    assert bits(a.idf["all"]) == bits(floor) and floor > 0  # df = N still: the floor
    assert a.corpus_size == 1500


@pytest.mark.parametrize("ids", [[0], [1499], [1499, 0]], ids=["first", "last", "both"])
def test_first_and_last_document(docs1500, ids):
    new = [["all", "brand", "new", "new"], ["one"]][:len(ids)]
    a = BM25Okapi(docs1500)
    assert a.replace_documents(ids, new) == len(ids)
    assert_equals_refit(a, edited(docs1500, ids, new))


def test_a_dropped_term_a_new_term_and_a_moved_first_appearance(docs1500):
    old = BM25Okapi(docs1500)
    # document 5 alone holds "solo5": replacing it drops the term; the replacement brings a word nobody had
    a = BM25Okapi(docs1500)
    a.replace_documents([5], [["all", "never-seen-before"]])
    b = assert_equals_refit(a, edited(docs1500, [5], [["all", "never-seen-before"]]))
    assert "solo5" in old.idf and "solo5" not in a.idf and "never-seen-before" in a.idf
    assert list(a.idf).index("never-seen-before") < len(a.idf) - 1, "the new term is not behind the old ones: null map is not enough"
    tm = term_map_of(old, b)
    assert (tm == -1).sum() >= 1 and len(b.idf) - (tm >= 0).sum() == 1
    # documents 0 .. 119 become one-word documents: the words first seen there move behind words that used to follow them
    ids = list(range(120))
    new = [["all"]] * 120
    c = BM25Okapi(docs1500)
    c.replace_documents(ids, new)
    d = assert_equals_refit(c, edited(docs1500, ids, new))
    kept = term_map_of(old, d)
    kept = kept[kept >= 0]
    assert not np.all(np.diff(kept) > 0), "the map old term id -> new term id is monotone: the case shows nothing"
    assert "rare0" not in c.idf and "rare12" in c.idf


def test_a_replacement_equal_to_the_original_changes_nothing(docs1500):
    import pickle
    a = BM25Okapi(docs1500)
    before = pickle.dumps(a)
    csr = [x.tobytes() for x in a.to_csr()]
    ids = [0, 7, 700, 1499]
    assert a.replace_documents(ids, [docs1500[i] for i in ids]) == 4
    assert pickle.dumps(a) == before
    assert [x.tobytes() for x in a.to_csr()] == csr
    assert_equals_refit(a, docs1500)


def test_replace_after_add_and_remove():
    rng = random.Random(12)
    base, more = corpus(rng, 400, extra=lambda i: [f"b{i % 9}"]), corpus(rng, 60, extra=lambda i: ["fresh", f"m{i}"])
    new = corpus(rng, 5, extra=lambda i: [f"n{i}"])
    a = BM25Okapi(base)
    a.add_documents(more)
    ids = [3, 399, 400, 459, 17]
    a.replace_documents(ids, new)
    docs = edited(base + more, ids, new)
    assert_equals_refit(a, docs)
    a.remove_documents([0, 400])
    docs = [d for i, d in enumerate(docs) if i not in (0, 400)]
    a.replace_documents([0, 457], new[:2])
    assert_equals_refit(a, edited(docs, [0, 457], new[:2]))
    assert set(a.__getstate__()) == set(BM25Okapi(base).__getstate__())  # the caches are still not pickled


def test_value_errors_leave_the_object_unchanged(docs1500):
    a = BM25Okapi(docs1500[:50])
    for ids, new in (([50], [["x"]]), ([-1], [["x"]]), ([0, 0], [["x"], ["y"]]), ([0, 1], [["x"]])):
        with pytest.raises(ValueError):
            a.replace_documents(ids, new)
    assert a.replace_documents([], []) == 0
    assert_equals_refit(a, docs1500[:50])


class ReplaceStub(StubIndex):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.replaced = []

    def replace(self, replace_ids, term_ptr_add, post_doc_add, post_tf_add, doc_len_add, idf, avgdl, term_map=None):
        self.replaced.append((replace_ids, term_ptr_add, post_doc_add, post_tf_add, doc_len_add, idf, avgdl, term_map))
        self.n_terms = len(idf)


@pytest.fixture()
def stub(monkeypatch):
    StubIndex.made = []
    monkeypatch.setattr(bm25_model._native, "BM25Index", ReplaceStub)
    return StubIndex


def test_a_resident_index_takes_the_replacement(stub, docs1500):
    docs = docs1500[:300]
    ids = [299, 5, 0, 57]
    new = [["all", "zz-new", "zz-new"], ["all"], ["w0", "zz-new"], ["all", "w1", "w1", "w2"]]
    old = BM25Okapi(docs)
    a = BM25Okapi(docs)
    g = a.gpu(0)
    assert a.replace_documents(ids, new) == 4
    assert a.gpu(0) is g and len(stub.made) == 1 and len(g.replaced) == 1
    replace_ids, tp, pd, pt, dl, idf, avgdl, term_map = g.replaced[0]
    whole = BM25Okapi(edited(docs, ids, new))
    assert replace_ids.dtype == np.int64 and replace_ids.tolist() == [0, 5, 57, 299]
    by_id = dict(zip(ids, new))
    ordered = [by_id[i] for i in (0, 5, 57, 299)]
    want = docs_csr([BM25Okapi([d]).doc_freqs[0] for d in ordered], whole.vocab())
    for x, y in zip((tp, pd, pt), want):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert dl.dtype == np.int32 and dl.tolist() == [len(d) for d in ordered]
    assert term_map.dtype == np.int32 and np.array_equal(term_map, term_map_of(old, whole))
    assert (term_map == -1).sum() >= 1  # "solo5" is gone
    assert idf.tobytes() == whole.to_csr()[3].tobytes() and bits(avgdl) == bits(whole.avgdl)
    assert a.vocab() == whole.vocab()
    # a row shard is not replaced in: it is dropped and uploaded again on its next use
    b = BM25Okapi(docs)
    s = b.gpu(0, rows=(0, 150))
    b.replace_documents(ids, new)
    assert s.replaced == [] and "_gpu" not in b.__dict__
    assert_equals_refit(b, edited(docs, ids, new))


@pytest.fixture(scope="module")
def chunks():
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    return load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")[:50]


def amend(chunk, text):
    return chunk.model_copy(update={"text": text})


def test_builder_replaces_in_place(stub, tmp_path, chunks, caplog):
    import logging
    from legal_rag_amd import artifacts, text
    from legal_rag_amd.retrieval.bm25_retriever import BM25Retriever
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    cfg = _cfg(tmp_path)
    assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "a.jsonl", chunks[:40])) == 40
    recorded = artifacts.read_bm25_pickle(cfg.retrieval.bm25_index_file)[0].__dict__["_tokenizer_id"]
    r = BM25Retriever(cfg)
    r.load()
    live, g = r.bm25, r.bm25.gpu(0)
    new = [amend(chunks[39], "The last article, amended: entirely new wording."),
           amend(chunks[0], chunks[0].text + " An amendment adds this sentence."),
           amend(chunks[45], "not in the index: left alone"),
           amend(chunks[7], "superseded by the next line"), amend(chunks[7], "Article seven as amended twice.")]
    path = _jsonl(tmp_path / "b.jsonl", new)
    # add_jsonl still adds nothing for known ids, and now says so
    with caplog.at_level(logging.INFO):
        assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "c.jsonl", new[:2])) == 0
    assert "skipped 2 incoming chunks" in caplog.text and "replace_jsonl" in caplog.text
    assert IncrementalBM25Builder(cfg).replace_jsonl(path) == 3
    r.load()
    assert r.bm25 is live and r.bm25.gpu(0) is g and len(g.replaced) == 1 and r.appends == 1 and len(stub.made) == 1
    assert g.replaced[0][0].tolist() == [0, 7, 39] and g.n_docs == 40
    after = list(chunks[:40])
    after[0], after[7], after[39] = new[1], new[4], new[0]
    assert [c.id for c in r.chunks] == [c.id for c in chunks[:40]] and [c.text for c in r.chunks] == [c.text for c in after]
    on_disk, disk_chunks = artifacts.read_bm25_pickle(cfg.retrieval.bm25_index_file)
    assert [c.text for c in disk_chunks] == [c.text for c in after]
    assert on_disk.__dict__["_tokenizer_id"] == recorded
    _same_model(live, on_disk)
    mode = text.cfg_mode(cfg)
    _same_model(live, BM25Okapi([text.jieba_cut(c.text, mode, text.cfg_dict_file(cfg)) for c in after]))
    # nothing to replace: the file stays
    before = open(cfg.retrieval.bm25_index_file, "rb").read()
    assert IncrementalBM25Builder(cfg).replace_jsonl(_jsonl(tmp_path / "d.jsonl", [chunks[45]])) == 0
    assert open(cfg.retrieval.bm25_index_file, "rb").read() == before and len(g.replaced) == 1


def test_builder_leaves_a_file_changed_underneath_to_reload(stub, tmp_path, chunks):
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
    assert IncrementalBM25Builder(cfg).replace_jsonl(_jsonl(tmp_path / "b.jsonl", [amend(chunks[3], "amended")])) == 1
    assert g.replaced == [] and r.appends == 0 and r.bm25 is live
    r.load()
    assert r.bm25 is not live and r.chunks[3].text == "amended" and len(r.chunks) == 30 and len(stub.made) == 2


def test_builder_without_an_index_and_row_sharded(stub, tmp_path, chunks):
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    cfg = _cfg(tmp_path)
    path = _jsonl(tmp_path / "b.jsonl", [chunks[0]])
    assert IncrementalBM25Builder(cfg).replace_jsonl(path) == 0  # no index file yet
    cfg.retrieval.shard = "rows"
    with pytest.raises(RuntimeError, match="replacement on a row-sharded index is not supported: rebuild and reload"):
        IncrementalBM25Builder(cfg).replace_jsonl(path)

"""IncrementalColBERTBuilder and artifacts.append_token_store on the host: ids are de-duplicated against
colbert_meta.jsonl, only the new chunks are encoded, the meta lines and the token store end up as a build over the
whole list writes them.  No retriever is live and the native library is never asked for (no GPU)."""
import json

import numpy as np
import pytest

from conftest import GOLDEN
from legal_rag_amd import _native, artifacts
from legal_rag_amd.config import AppConfig
from legal_rag_amd.retrieval import colbert_retriever
from legal_rag_amd.retrieval.builders.colbert_builder import build_colbert_index
from legal_rag_amd.retrieval.builders.incremental_colbert_builder import IncrementalColBERTBuilder
from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir


@pytest.fixture(autouse=True)
def no_native(monkeypatch):
    def refuse():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(_native, "load", refuse)


@pytest.fixture(scope="module")
def chunks():
    return load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")[:40]


def _cfg(root):
    cfg = AppConfig.for_data_dir(str(root), "en")
    cfg.retrieval.encoder_backend = "hashing"
    cfg.retrieval.enable_colbert = True
    return cfg


def _jsonl(path, chunks):
    path.write_text("".join(json.dumps(c.model_dump(), ensure_ascii=False) + "\n" for c in chunks), encoding="utf-8")
    return path


def _index_dir(cfg):
    r = cfg.retrieval
    return artifacts.colbert_index_dir(str(r.colbert_index_path), str(r.colbert_experiment), str(r.colbert_index_name))


def test_add_equals_a_build_of_the_whole_list(tmp_path, chunks, monkeypatch):
    cfg = _cfg(tmp_path / "grown")
    build_colbert_index(cfg, chunks[:30])
    # count what the add encodes: a wrapper around the encoder both builders obtain
    enc = colbert_retriever.get_token_encoder(cfg.retrieval.colbert_model_name, "hashing",
                                              int(cfg.retrieval.colbert_doc_maxlen), device="cuda:0")
    seen = []
    real = enc.encode_doc
    monkeypatch.setattr(enc, "encode_doc", lambda text: (seen.append(text), real(text))[1], raising=False)
    inc = _jsonl(tmp_path / "incoming.jsonl", chunks[25:40])  # 5 ids are there already
    assert IncrementalColBERTBuilder(cfg).add_jsonl(inc) == 10
    assert seen == [c.text.strip() for c in chunks[30:40]]  # only the new documents were encoded

    whole = _cfg(tmp_path / "whole")
    build_colbert_index(whole, chunks[:40])
    D, ptr = artifacts.read_token_store(_index_dir(cfg))
    De, ptre = artifacts.read_token_store(_index_dir(whole))
    assert D.dtype == np.float32 and ptr.dtype == np.int64
    assert np.array_equal(ptr, ptre) and np.array_equal(D, De)
    meta = artifacts.read_colbert_meta(cfg.retrieval.colbert_meta_file)
    assert list(meta) == list(range(40)) and [meta[i].id for i in range(40)] == [c.id for c in chunks]
    lines = [json.loads(x) for x in open(cfg.retrieval.colbert_meta_file, encoding="utf-8").read().splitlines()]
    assert [x["pid"] for x in lines] == list(range(40))
    assert open(cfg.retrieval.colbert_meta_file, "rb").read() == open(whole.retrieval.colbert_meta_file, "rb").read()

    # nothing new: 0, and neither file is touched
    store = _index_dir(cfg) / "amdr_tokens.npz"
    before = (store.read_bytes(), open(cfg.retrieval.colbert_meta_file, "rb").read(), store.stat().st_mtime_ns)
    assert IncrementalColBERTBuilder(cfg).add_jsonl(inc) == 0
    assert (store.read_bytes(), open(cfg.retrieval.colbert_meta_file, "rb").read(), store.stat().st_mtime_ns) == before
    assert not (_index_dir(cfg) / "amdr_tokens.tmp.npz").exists()


def test_add_refuses_what_it_cannot_do(tmp_path, chunks):
    cfg = _cfg(tmp_path)
    inc = _jsonl(tmp_path / "incoming.jsonl", chunks[:3])
    with pytest.raises(RuntimeError, match="build_colbert_index"):  # no index yet
        IncrementalColBERTBuilder(cfg).add_jsonl(inc)
    build_colbert_index(cfg, chunks[:5])
    with pytest.raises(FileNotFoundError):
        IncrementalColBERTBuilder(cfg).add_jsonl(tmp_path / "missing.jsonl")
    cfg.retrieval.shard = "rows"
    with pytest.raises(RuntimeError, match="incremental add on a row-sharded index is not supported: rebuild and reload"):
        IncrementalColBERTBuilder(cfg).add_jsonl(inc)
    cfg.retrieval.shard = None
    cfg.retrieval.enable_colbert = False
    with pytest.raises(RuntimeError, match="disabled"):
        IncrementalColBERTBuilder(cfg).add_jsonl(inc)


def test_append_token_store(tmp_path):
    rng = np.random.default_rng(5)
    d = tmp_path / "idx"
    D0 = rng.standard_normal((9, 128)).astype(np.float32)
    artifacts.write_token_store(d, D0, np.array([0, 4, 9]))
    D1 = rng.standard_normal((6, 128)).astype(np.float32)
    artifacts.append_token_store(d, D1, np.array([0, 1, 6]))
    D, ptr = artifacts.read_token_store(d)
    assert np.array_equal(D, np.concatenate([D0, D1])) and ptr.tolist() == [0, 4, 9, 10, 15] and ptr.dtype == np.int64
    for bad_D, bad_ptr in ((D1, [1, 6]), (D1, [0, 3, 3, 6]), (D1, [0, 5]), (D1[:, :64], [0, 6])):
        with pytest.raises(ValueError):
            artifacts.append_token_store(d, bad_D, np.array(bad_ptr))
    assert np.array_equal(artifacts.read_token_store(d)[0], D)
    with pytest.raises(RuntimeError):
        artifacts.append_token_store(tmp_path / "nothing", D1, np.array([0, 6]))


def test_append_onto_a_plaid_directory_writes_this_builds_store(tmp_path):
    from test_artifacts import _write_plaid_fixture
    rng = np.random.default_rng(3)
    doclens = [5, 1, 17, 220, 3, 8, 40]
    D = rng.standard_normal((sum(doclens), 128)).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    d = artifacts.colbert_index_dir(str(tmp_path / "colbert"), "experiment", "law_en")
    _write_plaid_fixture(d, D, doclens, nbits=4)
    head, head_ptr = artifacts.read_plaid_index(d)
    assert not (d / "amdr_tokens.npz").exists()
    add = rng.standard_normal((33, 128)).astype(np.float32)
    artifacts.append_token_store(d, add, np.array([0, 32, 33]))
    assert (d / "amdr_tokens.npz").exists()
    got, ptr = artifacts.read_token_store(d)  # prefers the new file
    n = head.shape[0]
    assert np.array_equal(got[:n], head) and np.array_equal(got[n:], add)
    assert ptr.tolist() == head_ptr.tolist() + [n + 32, n + 33]


def test_a_meta_file_and_a_store_that_disagree_are_refused(tmp_path, chunks):
    """An add that died between its two writes: ids in the meta file without token rows.  The next add must not number
    its documents past them."""
    cfg = _cfg(tmp_path)
    build_colbert_index(cfg, chunks[:10])
    with open(cfg.retrieval.colbert_meta_file, "a", encoding="utf-8") as f:
        f.write(json.dumps({"pid": 10, "chunk": chunks[10].model_dump()}, ensure_ascii=False) + "\n")
    store = _index_dir(cfg) / "amdr_tokens.npz"
    before = (store.read_bytes(), open(cfg.retrieval.colbert_meta_file, "rb").read())
    with pytest.raises(RuntimeError, match="inconsistent.*[Rr]ebuild"):
        IncrementalColBERTBuilder(cfg).add_jsonl(_jsonl(tmp_path / "incoming.jsonl", chunks[11:14]))
    assert (store.read_bytes(), open(cfg.retrieval.colbert_meta_file, "rb").read()) == before
    assert artifacts.token_store_ndocs(_index_dir(cfg)) == 10


class _StubSearcher:
    """What the builder and the retriever ask of a MaxSimIndex, on the host."""

    def __init__(self, n_docs):
        self.n_docs, self.adds = n_docs, 0

    def info(self):
        return (self.n_docs, 0, 0, 0, 1, 1)

    def add(self, tokens, doc_ptr):
        self.n_docs += len(doc_ptr) - 1
        self.adds += 1


def _live_retriever(cfg, monkeypatch):
    """A registered ColBERTRetriever whose resident store is a stub of the store on disk."""
    from legal_rag_amd.retrieval.colbert_retriever import ColBERTRetriever, _identity
    opened = []

    def open_store(self):
        stamp = self._store_stamp()
        opened.append(_StubSearcher(artifacts.token_store_ndocs(self.index_dir())))
        return opened[-1], 0, stamp
    monkeypatch.setattr(ColBERTRetriever, "_open_store", open_store)
    monkeypatch.setattr(ColBERTRetriever, "_instances_by_key", {})
    monkeypatch.setattr(ColBERTRetriever, "_searcher_cache", {})
    r = ColBERTRetriever.from_config(cfg)
    assert ColBERTRetriever._instances_by_key[_identity(cfg.retrieval) + ("none",)] is r and len(opened) == 1
    return r, opened


def test_in_place_append_holds_the_retrievers_lock_across_the_write(tmp_path, chunks, monkeypatch):
    """Between the builder's write of the store and its append to the resident store a search thread sees the new mtime:
    it must wait, not reload the file (which holds the new rows already) and have them added a second time."""
    import threading
    from legal_rag_amd.retrieval.colbert_retriever import ColBERTRetriever
    cfg = _cfg(tmp_path)
    build_colbert_index(cfg, chunks[:30])
    r, opened = _live_retriever(cfg, monkeypatch)
    searcher = r._searcher
    real, seen = artifacts.append_token_store, {}

    def append_then_look(*a):
        out = real(*a)
        assert r._store_stamp() != r._store_mtime  # what a search thread would see now

        def other_thread():
            seen["free"] = ColBERTRetriever._registry_lock.acquire(blocking=False)
            if seen["free"]:
                ColBERTRetriever._registry_lock.release()
        t = threading.Thread(target=other_thread)
        t.start()
        t.join()
        return out
    monkeypatch.setattr(artifacts, "append_token_store", append_then_look)
    assert IncrementalColBERTBuilder(cfg).add_jsonl(_jsonl(tmp_path / "incoming.jsonl", chunks[30:40])) == 10
    assert seen == {"free": False}  # the reload of another thread waits for the append
    assert r._searcher is searcher and searcher.adds == 1 and searcher.n_docs == 40 and len(opened) == 1
    assert sorted(r._pid2chunk) == list(range(40)) and r.store_is_current()
    r._load_meta_and_collection()  # and afterwards nothing is reloaded
    assert r._searcher is searcher and len(opened) == 1


def test_a_store_reloaded_meanwhile_is_not_added_to_again(tmp_path, chunks, monkeypatch):
    """The same window, had a reload got through (here: from the builder's own thread, which the re-entrant lock lets
    pass): the reloaded store ends behind the new rows, so note_appended reads the file instead of adding."""
    cfg = _cfg(tmp_path)
    build_colbert_index(cfg, chunks[:30])
    r, opened = _live_retriever(cfg, monkeypatch)
    real = artifacts.append_token_store

    def append_then_reload(*a):
        out = real(*a)
        r._load_meta_and_collection()
        assert len(opened) == 2 and r._searcher is opened[1] and r._searcher.n_docs == 40
        return out
    monkeypatch.setattr(artifacts, "append_token_store", append_then_reload)
    assert IncrementalColBERTBuilder(cfg).add_jsonl(_jsonl(tmp_path / "incoming.jsonl", chunks[30:40])) == 10
    assert r._searcher.n_docs == 40 and all(s.adds == 0 for s in opened)  # 40 documents resident, not 50
    assert sorted(r._pid2chunk) == list(range(40)) and r.store_is_current()

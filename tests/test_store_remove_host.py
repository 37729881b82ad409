"""The host halves of the dense / ColBERT removal that need no GPU: artifacts.remove_from_token_store against a plain
filter, and the refusals of the builders that are decided before any device is touched."""
import numpy as np
import pytest


def _store(rng, lens):
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rng.standard_normal((int(ptr[-1]), 128)).astype(np.float32), ptr


@pytest.mark.parametrize("rows", [[0], [6], [2, 3, 4], [1, 3, 5], [0, 1, 2, 3, 5, 6], [5, 2, 2]],
                         ids=["first", "last", "run", "alternating", "all-but-one", "unordered-duplicate"])
def test_remove_from_token_store_is_the_plain_filter(tmp_path, rows):
    from legal_rag_amd import artifacts
    rng = np.random.default_rng(3)
    D, ptr = _store(rng, [1, 31, 32, 33, 64, 220, 33])
    artifacts.write_token_store(tmp_path, D, ptr)
    out = artifacts.remove_from_token_store(tmp_path, rows)
    assert out == tmp_path / "amdr_tokens.npz" and not (tmp_path / "amdr_tokens.tmp.npz").exists()
    keep = [j for j in range(7) if j not in set(rows)]
    want = np.concatenate([D[ptr[j]:ptr[j + 1]] for j in keep])
    got_D, got_ptr = artifacts.read_token_store(tmp_path)
    assert got_D.dtype == np.float32 and got_ptr.dtype == np.int64
    assert np.array_equal(got_D.view(np.uint32), want.view(np.uint32))
    assert got_ptr.tolist() == np.concatenate([[0], np.cumsum([ptr[j + 1] - ptr[j] for j in keep])]).tolist()
    assert artifacts.token_store_ndocs(tmp_path) == len(keep)


def test_remove_from_token_store_refusals_leave_the_file(tmp_path):
    from legal_rag_amd import artifacts
    D, ptr = _store(np.random.default_rng(4), [3, 4, 5])
    path = artifacts.write_token_store(tmp_path, D, ptr)
    before = path.read_bytes()
    for rows in ([0, 1, 2], [3], [-1]):
        with pytest.raises(ValueError):
            artifacts.remove_from_token_store(tmp_path, rows)
        assert path.read_bytes() == before
    with pytest.raises(RuntimeError):
        artifacts.remove_from_token_store(tmp_path / "nowhere", [0])


def test_colbert_builder_refuses_disabled_and_sharded(tmp_path):
    from legal_rag_amd.config import AppConfig
    from legal_rag_amd.retrieval.builders.incremental_colbert_builder import IncrementalColBERTBuilder
    cfg = AppConfig.for_data_dir(str(tmp_path), "en")
    cfg.retrieval.enable_colbert = False
    with pytest.raises(RuntimeError, match="disabled"):
        IncrementalColBERTBuilder(cfg).remove_ids(["a"])
    cfg.retrieval.enable_colbert = True
    cfg.retrieval.shard = "rows"
    with pytest.raises(RuntimeError, match="row-sharded"):
        IncrementalColBERTBuilder(cfg).remove_ids(["a"])
    cfg.retrieval.shard = None
    assert IncrementalColBERTBuilder(cfg).remove_ids([]) == 0
    with pytest.raises(RuntimeError, match="not found"):
        IncrementalColBERTBuilder(cfg).remove_ids(["a"])


def test_graph_retriever_binds_rows_again_after_an_in_place_removal():
    """A removal followed by an add of equal size leaves the index object and its row count as they were; the removal
    count (FlatIPIndex.rows_epoch) is what tells GraphRetriever that its row map and norms name the old rows."""
    from legal_rag_amd.retrieval.graph_retriever import GraphRetriever
    from legal_rag_amd.schemas import LawChunk

    def chunk(i):
        return LawChunk(id=f"src.txt::{i}", law_name="Synthetic Code", article_no=f"§ {i}", article_id=str(i), text=f"t{i}",
                        lang="en", source="src.txt")

    class Index:  # faiss-shaped, with a device matrix behind `native`, as vector_store.FlatIPIndex
        native = object()

        def __init__(self, X):
            self.X, self.rows_epoch = X, 0

        @property
        def ntotal(self):
            return self.X.shape[0]

        def reconstruct_n(self, i0, n):
            return self.X[i0:i0 + n]

    class Store:
        pass

    store = Store()
    store.chunks = [chunk(i) for i in range(4)]
    store.index = Index(np.diag([1.0, 2.0, 3.0, 4.0]).astype(np.float32))
    g = GraphRetriever.__new__(GraphRetriever)
    g.store = store
    g._bind_rows()
    assert g._row_norms().tolist() == [1.0, 2.0, 3.0, 4.0] and g._row_of["2"] == 2 and "1" in g._row_of
    # row 1 leaves, a new row comes: the same index object, the same number of rows
    store.chunks = [chunk(0), chunk(2), chunk(3), chunk(9)]
    store.index.X = np.diag([1.0, 3.0, 4.0, 9.0]).astype(np.float32)
    store.index.rows_epoch += 1
    assert g._row_norms().tolist() == [1.0, 3.0, 4.0, 9.0]
    assert g._row_of["2"] == 1 and g._row_of["9"] == 3 and "1" not in g._row_of

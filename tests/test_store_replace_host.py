"""The host halves of the dense / ColBERT replacement that need no GPU: artifacts.replace_in_token_store against a store
written from the edited arrays, the refusals that are decided before any device is touched, and the helper that finds the
rows of incoming chunks."""
import numpy as np
import pytest


def _store(rng, lens):
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rng.standard_normal((int(ptr[-1]), 128)).astype(np.float32), ptr


LENS = [1, 31, 32, 33, 64, 220, 33]


@pytest.mark.parametrize("rows, new_lens", [([0], [5]), ([6], [1]), ([2, 3, 4], [32, 33, 31]), ([1, 3, 5], [31, 2, 300]),
                                            (list(range(7)), [2, 2, 2, 2, 2, 2, 2]), ([5, 2], [220, 32])],
                         ids=["first", "last", "run", "alternating", "every-document", "unordered-same-lengths"])
def test_replace_in_token_store_equals_a_store_written_from_the_edited_arrays(tmp_path, rows, new_lens):
    from legal_rag_amd import artifacts
    rng = np.random.default_rng(3)
    D, ptr = _store(rng, LENS)
    D_new, ptr_new = _store(rng, new_lens)
    artifacts.write_token_store(tmp_path / "a", D, ptr)
    out = artifacts.replace_in_token_store(tmp_path / "a", rows, D_new, ptr_new)
    assert out == tmp_path / "a" / "amdr_tokens.npz" and not (tmp_path / "a" / "amdr_tokens.tmp.npz").exists()
    docs = [D[ptr[j]:ptr[j + 1]] for j in range(7)]
    for i, r in enumerate(rows):
        docs[r] = D_new[ptr_new[i]:ptr_new[i + 1]]
    want_ptr = np.concatenate([[0], np.cumsum([d.shape[0] for d in docs])]).astype(np.int64)
    artifacts.write_token_store(tmp_path / "b", np.concatenate(docs), want_ptr)
    (ga, pa), (gb, pb) = artifacts.read_token_store(tmp_path / "a"), artifacts.read_token_store(tmp_path / "b")
    assert ga.dtype == gb.dtype == np.float32 and pa.dtype == pb.dtype == np.int64
    assert ga.tobytes() == gb.tobytes() and pa.tobytes() == pb.tobytes()
    assert artifacts.token_store_ndocs(tmp_path / "a") == 7


def test_replace_in_token_store_refusals_leave_the_file(tmp_path):
    from legal_rag_amd import artifacts
    rng = np.random.default_rng(4)
    D, ptr = _store(rng, [3, 4, 5])
    new, new_ptr = _store(rng, [2, 2])
    path = artifacts.write_token_store(tmp_path, D, ptr)
    before = path.read_bytes()
    for rows, d, p in (([0, 3], new, new_ptr), ([-1, 0], new, new_ptr), ([1, 1], new, new_ptr), ([0], new, new_ptr),
                       ([0, 1], new[:, :64], new_ptr), ([0, 1], new, new_ptr[:2]), ([0, 1], new, np.asarray([0, 0, 4])),
                       ([0, 1], new, np.asarray([1, 2, 4]))):
        with pytest.raises(ValueError):
            artifacts.replace_in_token_store(tmp_path, rows, d, p)
        assert path.read_bytes() == before
    with pytest.raises(RuntimeError):
        artifacts.replace_in_token_store(tmp_path / "nowhere", [0], new[:2], new_ptr[:2])


def test_row_sharded_indexes_refuse(tmp_path):
    from legal_rag_amd.config import AppConfig
    from legal_rag_amd.retrieval.builders.incremental_colbert_builder import IncrementalColBERTBuilder
    from legal_rag_amd.retrieval.vector_store import ShardedFlatIPIndex
    wording = "replacement on a row-sharded index is not supported: rebuild and reload"
    with pytest.raises(RuntimeError, match=wording):  # (decided before the object's state is looked at)
        ShardedFlatIPIndex.__new__(ShardedFlatIPIndex).replace_rows([0], np.zeros((1, 4), np.float32))
    cfg = AppConfig.for_data_dir(str(tmp_path), "en")
    cfg.retrieval.enable_colbert = False
    with pytest.raises(RuntimeError, match="disabled"):
        IncrementalColBERTBuilder(cfg).replace_jsonl(tmp_path / "x.jsonl")
    cfg.retrieval.enable_colbert = True
    cfg.retrieval.shard = "rows"
    with pytest.raises(RuntimeError, match=wording):
        IncrementalColBERTBuilder(cfg).replace_jsonl(tmp_path / "x.jsonl")
    cfg.retrieval.shard = None
    with pytest.raises(FileNotFoundError):
        IncrementalColBERTBuilder(cfg).replace_jsonl(tmp_path / "x.jsonl")


def test_amended_finds_rows_and_lets_the_later_line_count():
    from legal_rag_amd.retrieval.builders._incremental import amended
    from legal_rag_amd.schemas import LawChunk

    def chunk(i, text="t"):
        return LawChunk(id=f"src.txt::{i}", law_name="Synthetic Code", article_no=f"§ {i}", article_id=str(i), text=text,
                        lang="en", source="src.txt")

    ids = [chunk(i).id for i in range(5)]
    found = amended([chunk(4, "a"), chunk(9, "b"), chunk(1, "c"), chunk(4, "d")], ids)
    assert list(found) == [1, 4] and found[1].text == "c" and found[4].text == "d"
    assert amended([chunk(9)], ids) == {}

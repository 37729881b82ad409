"""The host side of diversified search (retrieval/diversity.py, the config defaults, HybridRetriever's last stage), without
a GPU: a fake dense index answers amdr_mmr with the fp64 oracle of tests/mmr_adversary.py."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import mmr_adversary as M
from legal_rag_amd.config import RetrievalConfig, diversity_default
from legal_rag_amd.retrieval import hybrid_retriever as HR
from legal_rag_amd.retrieval.diversity import MAX_POOL, Diversity, configured, resolve
from legal_rag_amd.schemas import LawChunk, RetrievalHit


def test_diversity_validates_its_fields():
    d = Diversity()
    assert (d.lam, d.pool) == (0.7, 0) and Diversity(1, 64).lam == 1.0 and isinstance(Diversity(1).lam, float)
    for lam in (-0.01, 1.01, math.nan, math.inf):
        with pytest.raises(ValueError, match=r"lam must be in \[0, 1\]"):
            Diversity(lam)
    for lam in ("0.5", None, True):
        with pytest.raises(TypeError, match="lam must be a number"):
            Diversity(lam)
    for pool in (-1, 65):
        with pytest.raises(ValueError, match=r"pool must be 0 \(automatic\) or in \[1, 64\]"):
            Diversity(0.5, pool)
    for pool in (3.0, "3", True):
        with pytest.raises(TypeError, match="pool must be an int"):
            Diversity(0.5, pool)
    with pytest.raises(Exception):  # frozen
        d.lam = 0.1
    assert MAX_POOL == 64 and Diversity(0.5) == Diversity(0.5, 0) and hash(Diversity(0.5)) == hash(Diversity(0.5))


def test_automatic_pool_rule():
    auto = Diversity(0.5)
    assert [auto.pool_for(k) for k in (1, 3, 4, 10, 21, 22, 64)] == [10, 10, 12, 30, 63, 64, 64]
    assert Diversity(0.5, 20).pool_for(10) == 20 and Diversity(0.5, 10).pool_for(10) == 10
    with pytest.raises(ValueError, match="pool=5 is smaller than top_k=10"):
        Diversity(0.5, 5).pool_for(10)
    for d in (auto, Diversity(0.5, 64)):
        with pytest.raises(ValueError, match="at most 64 candidates per question, got top_k=65"):
            d.pool_for(65)


def test_config_default_and_its_overrides():
    off = RetrievalConfig()
    assert off.diversity_lambda is None and off.diversity_pool == 0 and configured(off) is None and diversity_default(off) is None
    on = RetrievalConfig(diversity_lambda=0.6, diversity_pool=24)
    assert configured(on) == Diversity(0.6, 24) == diversity_default(SimpleNamespace(retrieval=on))
    with pytest.raises(ValueError, match="lam must be in"):
        RetrievalConfig(diversity_lambda=1.5)
    with pytest.raises(ValueError, match="pool must be"):
        RetrievalConfig(diversity_lambda=0.5, diversity_pool=100)
    assert RetrievalConfig(diversity_pool=100).diversity_lambda is None  # the pool alone switches nothing on
    assert resolve(None, off) is None and resolve(None, on) == Diversity(0.6, 24)
    assert resolve(False, on) is None and resolve(False, off) is None
    assert resolve(Diversity(0.2), on) == Diversity(0.2) == resolve(Diversity(0.2), off)
    for bad in (0.5, True, "mmr", (0.5, 10)):
        with pytest.raises(TypeError, match="diversity must be a Diversity, None or False"):
            resolve(bad, on)
    assert resolve(None, SimpleNamespace()) is None  # a duck-typed config that never heard of it


# ---- the last stage, on a fake index -------------------------------------------------------------------------------------
class FakeNative:
    def __init__(self, X):
        self.X, self.calls = X, []

    def mmr(self, rows, rel, count, pool, k_sel, lam):
        self.calls.append((np.array(rows), np.array(rel), np.array(count), pool, k_sel, lam))
        return M.mmr_oracle(self.X, rows, rel, count, pool, k_sel, lam)


def chunk(i):
    return LawChunk(id=f"c{i}", law_name="L", article_no=str(i), article_id=f"a{i}", text=f"text {i}", lang="en")


def fake_retriever(n=12, d=8, cfg=None):
    X = M.int_matrix(n, d)
    chunks = [chunk(i) for i in range(n)]
    r = HR.HybridRetriever.__new__(HR.HybridRetriever)
    r.cfg = SimpleNamespace(retrieval=cfg or RetrievalConfig())
    native = FakeNative(X)
    r.dense = SimpleNamespace(store=SimpleNamespace(load=lambda: None, chunks=chunks, index=SimpleNamespace(native=native)))
    return r, chunks, native, X


def hit(c, score, channel="dense"):
    return RetrievalHit(chunk=c, score=score, rank=None, score_breakdown={"channel": [channel], "final_score": score})


def test_stage_runs_once_for_the_batch_after_the_dedup_and_keeps_the_hits():
    r, chunks, native, X = fake_retriever()
    stranger = chunk(99)  # a chunk the dense store does not hold: row -1, similar to nothing
    lists = [
        # chunk 1 twice (dense and graph): the dedup keeps the better one and re-sorts, so the pool is in score order
        [hit(chunks[4], 0.50), hit(chunks[1], 0.40), hit(chunks[2], 0.90), hit(chunks[1], 0.95, "graph"), hit(stranger, 0.7),
         hit(chunks[5], 0.3), hit(chunks[6], 0.2)],
        [],
        [hit(chunks[7], 0.1)],
    ]
    div, pool = r._diversity(Diversity(0.5, 5), 3, "search_batch")
    assert (div, pool) == (Diversity(0.5, 5), 5)
    deduped = [HR._dedup_keep_best(list(h)) for h in lists]
    assert [h.chunk.id for h in deduped[0]] == ["c1", "c2", "c99", "c4", "c5", "c6"]
    scores = [[h.score for h in hs] for hs in deduped]
    out = r._mmr_stage(deduped, 3, div, pool)
    assert len(native.calls) == 1, "one batched call for all questions"
    rows, rel, count, p, k, lam = native.calls[0]
    assert (p, k, lam) == (5, 3, 0.5) and count.tolist() == [5, 0, 1]
    assert rows[0].tolist() == [1, 2, -1, 4, 5] and rel[0].tolist() == [0.95, 0.9, 0.7, 0.5, 0.3]
    assert rows[1].tolist() == [-1] * 5 and rows[2].tolist() == [7, -1, -1, -1, -1]
    pos, val, sim, cnt = M.mmr_oracle(X, rows, rel, count, 5, 3, 0.5)
    assert cnt.tolist() == [3, 0, 1] and [len(o) for o in out] == [3, 0, 1]
    for q, hits in enumerate(out):
        assert [h.chunk.id for h in hits] == [deduped[q][int(i)].chunk.id for i in pos[q, :cnt[q]]]
        assert [h.rank for h in hits] == list(range(1, len(hits) + 1))
        assert [h.score for h in hits] == [scores[q][int(i)] for i in pos[q, :cnt[q]]], "score untouched"
        assert [h.score_breakdown["mmr"] for h in hits] == val[q, :cnt[q]].tolist()
        assert [h.score_breakdown["mmr_max_sim"] for h in hits] == sim[q, :cnt[q]].tolist()
        assert all(h.score_breakdown["final_score"] == h.score for h in hits)
    assert out[0][0].chunk.id == "c1" and out[0][0].score_breakdown["channel"] == ["dense", "graph"]
    # rows 1 and 2 of the integer matrix are parallel: with the relevances this close the twin loses its place
    assert pos[0].tolist()[:2] == [0, 2] and sim[0][1] == 0.0
    assert r._mmr_stage([], 3, div, pool) == [] and len(native.calls) == 1


def test_refusals_need_no_device():
    r, chunks, native, X = fake_retriever()
    assert r._diversity(None, 10, "search") is None and r._diversity(False, 10, "search") is None
    assert r._diversity(Diversity(0.5), 10, "search") == (Diversity(0.5), 30)
    with pytest.raises(ValueError, match=r"HybridRetriever.search: diversity: MMR selection ranks at most 64"):
        r._diversity(Diversity(0.5), 65, "search")
    r.dense.store.index.spec = object()
    with pytest.raises(ValueError, match="HybridRetriever.search_batch: .* row-sharded index"):
        r._diversity(Diversity(0.5), 10, "search_batch")
    del r.dense.store.index.spec
    r.dense.store.index.native = None
    with pytest.raises(ValueError, match="needs this package's own dense index resident on the GPU"):
        r._diversity(Diversity(0.5), 10, "search_batch_arrays")
    r.dense = object()  # a duck-typed dense retriever
    with pytest.raises(ValueError, match="needs this package's own dense index"):
        r._diversity(Diversity(0.5), 10, "search")
    # the configured default goes the same way
    r2, *_ = fake_retriever(cfg=RetrievalConfig(diversity_lambda=0.25, diversity_pool=40))
    assert r2._diversity(None, 10, "search") == (Diversity(0.25, 40), 40) and r2._diversity(False, 10, "search") is None


def test_scatter_carries_the_mmr_columns_only_when_a_part_has_them():
    n, top_k = 4, 3
    base = {"rows": np.zeros((2, top_k), dtype=np.int64), "scores": np.ones((2, top_k)), "count": np.full(2, 3, dtype=np.int32),
            "channel_mask": np.ones((2, top_k), dtype=np.int32), "zh_exact": np.ones(2, dtype=bool)}
    with_mmr = dict(base, mmr=np.full((2, top_k), 0.5), mmr_max_sim=np.full((2, top_k), 0.25))
    out = HR.HybridRetriever._scatter_columns(n, top_k, False, [], [([0, 2], with_mmr), ([1], {k: v[:1] for k, v in base.items()})])
    assert out["mmr"].shape == (n, top_k) and out["mmr"][[0, 2]].tolist() == [[0.5] * 3] * 2 and (out["mmr"][[1, 3]] == 0.0).all()
    assert (out["mmr_max_sim"][[0, 2]] == 0.25).all()
    plain = HR.HybridRetriever._scatter_columns(n, top_k, False, [], [([0, 2], base), ([1], {k: v[:1] for k, v in base.items()})])
    assert "mmr" not in plain and "mmr_max_sim" not in plain
    assert [name for name, *_ in HR.MMR_COLUMNS] == ["mmr", "mmr_max_sim"] and len(HR.COLUMNS) == 13

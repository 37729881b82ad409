"""Diversified search through the public interface (retrieval/diversity.py, HybridRetriever, HybridEngine.diversify) on the
UCC-en fixture with the stand-in encoders: every entry point with diversity on returns what the fp64 oracle
(tests/mmr_adversary.py) selects from the list the same call returns with diversity off at depth `pool`.

The fixture's rows are real-valued, so each comparison first checks the oracle's certificate for that list — the winner of
every step leads by more than 2 (1 - lam) E, E the rounding bound of an fp32 Gram — and then asks for EQUAL ids in equal
order.  The questions are fixed and the stand-in encoders deterministic, so the certificate is a property of this file
(of 22 questions tried, 20 certify in every call form; "Short Titles" is one that does not).

search() and search_batch() take different dense kernels, whose fp32 scores differ in the last bits on real-valued rows,
so each entry point is compared with ITS OWN result at diversity off, never with another entry point's."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest

import mmr_adversary as M
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LAM, TOP_K, POOL = 0.5, 10, 30  # Diversity(0.5): pool = min(64, max(3 * 10, 10))
QUESTIONS = ["what warranty does a merchant give that goods are merchantable", "firm offer by a merchant in a signed writing",
             "statute of frauds signed writing sale of goods price of $500", "risk of loss passes to the buyer",
             "when may a buyer reject goods that fail to conform to the contract", "remedies of the seller on breach"]


def configure(cfg):
    cfg.retrieval.encoder_backend = "hashing"
    cfg.retrieval.enable_rerank = False
    cfg.retrieval.top_k = 40           # the per-channel depth of every call here, whatever its top_k
    cfg.retrieval.min_final_score = -1.0
    cfg.retrieval.graph_seed_k = 12    # (its default follows top_k)
    return cfg


@pytest.fixture(scope="module")
def ucc(tmp_path_factory):
    """(config, chunks) of the UCC-en indexes built with the product builders; no ColBERT, a law graph beside them."""
    from legal_rag_amd.config import AppConfig
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    from test_graph_device_gpu import ucc_graph
    data = tmp_path_factory.mktemp("mmr_data")
    cfg = configure(AppConfig.for_data_dir(str(data), "zh").with_lang("en"))
    cfg.retrieval.enable_colbert = False
    chunks = load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")
    build_faiss_index(cfg, chunks)
    build_bm25_index(cfg, chunks)
    gpath = data / "ucc_graph.jsonl"
    ucc_graph(chunks, gpath)
    cfg.paths.law_graph_jsonl = str(gpath)
    return cfg, chunks


@pytest.fixture(scope="module")
def retr(ucc):
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    r = HybridRetriever(ucc[0])
    r.search(QUESTIONS[0], top_k=TOP_K)  # loads the indexes
    return r


@pytest.fixture(scope="module")
def matrix(retr):
    idx = retr.dense.store.index.native
    X = idx.read_rows(0, idx.ntotal)
    X.setflags(write=False)
    return X


def dump(h, drop=()):
    sb = {k: v for k, v in (h.score_breakdown or {}).items() if k not in drop}
    return {"id": h.chunk.id, "score": float(h.score), "rank": h.rank, "source": h.source, "breakdown": sb}


def same_hits(a, b, what, drop=()):
    """Equal dumps, and on a difference the first field that differs."""
    da, db = [dump(h, drop) for h in a], [dump(h, drop) for h in b]
    assert len(da) == len(db), (what, len(da), len(db))
    for j, (x, y) in enumerate(zip(da, db)):
        for key in ("id", "score", "rank", "source"):
            assert x[key] == y[key], (what, j, key, x[key], y[key])
        assert set(x["breakdown"]) == set(y["breakdown"]), (what, j, sorted(x["breakdown"]), sorted(y["breakdown"]))
        for key, v in x["breakdown"].items():
            assert v == y["breakdown"][key], (what, j, key, v, y["breakdown"][key])


def select(X, rows, rel, lam=LAM, top_k=TOP_K, pool=POOL, what=""):
    """The oracle's (positions, mmr, maxsim) for one candidate list, its certificate checked first."""
    pos, val, sim, lead = M.mmr_one(X, rows, rel, len(rows), pool, top_k, lam)
    bar = 2.0 * (1.0 - lam) * M.cos_bound(X.shape[1])
    print(what, "lead", lead, "bar", bar)
    assert lead > bar, (what, "this list does not certify: pick another question", lead, bar)
    return pos, val, sim


def check_hits(retr, X, got, plain, what, lam=LAM, top_k=TOP_K, pool=POOL):
    """got: the diversified hits; plain: the same call with diversity off at top_k = pool."""
    from legal_rag_amd.retrieval.scope import resolver_for
    row_of = resolver_for(retr.dense.store.chunks).row_of
    pos, val, sim = select(X, [row_of(h.chunk.id) for h in plain], [float(h.score) for h in plain], lam, top_k, pool, what)
    assert [h.chunk.id for h in got] == [plain[p].chunk.id for p in pos], what
    assert [h.rank for h in got] == list(range(1, len(got) + 1))
    E = M.cos_bound(X.shape[1])
    for h, p, v, s in zip(got, pos, val, sim):
        assert dump(h, ("mmr", "mmr_max_sim", "rank")) | {"rank": 0} == dump(plain[p], ("rank",)) | {"rank": 0}, "hit untouched"
        assert abs(h.score_breakdown["mmr"] - v) <= (1.0 - lam) * E and abs(h.score_breakdown["mmr_max_sim"] - s) <= E


def test_search_and_search_batch_select_what_the_oracle_selects(retr, matrix):
    from legal_rag_amd.retrieval.diversity import Diversity
    div = Diversity(LAM)
    assert div.pool_for(TOP_K) == POOL
    batch = retr.search_batch(QUESTIONS, top_k=TOP_K, diversity=div)
    plain = retr.search_batch(QUESTIONS, top_k=POOL)
    moved = 0
    for j, q in enumerate(QUESTIONS):
        assert len(plain[j]) == POOL
        check_hits(retr, matrix, batch[j], plain[j], ("search_batch", q))
        check_hits(retr, matrix, retr.search(q, top_k=TOP_K, diversity=div), retr.search(q, top_k=POOL), ("search", q))
        moved += [h.chunk.id for h in batch[j]] != [h.chunk.id for h in plain[j][:TOP_K]]
    assert moved >= len(QUESTIONS) // 2, "the selection should reorder most lists of a corpus of near-duplicates"


def test_columnar_form_selects_on_the_device(retr, matrix):
    from legal_rag_amd.retrieval.diversity import Diversity
    div = Diversity(LAM)
    plain = retr.search_batch_arrays(QUESTIONS, top_k=POOL, diversity=False)
    full = retr.search_batch_arrays(QUESTIONS, top_k=TOP_K, diversity=div)
    lean = retr.search_batch_arrays(QUESTIONS, top_k=TOP_K, diversity=div, values=False)
    hits = retr.search_batch(QUESTIONS, top_k=TOP_K, diversity=div)
    E = M.cos_bound(matrix.shape[1])
    assert full["mmr"].shape == full["mmr_max_sim"].shape == (len(QUESTIONS), TOP_K) and "mmr" not in lean and "mmr" not in plain
    for j, q in enumerate(QUESTIONS):
        m = int(plain["count"][j])
        pos, val, sim = select(matrix, plain["rows"][j, :m], plain["scores"][j, :m], what=("arrays", q))
        assert full["count"][j] == lean["count"][j] == len(pos) == TOP_K
        assert full["rows"][j].tolist() == lean["rows"][j].tolist() == [int(plain["rows"][j, p]) for p in pos], q
        assert full["scores"][j].tolist() == lean["scores"][j].tolist() == [float(plain["scores"][j, p]) for p in pos]
        assert full["channel_mask"][j].tolist() == lean["channel_mask"][j].tolist() == [int(plain["channel_mask"][j, p]) for p in pos]
        assert np.array_equal(full["values"][j], plain["values"][j, pos])
        assert np.abs(full["mmr"][j] - val).max() <= (1 - LAM) * E and np.abs(full["mmr_max_sim"][j] - sim).max() <= E
        # the rows of one index are distinct chunks: the hit-object path selects the same ones
        assert [full["chunks"][int(x)].id for x in full["rows"][j]] == [h.chunk.id for h in hits[j]]


def test_off_is_the_retriever_as_it_was(retr, ucc):
    from legal_rag_amd.retrieval.diversity import Diversity
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    base = [[dump(h) for h in hits] for hits in retr.search_batch(QUESTIONS, top_k=TOP_K)]
    for kw in (dict(diversity=None), dict(diversity=False)):
        assert [[dump(h) for h in hits] for hits in retr.search_batch(QUESTIONS, top_k=TOP_K, **kw)] == base
        for q in QUESTIONS:
            same_hits(retr.search(q, top_k=TOP_K, **kw), retr.search(q, top_k=TOP_K), ("search", q, kw))
    a = retr.search_batch_arrays(QUESTIONS, top_k=TOP_K)
    for kw in (dict(diversity=None), dict(diversity=False)):
        b = retr.search_batch_arrays(QUESTIONS, top_k=TOP_K, **kw)
        assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in ("rows", "scores", "count", "channel_mask", "values"))
    # a configured default is honoured, and one call can override it either way
    cfg2 = copy.deepcopy(ucc[0])
    cfg2.retrieval.diversity_lambda, cfg2.retrieval.diversity_pool = LAM, 0
    r2 = HybridRetriever(cfg2)
    want = [[dump(h) for h in hits] for hits in retr.search_batch(QUESTIONS, top_k=TOP_K, diversity=Diversity(LAM))]
    assert want != base
    assert [[dump(h) for h in hits] for hits in r2.search_batch(QUESTIONS, top_k=TOP_K)] == want
    for q in QUESTIONS:
        same_hits(r2.search(q, top_k=TOP_K), retr.search(q, top_k=TOP_K, diversity=Diversity(LAM)), ("configured search", q))
        same_hits(r2.search(q, top_k=TOP_K, diversity=False), retr.search(q, top_k=TOP_K), ("configured, switched off", q))
    assert [[dump(h) for h in hits] for hits in r2.search_batch(QUESTIONS, top_k=TOP_K, diversity=False)] == base
    other = r2.search_batch(QUESTIONS, top_k=TOP_K, diversity=Diversity(0.9, pool=20))
    assert [[dump(h) for h in hits] for hits in other] == \
        [[dump(h) for h in hits] for hits in retr.search_batch(QUESTIONS, top_k=TOP_K, diversity=Diversity(0.9, pool=20))]
    assert np.array_equal(r2.search_batch_arrays(QUESTIONS, top_k=TOP_K)["rows"],
                          retr.search_batch_arrays(QUESTIONS, top_k=TOP_K, diversity=Diversity(LAM))["rows"])


def test_lambda_one_is_the_plain_ranking(retr):
    from legal_rag_amd.retrieval.diversity import Diversity
    plain = retr.search_batch(QUESTIONS, top_k=TOP_K)
    got = retr.search_batch(QUESTIONS, top_k=TOP_K, diversity=Diversity(1.0))
    for a, b in zip(got, plain):
        assert [dump(h, ("mmr", "mmr_max_sim")) for h in a] == [dump(h) for h in b]
        assert [h.score_breakdown["mmr"] for h in a] == [float(h.score) for h in b]
    arr = retr.search_batch_arrays(QUESTIONS, top_k=TOP_K, diversity=Diversity(1.0))
    off = retr.search_batch_arrays(QUESTIONS, top_k=TOP_K)
    assert np.array_equal(arr["rows"], off["rows"]) and np.array_equal(arr["scores"], off["scores"])


def test_scoped_graph_and_blank_questions_in_one_batch(retr, matrix, ucc):
    from legal_rag_amd.retrieval.diversity import Diversity
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from legal_rag_amd.retrieval.scope import Scope
    cfg = copy.deepcopy(ucc[0])
    cfg.retrieval.enable_graph = True
    hr = HybridRetriever(cfg)
    assert hr.graph is not None
    chunks = ucc[1]
    sizes = {}
    for c in chunks:
        sizes[c.section] = sizes.get(c.section, 0) + 1
    big = Scope(section=max(sizes, key=sizes.get))
    qs = [QUESTIONS[0], QUESTIONS[2], "", QUESTIONS[3]]
    scopes = [big, None, None, None]
    decisions = [None, SimpleNamespace(mode="GRAPH_AUGMENTED"), None, SimpleNamespace(mode="HYBRID")]
    got = hr.search_batch(qs, top_k=TOP_K, scopes=scopes, decisions=decisions, diversity=Diversity(LAM))
    plain = hr.search_batch(qs, top_k=POOL, scopes=scopes, decisions=decisions)
    assert any("graph" in (h.score_breakdown.get("channel") or []) for h in plain[1]), "the graph channel contributed"
    for j in range(len(qs)):
        if not plain[j]:
            assert got[j] == []
            continue
        check_hits(hr, matrix, got[j], plain[j], ("mixed batch", j), pool=POOL)
        if scopes[j] is not None:
            assert all(h.chunk.section == scopes[j].section for h in got[j])
        one = hr.search(qs[j], top_k=TOP_K, scope=scopes[j], decision=decisions[j], diversity=Diversity(LAM))
        check_hits(hr, matrix, one, hr.search(qs[j], top_k=POOL, scope=scopes[j], decision=decisions[j]), ("mixed, alone", j))
    # the columnar form: scoped parts and plain parts go through the same device call
    arr = hr.search_batch_arrays([qs[0], qs[3]], top_k=TOP_K, scopes=[big, None], diversity=Diversity(LAM))
    for j, k in ((0, 0), (1, 3)):
        assert [arr["chunks"][int(x)].id for x in arr["rows"][j, :arr["count"][j]]] == [h.chunk.id for h in got[k]]


def test_refusals_come_before_any_launch(retr, ucc, monkeypatch):
    from legal_rag_amd import _native
    from legal_rag_amd.retrieval.diversity import Diversity
    from legal_rag_amd.retrieval.engine import HybridEngine
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    div = Diversity(LAM)
    launched = []
    monkeypatch.setattr(HybridRetriever, "_run", lambda self, *a, **k: launched.append(1))
    calls = (lambda **kw: retr.search(QUESTIONS[0], **kw), lambda **kw: retr.search_batch(QUESTIONS, **kw),
             lambda **kw: retr.search_batch_arrays(QUESTIONS, **kw))
    for call in calls:
        with pytest.raises(ValueError, match=r"at most 64 candidates per question, got top_k=65"):
            call(top_k=65, diversity=div)
        with pytest.raises(ValueError, match="pool=5 is smaller than top_k=10"):
            call(top_k=10, diversity=Diversity(LAM, pool=5))
        with pytest.raises(TypeError, match="diversity must be a Diversity"):
            call(top_k=10, diversity=0.5)
    index = retr.dense.store.index
    monkeypatch.setattr(index, "spec", SimpleNamespace(group=None), raising=False)
    for call in calls:
        with pytest.raises(ValueError, match="does not run on a row-sharded index"):
            call(top_k=10, diversity=div)
    monkeypatch.delattr(index, "spec")
    stub = HybridRetriever.__new__(HybridRetriever)
    stub.cfg = ucc[0]
    stub.dense = SimpleNamespace(store=SimpleNamespace(load=lambda: None, index=SimpleNamespace(native=None)))
    for name in ("search", "search_batch", "search_batch_arrays"):
        with pytest.raises(ValueError, match="needs this package's own dense index resident on the GPU"):
            getattr(stub, name)(QUESTIONS[0] if name == "search" else QUESTIONS, top_k=10, diversity=div)
    assert not launched
    # the engine's own refusals
    rng = np.random.default_rng(5)
    X = rng.standard_normal((20, 8)).astype(np.float32)
    import torch
    res = SimpleNamespace(ids=torch.zeros((1, 4), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="row-sharded"):
        HybridEngine(_native.DenseIndex(X), None, shard_offset=0).diversify(res, 2, 0.5, 4)
    with pytest.raises(ValueError, match="dense_row2uid"):
        HybridEngine(_native.DenseIndex(X), None, dense_row2uid=torch.arange(20, device="cuda")).diversify(res, 2, 0.5, 4)


def test_per_channel_fallback_path_diversifies_too(retr, matrix, monkeypatch):
    """AMDR_SEARCH_NATIVE=0: search() fuses per-channel lists on the host side of the API; MMR is still the last stage."""
    from legal_rag_amd.retrieval.diversity import Diversity
    monkeypatch.setenv("AMDR_SEARCH_NATIVE", "0")
    q = QUESTIONS[0]
    plain = retr.search(q, top_k=POOL)
    got = retr.search(q, top_k=TOP_K, diversity=Diversity(LAM))
    check_hits(retr, matrix, got, plain, ("per-channel path", q))


def test_captured_step_with_diversity_replays_to_the_same_bits():
    """HybridEngine.capture(..., diversity=): a replay over new queries equals the eager step bit for bit and allocates
    nothing (the MMR kernel has no workspace)."""
    import torch
    from legal_rag_amd import _native as nat
    from legal_rag_amd.retrieval.engine import HybridEngine
    from oracle import bm25 as OB
    rng = np.random.default_rng(3)
    n, d, nq, k = 400, 64, 6, 12
    C = rng.standard_normal((8, d))
    X = (C[rng.integers(0, 8, size=n)] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    words = [f"w{i}" for i in range(120)]
    docs = [[words[j] for j in rng.integers(0, 120, size=int(rng.integers(5, 40)))] for _ in range(n)]
    ob = OB.BM25Okapi(docs)
    csr = OB.to_csr(ob)
    bm = nat.BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"], csr["doc_len"], ob.avgdl, ob.k1, ob.b)
    eng = HybridEngine(nat.DenseIndex(X), bm, None)
    params = nat.make_fuse_params(min_final_score=0.0)
    dev = torch.device("cuda", 0)
    Q = torch.zeros((nq, d), dtype=torch.float32, device=dev)
    q_terms, q_ptr = nat.BM25Index.pack_queries([[int(t) for t in rng.integers(0, 120, size=5)] for _ in range(nq)])
    q_terms_d, q_ptr_d = torch.from_numpy(q_terms).to(dev), torch.from_numpy(q_ptr).to(dev)

    def write(seed):
        r = np.random.default_rng(seed)
        q = X[r.integers(0, n, size=nq)] + 0.1 * r.standard_normal((nq, d)).astype(np.float32)
        Q.copy_(torch.from_numpy((q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)))
        q_terms_d.copy_(torch.from_numpy(r.integers(0, 120, size=q_terms.size).astype(np.int32)))

    def snapshot(res):
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (res.ids, res.vals, res.mask, res.count, res.mmr_pos, res.mmr, res.mmr_max_sim)]
    kw = dict(q_emb=Q, q_terms=q_terms_d, q_ptr=q_ptr_d, diversity=(5, 0.5, 16))
    write(1)
    graph, gres = eng.capture(params, k, **kw)
    assert tuple(gres.ids.shape) == (nq, 5)
    g0 = nat.workspace_growths()
    for seed in (2, 3):
        write(seed)
        graph.replay()
        got = snapshot(gres)
        assert nat.workspace_growths() == g0
        exp = snapshot(eng.search_batch(params, k, **kw))
        assert nat.workspace_growths() == g0
        for a, b in zip(got, exp):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        off = eng.search_batch(params, k, **{**kw, "diversity": None})
        torch.cuda.synchronize()
        ids, cnt = off.ids.cpu().numpy(), off.count.cpu().numpy()
        assert (got[3] == np.minimum(cnt, 5)).all() and (got[4] < 16).all()
        for q in range(nq):  # the selected ids are the fused ids at the selected positions
            assert got[0][q, :got[3][q]].tolist() == ids[q, got[4][q, :got[3][q]]].tolist()
        assert any(got[4][q, :got[3][q]].tolist() != list(range(got[3][q])) for q in range(nq)), "nothing was reordered"

"""Graph channel on the device (csrc/graph.hip, amdr_graph_*): the walk against the reference's vectors and the host
walk on random graphs, the search against the reference's vectors, search_batch with graph_channel="device" against
"host" on UCC-en, and the captured step against eager."""
import json
import random
import types

import numpy as np
import pytest

from graph_adversary import random_graph
from test_graph import G, HostStore, make_cfg, node_view

pytestmark = pytest.mark.gpu


def walk_params(t, cfg, relation_max_depth=None, rel_types=None, min_conf=0.0, limit=80):
    """amdr_graph_params_t of one LawGraphStore.walk call, resolved as walk() resolves its arguments."""
    from legal_rag_amd import _native
    from legal_rag_amd.retrieval.graph_retriever import _depth_bound
    rcfg = cfg.retrieval
    rmd = relation_max_depth if relation_max_depth is not None else (getattr(rcfg, "graph_walk_depths", None)
                                                                     or {"default": 2})
    if rel_types is None:
        rel_types = getattr(rcfg, "graph_rel_types", None)
    dd = rmd.get("default", 2)
    allowed = {str(r) for r in rel_types} if rel_types else None
    limit = max(1, int(limit))
    md = np.array([_depth_bound(rmd.get(r, dd)) for r in t.rel_names] or [0], np.int32)
    al = np.array([1 if allowed is None or r in allowed else 0 for r in t.rel_names] or [0], np.int32)
    return _native.GraphIndex.host_params(limit, _depth_bound(dd), float(min_conf or 0.0), md, al,
                                          np.ones(max(1, len(t.rel_names))), np.ones(limit + 1))


def device_index(gs, chunks=(), norms=None):
    from legal_rag_amd import _native
    from legal_rag_amd.retrieval.graph_retriever import build_graph_tables
    t = build_graph_tables(gs, list(chunks))
    norms = np.ones(len(t.row_node), np.float32) if norms is None else norms
    g = _native.GraphIndex(t.node_ptr, t.edge_dst, t.edge_rel, t.conf_raw, t.conf_eff, t.evidence, t.present,
                           t.node_row, t.row_node, norms, t.row_lang, n_rel=len(t.rel_names), device=0)
    return g, t


def device_walk_views(gs, g, t, start_lists, **args):
    from legal_rag_amd.retrieval.graph_store import _clean
    idx = {a: i for i, a in enumerate(t.names)}
    seeds = [[idx[_clean(x)] for x in s if _clean(x) and _clean(x) in idx] for s in start_lists]
    p, keep = walk_params(t, gs.cfg, **args)
    res = g.walk(seeds, p)
    del keep
    out = []
    for walk in res:
        views = []
        for node, depth, parent, rel, ev, conf in walk:
            stored = gs.nodes[t.names[node]]
            meta = stored.meta or {}
            views.append({"article_id": t.names[node], "graph_depth": depth, "graph_parent": t.names[parent],
                          "relations": [t.rel_names[rel]], "edge_conf": conf if ev else meta.get("_edge_conf"),
                          "has_evidence": bool(ev) or "_edge_evidence" in meta})
        out.append(views)
    return out


@pytest.mark.parametrize("case", G["walk"], ids=[f"walk{i}" for i in range(len(G["walk"]))])
def test_device_walk_matches_reference(case):
    from legal_rag_amd.retrieval.graph_store import LawGraphStore
    gs = LawGraphStore(make_cfg())
    g, t = device_index(gs)
    a = dict(case["args"])
    starts = a.pop("start_ids")
    got = device_walk_views(gs, g, t, [starts], **a)[0]
    assert got == case["nodes"]
    g.close()


def test_device_walk_equals_host_walk_on_random_graphs(tmp_path):
    from legal_rag_amd.retrieval.graph_store import LawGraphStore
    rng = random.Random(7)
    checked = cut = deep = 0
    sizes = [rng.choice([3, 10, 40, 200, 1500]) for _ in range(300)] + [20000]  # the last one beyond the LDS bound
    for gi, n in enumerate(sizes):
        path = tmp_path / f"g{gi}.jsonl"
        random_graph(rng, n, path)
        cfg = make_cfg()
        cfg.paths.law_graph_jsonl = str(path)
        gs = LawGraphStore(cfg)
        gs.load()
        g, t = device_index(gs)
        if n == 20000:
            assert len(t.names) > 12288  # the workspace claim-slot path
        for _ in range(3 if n < 20000 else 8):
            args = {"limit": rng.choice([0, 1, 2, 5, 17, 80, 800, 4096]),
                    "relation_max_depth": rng.choice([None, {"default": 0}, {"default": 1}, {"default": 3, "next": 1},
                                                      {"default": 2, "cite": 4, "x": 0}, {"default": 6}]),
                    "rel_types": rng.choice([None, None, ["cite", "next", "neighbor"], ["x"]]),
                    "min_conf": rng.choice([0.0, 0.0, 0.5, 0.8])}
            batch = [[rng.choice([str(rng.randrange(n)), f" {rng.randrange(n)} ", "absent0", "nope"])
                      for _ in range(rng.choice([1, 2, 5, 30]))] for _ in range(4)]
            got = device_walk_views(gs, g, t, batch, **args)
            for starts, gv in zip(batch, got):
                exp = [node_view(x) for x in gs.walk(starts, **args)]
                assert gv == exp, (gi, n, args, starts)
                checked += 1
                cut += int(len(exp) == max(1, args["limit"]) and len(exp) > 1)
                deep += int(any(v["graph_depth"] >= 3 for v in exp))
        g.close()
    assert checked >= 900 and cut > 20 and deep > 20


class DeviceStore(HostStore):
    def __init__(self):
        from legal_rag_amd.retrieval.vector_store import FlatIPIndex
        super().__init__()
        X = np.stack([self.table[c.text] for c in self.chunks]).astype(np.float32)
        self.index = FlatIPIndex(X, device=0)


def test_device_search_matches_reference():
    from legal_rag_amd.retrieval.graph_retriever import GraphRetriever
    from legal_rag_amd.retrieval.graph_store import LawGraphStore
    store = DeviceStore()
    tol = 2e-6
    for case in G["search"]:
        a = case["args"]
        cfg = make_cfg(**a["retrieval"])
        gr = GraphRetriever(cfg, graph=LawGraphStore(cfg), store=store)
        rows = [max(r for r, c in enumerate(store.chunks) if c.article_id == i) for i in a["seed_ids"]]
        hits = gr.search_device(store.q[None], np.array([rows + [0]], np.int64), np.array([len(rows)], np.int32),
                                top_k=a["top_k"], lang=a["lang"])[0]
        exp = case["hits"]
        assert [h.chunk.article_id for h in hits] == [e["article_id"] for e in exp], a
        for h, e in zip(hits, exp):
            assert h.rank == e["rank"] and h.source == e["source"] == "graph" and h.chunk.source == e["chunk_source"]
            sb, eb = h.score_breakdown, e["score_breakdown"]
            assert set(sb) == set(eb)
            for key in ("channel", "graph_depth", "relations", "depth_decay", "relation_weight", "edge_conf"):
                assert sb[key] == eb[key], key
            assert abs(sb["semantic"] - eb["semantic"]) <= tol and abs(sb["final"] - eb["final"]) <= tol
            assert abs(h.score - e["score"]) <= tol
    assert store.embedded == 0 and all(c.source == "src.txt" for c in store.chunks)


def ucc_graph(chunks, path, seed=11):
    """Seeded synthetic graph on the UCC chunk ids: prev/next chains plus random cite / defined_by edges."""
    rng = random.Random(seed)
    ids = [c.article_id for c in chunks]
    with open(path, "w", encoding="utf-8") as f:
        for i, aid in enumerate(ids):
            nbs = []
            if i + 1 < len(ids):
                nbs.append({"id": ids[i + 1], "relation": "next", "conf": 1.0})
            if i > 0:
                nbs.append({"id": ids[i - 1], "relation": "prev", "conf": 1.0})
            for _ in range(rng.randrange(4)):
                e = {"id": rng.choice(ids), "relation": rng.choice(["cite", "defined_by"]),
                     "conf": round(rng.uniform(0.3, 1.0), 3)}
                if rng.random() < 0.4:
                    e["evidence"] = {"span": "see " + e["id"]}
                nbs.append(e)
            f.write(json.dumps({"article_id": aid, "neighbors": nbs}) + "\n")


def ucc_retriever(tmp_path, channel):
    from legal_rag_amd.config import AppConfig
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from conftest import GOLDEN
    cfg = AppConfig.for_data_dir(str(tmp_path), "zh").with_lang("en")
    cfg.retrieval.encoder_backend = "hashing"
    cfg.retrieval.enable_colbert = False
    cfg.retrieval.enable_rerank = False
    cfg.retrieval.enable_graph = True
    cfg.retrieval.graph_channel = channel
    chunks = load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")
    if not (tmp_path / "built").exists():
        build_faiss_index(cfg, chunks)
        build_bm25_index(cfg, chunks)
        (tmp_path / "built").write_text("1")
    gpath = tmp_path / "ucc_graph.jsonl"
    if not gpath.exists():
        ucc_graph(chunks, gpath)
    cfg.paths.law_graph_jsonl = str(gpath)
    hr = HybridRetriever(cfg)
    assert hr.graph is not None
    return hr, chunks


def test_search_batch_device_graph_matches_host_on_ucc(tmp_path):
    from legal_rag_amd.evaluation import synthetic_queries
    hr_h, chunks = ucc_retriever(tmp_path, "host")
    hr_d, _ = ucc_retriever(tmp_path, "device")
    qs = [q for q, _, _ in synthetic_queries(chunks, seed=0)][:160]
    decisions = [types.SimpleNamespace(mode="GRAPH_AUGMENTED" if i % 3 else "HYBRID") for i in range(len(qs))]
    exp = hr_h.search_batch(qs, top_k=10, decisions=decisions)
    got = hr_d.search_batch(qs, top_k=10, decisions=decisions)
    graph_hits = 0
    for qi, (e, g) in enumerate(zip(exp, got)):
        assert len(e) == len(g), qi
        assert [h.chunk.id for h in g] == [h.chunk.id for h in e] or all(
            abs(a.score - b.score) < 2e-6 for a, b in zip(e, g)), qi
        ge = {h.chunk.id: h for h in e}
        for j, h in enumerate(g):
            if h.chunk.id != e[j].chunk.id:  # a swap only between hits whose host scores are within the bar
                assert abs(ge[h.chunk.id].score - e[j].score) < 2e-6, qi
            x = ge[h.chunk.id]
            assert abs(h.score - x.score) <= 2e-6 and h.source == x.source, qi
            assert h.score_breakdown.get("channel") == x.score_breakdown.get("channel"), qi
            graph_hits += int(h.score_breakdown.get("channel") == ["graph"])
    assert graph_hits > 50
    # the columnar form carries the same graph lists
    arr = hr_d.search_batch_arrays(qs, top_k=10, decisions=decisions)
    assert arr["graph_count"][0] == 0 and int(arr["graph_count"].sum()) > 0


def test_captured_step_with_graph_stage_replays_like_eager(tmp_path):
    import torch

    from legal_rag_amd import _native
    from legal_rag_amd.evaluation import synthetic_queries
    hr, chunks = ucc_retriever(tmp_path, "device")
    qs = [q for q, _, _ in synthetic_queries(chunks, seed=0)][:48]
    decisions = [types.SimpleNamespace(mode="GRAPH_AUGMENTED")] * len(qs)
    hr.search_batch(qs, top_k=10, decisions=decisions)  # builds the engine and its graph channel
    eng = hr.native_engine(with_colbert=False)
    assert eng.graph is not None
    store, bm = hr.dense.store, hr.bm25
    dev = torch.device("cuda", 0)
    q_emb = store.embed_device(qs, is_query=True)
    q_graph = store.embed_device(qs, is_query=False)
    qt, qp, _ = bm.term_ids_batch(qs)
    q_terms = torch.from_numpy(np.ascontiguousarray(qt, np.int32)).to(dev)
    q_ptr = torch.from_numpy(np.ascontiguousarray(qp, np.int64)).to(dev)
    params = hr._params(hr._knobs(), float(hr.cfg.retrieval.min_final_score))
    eff, seed_n = 10, int(hr.cfg.retrieval.graph_seed_k)
    graph, res = eng.capture(params, eff, q_emb=q_emb, q_terms=q_terms, q_ptr=q_ptr,
                             graph=dict(q_emb=q_graph, k=eff, seed_n=seed_n))
    before = _native.workspace_growths()
    r = eng.search_batch(params, eff, q_emb=q_emb, q_terms=q_terms, q_ptr=q_ptr)
    ge = eng.graph_topk(r.ids, r.count, q_graph, eff, seed_n)
    eager = {n: v.clone() for n, v in ge.items()}
    torch.cuda.synchronize()
    assert _native.workspace_growths() == before
    for n in eager:
        res.graph[n].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _native.workspace_growths() == before
    for n, v in eager.items():
        assert torch.equal(res.graph[n], v), n
    assert int(eager["count"].sum()) > 0

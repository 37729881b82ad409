"""tests/graph_adversary.py on the CPU: walk_oracle against LawGraphStore.walk, score_oracle against the reference's
search vectors, and the case lists of tests/test_graph_adversary_gpu.py against what they claim to contain."""
import random

import numpy as np
import pytest

import graph_adversary as GA
from test_graph import G, make_cfg, node_view, store_chunks


def store_tables(gs, chunks=()):
    from legal_rag_amd.retrieval.graph_retriever import build_graph_tables
    t = build_graph_tables(gs, list(chunks))
    t.n_rel = max(1, len(t.rel_names))  # GraphTables carries neither of these two
    t.row_norm = np.ones(len(t.row_node), np.float32)
    GA.check_tables(t)
    return t


def store_params(t, cfg, relation_max_depth=None, rel_types=None, min_conf=0.0, limit=80):
    """The parameters of one LawGraphStore.walk call, resolved as walk() resolves its arguments (walk_params of
    tests/test_graph_device_gpu.py, as a dict)."""
    from legal_rag_amd.retrieval.graph_retriever import _depth_bound
    rcfg = cfg.retrieval
    rmd = relation_max_depth if relation_max_depth is not None else (getattr(rcfg, "graph_walk_depths", None)
                                                                     or {"default": 2})
    if rel_types is None:
        rel_types = getattr(rcfg, "graph_rel_types", None)
    dd = rmd.get("default", 2)
    allowed = {str(r) for r in rel_types} if rel_types else None
    limit = max(1, int(limit))
    return GA.make_params(limit, default_depth=_depth_bound(dd), min_conf=float(min_conf or 0.0),
                          rel_max_depth=[_depth_bound(rmd.get(r, dd)) for r in t.rel_names] or [0],
                          rel_allowed=[1 if allowed is None or r in allowed else 0 for r in t.rel_names] or [0],
                          rel_weight=np.ones(t.n_rel), decay=np.ones(limit + 1))


def oracle_views(gs, t, starts, **args):
    from legal_rag_amd.retrieval.graph_store import _clean
    idx = {a: i for i, a in enumerate(t.names)}
    seeds = [idx[_clean(x)] for x in starts if _clean(x) and _clean(x) in idx]
    views = []
    for node, depth, parent, e in GA.walk_oracle(t, seeds, store_params(t, gs.cfg, **args), True):
        meta = gs.nodes[t.names[node]].meta or {}
        ev = bool(t.evidence[e])
        views.append({"article_id": t.names[node], "graph_depth": depth, "graph_parent": t.names[parent],
                      "relations": [t.rel_names[int(t.edge_rel[e])]],
                      "edge_conf": float(t.conf_raw[e]) if ev else meta.get("_edge_conf"),
                      "has_evidence": ev or "_edge_evidence" in meta})
    return views


@pytest.mark.parametrize("case", G["walk"], ids=[f"walk{i}" for i in range(len(G["walk"]))])
def test_walk_oracle_matches_reference_vectors(case):
    from legal_rag_amd.retrieval.graph_store import LawGraphStore
    gs = LawGraphStore(make_cfg())
    t = store_tables(gs)
    a = dict(case["args"])
    starts = a.pop("start_ids")
    assert oracle_views(gs, t, starts, **a) == case["nodes"]


def test_walk_oracle_equals_host_walk_on_random_graphs(tmp_path):
    from legal_rag_amd.retrieval.graph_store import LawGraphStore
    rng = random.Random(7)
    checked = cut = deep = 0
    for gi in range(200):
        n = rng.choice([3, 10, 40, 200, 1500])
        path = tmp_path / f"g{gi}.jsonl"
        GA.random_graph(rng, n, path)
        cfg = make_cfg()
        cfg.paths.law_graph_jsonl = str(path)
        gs = LawGraphStore(cfg)
        gs.load()
        t = store_tables(gs)
        for _ in range(3):
            args = {"limit": rng.choice([0, 1, 2, 5, 17, 80, 800, 4096]),
                    "relation_max_depth": rng.choice([None, {"default": 0}, {"default": 1}, {"default": 3, "next": 1},
                                                      {"default": 2, "cite": 4, "x": 0}, {"default": 6}]),
                    "rel_types": rng.choice([None, None, ["cite", "next", "neighbor"], ["x"]]),
                    "min_conf": rng.choice([0.0, 0.0, 0.5, 0.8])}
            for _q in range(4):
                starts = [rng.choice([str(rng.randrange(n)), f" {rng.randrange(n)} ", "absent0", "nope"])
                          for _ in range(rng.choice([1, 2, 5, 30]))]
                exp = [node_view(x) for x in gs.walk(starts, **args)]
                assert oracle_views(gs, t, starts, **args) == exp, (gi, n, args, starts)
                checked += 1
                cut += int(len(exp) == max(1, args["limit"]) and len(exp) > 1)
                deep += int(any(v["graph_depth"] >= 3 for v in exp))
    assert checked >= 2400 and cut > 20 and deep > 20


def test_score_oracle_reproduces_the_reference_search_vectors():
    from legal_rag_amd.retrieval.graph_retriever import graph_call_params
    from legal_rag_amd.retrieval.graph_store import LawGraphStore
    chunks = store_chunks()
    vec = {c["text"]: np.array(c["vec"], np.float32) for c in G["store"]["chunks"]}
    X = np.stack([vec[c.text] for c in chunks]).astype(np.float32)
    q = np.array(G["store"]["q"], np.float32)
    tol = 2e-6
    hits = 0
    for case in G["search"]:
        a = case["args"]
        cfg = make_cfg(**a["retrieval"])
        gs = LawGraphStore(cfg)
        t = store_tables(gs, chunks)
        t.row_norm = np.linalg.norm(X, axis=1).astype(np.float32)
        p = graph_call_params(cfg.retrieval, t.rel_names, a["top_k"])
        p["lang"] = -1 if not a["lang"] else (t.lang_names.index(a["lang"]) if a["lang"] in t.lang_names else len(t.lang_names))
        rows = [max(r for r, c in enumerate(chunks) if c.article_id == i) for i in a["seed_ids"]]
        found = GA.walk_oracle(t, rows, p, False)
        k = max(1, int(a["top_k"]))
        out = GA.score_oracle(t, X, q, found, p, k, len(chunks))
        exp = case["hits"]
        assert out["count"] == len(exp), a
        assert [chunks[r].article_id for r in out["rows"][:out["count"]]] == [e["article_id"] for e in exp], a
        for j, e in enumerate(exp):
            eb = e["score_breakdown"]
            assert int(out["depth"][j]) == eb["graph_depth"] and [t.rel_names[out["relation"][j]]] == eb["relations"]
            assert float(out["edge_conf"][j]) == eb["edge_conf"]
            assert float(p["decay"][out["depth"][j]]) == eb["depth_decay"]
            assert float(p["rel_weight"][out["relation"][j]]) == eb["relation_weight"]
            assert abs(float(out["semantic"][j]) - eb["semantic"]) <= tol and abs(float(out["final"][j]) - eb["final"]) <= tol
            hits += 1
        assert np.all(out["rows"][out["count"]:] == -1) and np.all(out["final"][out["count"]:] == 0.0)
    assert hits > 10


def test_rank_order_rule():
    nan, inf = float("nan"), float("inf")
    f = np.array([1.0, nan, -inf, 0.0, inf, -0.0, nan, 1.0])
    assert GA.rank_order(f).tolist() == [4, 0, 7, 3, 5, 2, 1, 6]


# ---------------------------------------------------------------------------------------------------------------------
# the case lists really contain what the GPU file says it runs

@pytest.fixture(scope="module")
def world():
    return GA.score_world(252)


@pytest.fixture(scope="module")
def world_expected(world):
    return {c.name: GA.case_expected(world, c) for c in world.cases}


def test_score_cases_reach_every_found_count(world, world_expected):
    _exp, walks, scored = world_expected["F"]
    assert tuple(len(f) for f in walks) == GA.F_GRID
    assert {0, 1, 511, 512, 513, 4096} <= set(GA.F_GRID)
    for k in GA.K_GRID:
        assert {max(0, k - 1), k, k + 1} <= set(GA.F_GRID)
    # rows dropped for each of the three reasons, and valid counts on both sides of k and of F
    t = world.t
    no_row = past = 0
    for f in walks:
        rows = t.node_row[[x[0] for x in f]] if f else np.zeros(0, np.int64)
        no_row += int((rows < 0).sum())
        past += int((rows >= world.n_dense).sum())
    assert no_row > 100 and past > 5
    valid = [len(s[0]) for s in scored]
    assert sum(v < len(f) for v, f in zip(valid, walks)) >= 10
    for c in world.cases[1:]:
        L = c.params["limit"]
        _e, walks, scored = world_expected[c.name]
        assert len(walks[0]) == L, c.name  # F reaches the limit
        if L >= 511:  # several depths (decay values) in one list: query 0 from the limit 4095 on, query 1 throughout
            assert len({x[1] for x in walks[1]}) >= 2 and (L < 4095 or len({x[1] for x in walks[0]}) >= 3), c.name
        if c.params["lang"] >= 0:
            f = walks[0]
            rows = t.node_row[[x[0] for x in f]]
            ok = (rows >= 0) & (rows < world.n_dense)
            assert int((t.row_lang[rows[ok]] != c.params["lang"]).sum()) > 0, c.name
    assert sum(c.params["lang"] >= 0 for c in world.cases) == 2
    # odd F: the two-rows-per-iteration pairing with a lone last row
    assert sum(len(f) % 2 for c in world.cases for f in world_expected[c.name][1]) >= 8


def test_score_cases_hold_ties_inside_and_across_the_cut(world, world_expected):
    inside = straddle = near = neg = zero = cases = 0
    for c in world.cases:
        exp, walks, scored = world_expected[c.name]
        for (order, _row, _sem, final), f in zip(scored, walks):
            fo = final[order]
            for k in GA.K_GRID:
                cases += 1
                inside += int(np.any(fo[:k][1:] == fo[:k][:-1]) and fo[0] != fo[min(k, len(fo)) - 1]) if len(fo) > 1 else 0
                straddle += int(len(fo) > k and fo[k - 1] == fo[k])
            d = np.diff(fo)
            near += int(np.any((d != 0) & (np.abs(d) <= 4e-16 * np.abs(fo[:-1]))))
            neg += int(np.any(fo < 0))
            zero += int(np.any(fo == 0))
    # a family may not silently degenerate: at least a quarter of the (query, k) pairs tie across position k, etc.
    assert cases == len(GA.K_GRID) * sum(len(c.seed_count) for c in world.cases)
    assert inside >= cases // 4, (inside, cases)
    assert straddle >= cases // 8, (straddle, cases)
    assert near >= 5 and neg >= 20 and zero >= 20, (near, neg, zero)
    # fewer than 5 % of the queries have fewer than 2 found nodes beyond those of the F grid that are meant to
    few = sum(len(f) < 2 for c in world.cases[1:] if c.params["limit"] > 1 for f in world_expected[c.name][1])
    assert few == 0  # limit 1 finds one node per query by construction; no other limit case may


def test_score_case_inputs_are_exact():
    for d in GA.D_GRID:
        rng = np.random.default_rng(d)
        X, Q = GA.exact_rows(rng, 50, d), GA.exact_queries(rng, 40, d)
        assert np.all(X == np.rint(X)) and np.abs(X).max() <= 8
        qq = (Q.astype(np.float64) ** 2).sum(1)
        assert np.all(np.isin(Q, (-1.0, 0.0, 1.0))) and np.all(np.sqrt(qq) == np.rint(np.sqrt(qq))) and np.all(qq >= 1)
        assert np.all(Q[:, -1] != 0)  # the last float4 piece of a row takes part (d = 252, 260: a partial last pass)


def test_walk_cases_cut_inside_a_hub_list_and_run_wide_frontiers():
    t = GA.hub_tables()
    e0, e1 = int(t.node_ptr[GA.HUB]), int(t.node_ptr[1])
    big = {c.name: c for c in GA.hub_cases(t)}
    full = GA.walk_oracle(t, [GA.HUB], big["hub-limit-4096"].params, True)
    assert len(full) == 4096
    cut_at, cut_late = set(), 0
    for L in (63, 64, 65):
        c = big[f"hub-limit-{L}"]
        f = GA.walk_oracle(t, c.seeds[0], c.params, True)
        assert len(f) == L and all(x[2] == GA.HUB for x in f)
        cut_at.add(f[-1][3] - e0 + 1)      # the list position after which the walk was cut
        f1 = GA.walk_oracle(t, c.seeds[1], c.params, True)
        assert len(f1) == L
        cut_late += int(f1[-1][3] - e1 + 1 > L)
    assert cut_at == {63, 64, 65} and cut_late == 3
    # the hub's degree exceeds every limit, and its list holds repeats and ids that are no stored node
    lst = t.edge_dst[e0:e0 + GA.HUB_DEG]
    assert GA.HUB_DEG > GA.MAX_LIMIT and len(set(lst.tolist())) < GA.HUB_DEG - 500 and int((t.present[lst] == 0).sum()) > 50
    # min_conf 0.5 removes exactly the first 64 entries
    c = big["hub-min-conf"]
    f = GA.walk_oracle(t, c.seeds[0], c.params, True)
    assert f[0][3] - e0 == 64 and len(f) > 3000 and all(x[2] == GA.HUB for x in f)
    assert GA.walk_oracle(t, [GA.HUB], big["hub-depth-0"].params, True) == []
    c = big["hub-relations-stop"]
    f = GA.walk_oracle(t, c.seeds[0], c.params, True)
    assert f and all(int(t.edge_rel[x[3]]) != 2 for x in f) and max(x[1] for x in f) >= 2
    # the fan-out: a level of more than 256 frontier entries, all of which expand
    ft = GA.fanout_tables()
    c = GA.fanout_case(ft)
    f = GA.walk_oracle(ft, c.seeds[0], c.params, True)
    per_level = [sum(x[1] == d for x in f) for d in (1, 2, 3)]
    assert per_level == [20, 400, 1200]
    assert len({x[2] for x in f if x[1] == 3}) == 400


def test_walk_cases_at_the_lds_boundary():
    t, t1 = GA.lds_boundary_tables()
    assert t.n_nodes == GA.LDS_NODES and t1.n_nodes == GA.LDS_NODES + 1
    c = GA.lds_boundary_case(t)
    assert c.params["limit"] == 4096 and len(c.seeds[0]) == 1024 and len(set(c.seeds[1])) < 100
    # the largest LDS launch of the walk: (2 * max(seed_n, limit) + seed_n + n_nodes) * 4 bytes
    assert (2 * max(1024, 4096) + 1024 + t.n_nodes) * 4 == 86016
    walks = [GA.walk_oracle(t, s, c.params, True) for s in c.seeds]
    assert [len(f) for f in walks][:2] == [4096, 4096] and 0 < len(walks[2])
    assert max(x[1] for x in walks[1]) >= 4
    # the appended id changes no walk
    assert walks == [GA.walk_oracle(t1, s, c.params, True) for s in c.seeds]
    m = GA.many_queries_case(t1, 11)
    lens = [len(GA.walk_oracle(t1, s, m.params, True)) for s in m.seeds]
    assert len(lens) == 300 and sum(x == 64 for x in lens) > 30 and sum(x < 2 for x in lens) < 15  # fewer than 5 %

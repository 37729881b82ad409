"""Graph channel on the device, host side: the tables amdr_graph_create takes, built from the graph fixture and the
store's chunks (retrieval/graph_retriever.py build_graph_tables), the per-call parameters, and the graph_channel knob.
No GPU needed."""
import copy

import pytest

from test_graph import G, make_cfg, store_chunks


def tables(chunks=None):
    from legal_rag_amd.retrieval.graph_retriever import build_graph_tables
    from legal_rag_amd.retrieval.graph_store import LawGraphStore
    gs = LawGraphStore(make_cfg())
    return gs, build_graph_tables(gs, store_chunks() if chunks is None else chunks)


def test_tables_intern_nodes_absent_destinations_and_follow_the_csr():
    gs, t = tables()
    assert t.names[:len(gs.nodes)] == list(gs.nodes)
    absent = [n for n in t.names if n not in gs.nodes]
    # destinations that are no stored node are interned (they are "seen" by the walk) but not present
    dsts = {d for es in gs.adj.values() for d, _r, _c, _e in es}
    assert set(absent) <= dsts and absent
    assert all(t.present[t.names.index(a)] == 0 for a in absent)
    assert int(t.present.sum()) == len(gs.nodes) == G["n_nodes"]
    assert int(t.node_ptr[-1]) == G["n_edges"]
    for i, aid in enumerate(t.names):
        es = gs.adj.get(aid, []) if aid in gs.nodes else []
        lo, hi = int(t.node_ptr[i]), int(t.node_ptr[i + 1])
        assert [t.names[d] for d in t.edge_dst[lo:hi]] == [e[0] for e in es]
        assert [t.rel_names[r] for r in t.edge_rel[lo:hi]] == [e[1] for e in es]
        assert list(t.conf_raw[lo:hi]) == [e[2] for e in es]
        assert list(t.evidence[lo:hi]) == [1 if e[3] else 0 for e in es]


def test_evidence_less_edges_take_the_stored_nodes_edge_conf():
    from legal_rag_amd.retrieval.graph_retriever import build_graph_tables
    from legal_rag_amd.retrieval.graph_store import LawGraphStore
    gs = LawGraphStore(make_cfg())
    gs.load()
    # give two stored nodes an _edge_conf of their own: an edge without evidence into them scores with it
    gs.nodes["1"].meta = dict(gs.nodes["1"].meta or {}, _edge_conf=0.25)
    gs.nodes["2"].meta = dict(gs.nodes["2"].meta or {}, _edge_conf=0)  # falsy -> 1.0
    t = build_graph_tables(gs, store_chunks())
    seen = 0
    for i, aid in enumerate(t.names):
        for e in range(int(t.node_ptr[i]), int(t.node_ptr[i + 1])):
            dst = t.names[t.edge_dst[e]]
            if t.evidence[e]:
                assert t.conf_eff[e] == t.conf_raw[e]
            elif dst == "1":
                assert t.conf_eff[e] == 0.25
                seen += 1
            elif dst in gs.nodes:
                assert t.conf_eff[e] == 1.0
    assert seen > 0


def test_node_row_last_chunk_wins_and_stripped_seed_keys():
    from legal_rag_amd.schemas import LawChunk
    chunks = store_chunks()
    extra = [
        # a second chunk of article "7": the LAST one wins (_bind_rows)
        LawChunk(id="dup.txt::7", law_name="Synthetic Code", article_no="7", article_id="7", text="second copy of 7",
                 lang="en", source="dup.txt"),
        # a padded key: its row seeds the walk from the stripped id, but the node's row stays the exact key's
        LawChunk(id="pad.txt::9", law_name="Synthetic Code", article_no="9", article_id=" 9 ", text="padded 9",
                 lang="zh", source="pad.txt"),
        # an article id nowhere in the graph: interned (a seed without edges)
        LawChunk(id="new.txt::zz", law_name="Synthetic Code", article_no="zz", article_id="zz", text="x", lang="zh",
                 source="new.txt"),
        # empty text: no row for its node
        LawChunk(id="empty.txt::12", law_name="Synthetic Code", article_no="12", article_id="12", text="   ", lang="zh",
                 source="empty.txt"),
    ]
    all_chunks = chunks + extra
    gs, t = tables(all_chunks)
    n0 = len(chunks)
    idx = {a: i for i, a in enumerate(t.names)}
    assert t.node_row[idx["7"]] == n0
    assert t.row_node[n0 + 1] == idx["9"] and t.node_row[idx["9"]] == [i for i, c in enumerate(chunks)
                                                                          if c.article_id == "9"][-1]
    assert "zz" in idx and t.present[idx["zz"]] == 0 and t.row_node[n0 + 2] == idx["zz"]
    assert t.node_row[idx["12"]] == -1
    assert all(t.row_node[r] == idx[c.article_id] for r, c in enumerate(chunks))
    assert t.lang_names[t.row_lang[n0]] == "en"


def test_call_params_follow_the_host_resolution():
    from legal_rag_amd.retrieval.graph_retriever import _depth_decay, _relation_weight, graph_call_params
    _gs, t = tables()
    cfg = make_cfg(graph_limit=0, graph_rel_types=["cite", "next"], graph_min_conf=0.5, graph_depth_gamma=1.3,
                   graph_walk_depths={"default": 3, "next": 1.5})
    p = graph_call_params(cfg.retrieval, t.rel_names, 10)
    assert p["limit"] == 1 and p["default_depth"] == 3 and p["min_conf"] == 0.5
    for r, name in enumerate(t.rel_names):
        assert p["rel_allowed"][r] == (name in ("cite", "next"))
        assert p["rel_max_depth"][r] == {"next": 2}.get(name, 3)
        assert p["rel_weight"][r] == _relation_weight([name])
    assert list(p["decay"]) == [_depth_decay(d, gamma=1.3) for d in range(2)]


def test_graph_channel_is_validated():
    from legal_rag_amd.config import AppConfig, RetrievalConfig, graph_channel_mode
    assert RetrievalConfig().graph_channel == "host"
    assert graph_channel_mode(AppConfig()) == "host"
    assert graph_channel_mode(RetrievalConfig(graph_channel="device")) == "device"
    with pytest.raises(ValueError, match="graph_channel"):
        RetrievalConfig(graph_channel="gpu")
    cfg = AppConfig()
    cfg.retrieval = copy.copy(cfg.retrieval)
    cfg.retrieval.graph_channel = "Device"
    with pytest.raises(ValueError, match="graph_channel"):
        graph_channel_mode(cfg)


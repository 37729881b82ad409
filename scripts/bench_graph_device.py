"""Graph channel on the device (csrc/graph.hip) against the host path, on the UCC-en fixture.

All UCC-en synthetic bench questions over a seeded synthetic law graph on the UCC chunk ids (prev/next chains plus
random cite / defined_by edges, some with evidence), graph_seed_k = 30, graph_limit = 800.  Prints ONE JSON line:
  graph_stage_ms        device graph stage (amdr_graph_search_device: walk + score + select) per batch, HIP events
  host_ms_per_query     GraphRetriever.search (host walk + one score_rows call) per query, on a 64-query sample
  arrays_qps            search_batch_arrays with every query in graph mode (fused channels + graph stage + copies)

    python scripts/bench_graph_device.py [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import random
import sys
import tempfile
import time
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def ucc_graph(chunks, path, seed=11):
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch

    from legal_rag_amd.config import AppConfig
    from legal_rag_amd.evaluation import synthetic_queries
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever

    tmp = Path(tempfile.mkdtemp(prefix="bench_graph_"))
    cfg = AppConfig.for_data_dir(str(tmp), "zh").with_lang("en")
    r = cfg.retrieval
    r.encoder_backend = "hashing"
    r.enable_colbert = r.enable_rerank = False
    r.enable_graph = True
    r.graph_seed_k, r.graph_limit = 30, 800
    r.graph_channel = "device"
    chunks = load_chunks_from_dir(str(ROOT / "tests" / "golden" / "corpus"), "law_en.jsonl")
    build_faiss_index(cfg, chunks)
    build_bm25_index(cfg, chunks)
    ucc_graph(chunks, tmp / "graph.jsonl")
    cfg.paths.law_graph_jsonl = str(tmp / "graph.jsonl")
    hr = HybridRetriever(cfg)
    qs = [q for q, _, _ in synthetic_queries(chunks, seed=0)]
    dec = [types.SimpleNamespace(mode="GRAPH_AUGMENTED")] * len(qs)
    top_k = 10

    # search_batch_arrays, every query in graph mode
    hr.search_batch_arrays(qs, top_k=top_k, decisions=dec)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        out = hr.search_batch_arrays(qs, top_k=top_k, decisions=dec)
    arrays_s = (time.perf_counter() - t0) / args.reps

    # the device graph stage alone, on the engine's last fused result
    eng = hr.native_engine(with_colbert=False)
    store = hr.dense.store
    q_graph = store.embed_device(qs, is_query=False)
    q_emb = store.embed_device(qs, is_query=True)
    qt, qp, _ = hr.bm25.term_ids_batch(qs)
    dev = torch.device("cuda", 0)
    res = eng.search_batch(hr._params(hr._knobs(), float(r.min_final_score)), hr._eff_depth(top_k, "bench"),
                           q_emb=q_emb, q_terms=torch.from_numpy(np.ascontiguousarray(qt, np.int32)).to(dev),
                           q_ptr=torch.from_numpy(np.ascontiguousarray(qp, np.int64)).to(dev))
    eff = hr._eff_depth(top_k, "bench")
    eng.graph_topk(res.ids, res.count, q_graph, eff, r.graph_seed_k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        g = eng.graph_topk(res.ids, res.count, q_graph, eff, r.graph_seed_k)
    e1.record()
    torch.cuda.synchronize()
    stage_ms = e0.elapsed_time(e1) / args.reps
    found = int(g["count"].sum())

    # the host path per query (walk + one score_rows call + sort), seeds = the same fused lists
    hcfg = cfg
    hcfg.retrieval.graph_channel = "host"
    sample = qs[:: max(1, len(qs) // 64)][:64]
    fused = hr.search_batch(sample, top_k=30)  # no decisions: the first 30 fused hits are the seeds
    hr.search_graph(sample[0], eff, seeds=fused[0][:30])
    t0 = time.perf_counter()
    for q, f in zip(sample, fused):
        hr.search_graph(q, eff, seeds=f[:30])
    host_ms = (time.perf_counter() - t0) / len(sample) * 1e3

    print(json.dumps({"bench": "graph_device", "queries": len(qs), "graph_seed_k": r.graph_seed_k,
                      "graph_limit": r.graph_limit, "graph_nodes": len(chunks), "graph_stage_ms": round(stage_ms, 4),
                      "graph_hits": found, "host_ms_per_query": round(host_ms, 3), "host_sample": len(sample),
                      "arrays_qps": round(len(qs) / arrays_s, 1),
                      "arrays_graph_count": int(out["graph_count"].sum())}))


if __name__ == "__main__":
    main()

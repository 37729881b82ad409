"""The scoped step against the unscoped one on the UCC-en fixture (591 chunks, d = 768, dense + BM25, k = 10), in one
process: (1) the scoped serving step — 1 query, a 28-row section — as the one launch of scope_hybrid_kernel ("scoped")
and with AMDR_SCOPE_FUSED=0, the separate launches of the same library ("scoped_unfused"); (2) the unscoped one-launch
serving step; (3) the scoped batch of 1 168 queries, each with the section scope of the chunk it was cut from, both
forms again (its scopes reach 591 rows — the chunks without a section take their whole law — so both forms run the
separate launches), and the same batch cut from chunks that have a section only (every scope inside one slab: the one
launch); (4) the unscoped batch.  Then the two scoped forms once more with a ColBERT channel (a stand-in store of
32 random unit token vectors per chunk: scope_maxsim_kernel runs first, the step is two launches against four).
Per form: eager p50 of HybridEngine.search_batch (host call + device, synchronised per call) and the median over 5
windows of the device time of 200 hipGraph replays (events around the window).  `--profile N`: N eager scoped steps of
each size and nothing else (run under `rocprofv3 --kernel-trace --stats` for the three kernels' own times)."""
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from legal_rag_amd import _native, encoders  # noqa: E402
from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir  # noqa: E402
from legal_rag_amd.retrieval.engine import HybridEngine  # noqa: E402
from legal_rag_amd.retrieval.scope import Scope, ScopeResolver  # noqa: E402
from oracle import bm25 as OB  # noqa: E402  (corpus builder only: the timed path is the native one)

K, NQ_BATCH = 10, 1168


def eager_p50(fn, reps=300):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(ts), 1)


def graph_device_us(g, reps=200, windows=5):
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return round(statistics.median(out), 2), round(min(out), 2), round(max(out), 2)


def main():
    profile = int(sys.argv[sys.argv.index("--profile") + 1]) if "--profile" in sys.argv else 0
    dev = torch.device("cuda", 0)
    chunks = load_chunks_from_dir(str(Path(__file__).resolve().parent.parent / "tests" / "golden" / "corpus"), "law_en.jsonl")
    emb = encoders.HashingEmbedder(768)
    X = emb.encode([c.text for c in chunks])
    ob = OB.BM25Okapi([OB.tokenize_en(c.text) for c in chunks])
    csr = OB.to_csr(ob)
    rng = np.random.default_rng(0)
    D = rng.standard_normal((32 * len(chunks), 128)).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    eng = HybridEngine(_native.DenseIndex(X), _native.BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"],
                                                                csr["doc_len"], ob.avgdl, ob.k1, ob.b),
                       _native.MaxSimIndex(D, np.arange(len(chunks) + 1, dtype=np.int64) * 32))
    res = ScopeResolver(chunks)
    sizes = {}
    for c in chunks:
        if c.section:
            sizes[c.section] = sizes.get(c.section, 0) + 1
    sec28 = min(sizes, key=lambda s: (abs(sizes[s] - 28), s))
    src = [chunks[(7 * j) % len(chunks)] for j in range(NQ_BATCH)]
    with_section = [c for c in chunks if c.section]
    src_sec = [with_section[(7 * j) % len(with_section)] for j in range(NQ_BATCH)]
    params = _native.make_fuse_params()
    out = {"section_rows": sizes[sec28]}
    for name, nq, src in (("serving", 1, src), ("batch", NQ_BATCH, src), ("batch_sections", NQ_BATCH, src_sec)):
        texts = [" ".join(c.text.split()[2:21]) for c in src]  # 19 words of the chunk a query was cut from
        scopes = [Scope(section=c.section) if c.section else Scope(law_name=c.law_name) for c in src]
        out[f"{name}_scope_rows_max"] = sizes[sec28] if nq == 1 else int(res.table(scopes)[3])
        Q = torch.from_numpy(emb.encode_queries(texts[:nq])).to(dev)
        qt_h, qp_h = _native.BM25Index.pack_queries([[csr["vocab"].get(t, -1) for t in OB.tokenize_en(x)] for x in texts[:nq]])
        qt, qp = torch.from_numpy(qt_h).to(dev), torch.from_numpy(qp_h).to(dev)
        tb = eng.upload_scopes(*res.table([Scope(section=sec28)] if nq == 1 else scopes[:nq])[:3],
                               channel={"serving": 0, "batch": 1, "batch_sections": 2}[name])  # (one staging ring each)
        eng.reserve(nq, K, int(qp_h[-1]), rows_max=tb[4])
        Qt = rng.standard_normal((nq, 32, 128)).astype(np.float32)
        Qt = torch.from_numpy(Qt / np.linalg.norm(Qt, axis=2, keepdims=True)).to(dev)
        scoped = dict(q_emb=Q, q_terms=qt, q_ptr=qp, scopes=(tb, tb, None))
        scoped_c = dict(q_emb=Q, q_terms=qt, q_ptr=qp, q_tok=Qt, scopes=(tb, tb, tb))
        # (form, AMDR_SCOPE_FUSED, arguments); the variable is read per call, a captured graph keeps the form it recorded.
        # "seq": the one launch with AMDR_SCOPE_OVERLAP=0, all four waves dense, then all four BM25
        forms = {"scoped": ("1", scoped), "scoped_seq": ("seq", scoped), "scoped_unfused": ("0", scoped),
                 "unscoped": ("1", dict(q_emb=Q, q_terms=qt, q_ptr=qp)),
                 "scoped_colbert": ("1", scoped_c), "scoped_colbert_seq": ("seq", scoped_c),
                 "scoped_colbert_unfused": ("0", scoped_c)}
        if profile:
            for _ in range(profile):
                eng.search_batch(params, K, **scoped)
            torch.cuda.synchronize()
            continue
        for form, (fused, kw) in forms.items():
            os.environ["AMDR_SCOPE_FUSED"] = "1" if fused == "seq" else fused
            os.environ["AMDR_SCOPE_OVERLAP"] = "0" if fused == "seq" else "1"
            step = lambda: eng.search_batch(params, K, **kw)  # noqa: E731
            for _ in range(30):
                step()
            torch.cuda.synchronize()
            p50 = eager_p50(step)
            g, _res = eng.capture(params, K, **kw)
            for _ in range(20):
                g.replay()
            torch.cuda.synchronize()
            med, lo, hi = graph_device_us(g)
            out[f"{name}_{form}"] = {"nq": nq, "eager_p50_us": p50, "graph_device_us": med, "graph_windows_min_max_us": [lo, hi]}
        os.environ.pop("AMDR_SCOPE_FUSED", None)
        os.environ.pop("AMDR_SCOPE_OVERLAP", None)
        out[f"{name}_plan"] = eng.scope.plan_info(nq, K, tb[4])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

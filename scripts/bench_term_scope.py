"""amdr_term_scope_device: the event time of its three launches (count, scan, write), beside the host time of the path a
caller had before it for the same tables — set algebra on the host's own copy of the postings, then
HybridEngine.upload_scopes — at two shapes:

  tests    the largest shape of tests/test_term_scope_gpu.py: the 65 constraints of tests/term_scope_cases.py over its
           4 100-document corpus (longest driver 2 444: three tiles a constraint);
  ucc-en   tests/golden/corpus/law_en.jsonl cut by the index's own tokeniser: 1 168 distinct constraints of two MUST terms
           each (pairs of vocabulary tokens that stand in 20 .. 300 articles).

The device figure is the median of --reps timed calls between two events on the stream, after one untimed call; the
operands are resident (their upload is one pinned copy, as the host path's table upload is, and is not timed on either
side).  The host figure is the median wall time of building the same table with numpy (np.intersect1d over the term's
document lists, the arrays a host copy of the postings would hold) plus the wall time of upload_scopes including its
stream synchronise.  Both tables are compared before anything is timed.  Prints ONE JSON line.

    python scripts/bench_term_scope.py [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

T_OPS = ("int64", "int32", "int64", "int32", "int64", "int64", "int32")


def must_pairs_ops(pairs):
    """The operands of one constraint per pair: two MUST groups of one term each, no base."""
    n = len(pairs)
    return (np.arange(0, 2 * n + 1, 2, dtype=np.int64), np.zeros(2 * n, dtype=np.int32), np.arange(2 * n + 1, dtype=np.int64),
            np.asarray(pairs, dtype=np.int32).reshape(-1), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64),
            np.full(n, -1, dtype=np.int32))


def device_ms(torch, nat, gi, ops, cand_max, rows_cap, reps):
    dev = torch.device("cuda", 0)
    n_cons, n_groups, n_base = ops[6].size, ops[1].size, ops[4].size - 1
    t = []
    for a, dt in zip(ops, T_OPS):
        x = torch.zeros(max(a.size, 1), dtype=getattr(torch, dt), device=dev)
        if a.size:
            x[:a.size].copy_(torch.from_numpy(np.ascontiguousarray(a)))
        t.append(x)
    sp = torch.zeros(n_cons + 1, dtype=torch.int64, device=dev)
    rw = torch.zeros(max(rows_cap, 1), dtype=torch.int64, device=dev)
    st = torch.zeros(n_cons, dtype=torch.int32, device=dev)
    wb = nat.term_scope_plan(n_cons, cand_max)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        gi.term_scope_device([x.data_ptr() for x in t], n_base, n_cons, n_groups, cand_max, rows_cap, sp.data_ptr(),
                             rw.data_ptr(), st.data_ptr(), work.data_ptr(), wb, stream)
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    assert not st.cpu().numpy().any()
    ptr = sp.cpu().numpy()
    return ms, ptr, rw.cpu().numpy()[:ptr[-1]], wb


def report(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def host_path(torch, eng, build, reps):
    """(table ms, upload ms, the table): `build()` makes (scope_ptr, rows) on the host."""
    t_build, t_up = [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        ptr, rows = build()
        t1 = time.perf_counter()
        eng.upload_scopes(ptr, rows, np.arange(ptr.size - 1, dtype=np.int32))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_build.append((t1 - t0) * 1e3)
        t_up.append((t2 - t1) * 1e3)
    return t_build[1:], t_up[1:], (ptr, rows)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch

    import term_scope_cases as TC
    from legal_rag_amd import _native as nat
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.retrieval.builders.bm25_builder import tokenize_corpus
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    from legal_rag_amd.retrieval.engine import HybridEngine
    from legal_rag_amd.retrieval.terms import driver_length
    out = {"device": nat.device_name(0), "reps": args.reps}

    # ---- the largest test shape ----
    corpus = TC.corpora()["big"]
    fam = next(f for f in TC.families() if f.name == "65 constraints")
    tp, pd, pt, idf, dl, avgdl = corpus.postings()
    gi = nat.BM25Index(tp, pd, pt, idf, dl, avgdl)
    eng = HybridEngine(None, gi, None)
    df = corpus.df()
    lens = [driver_length(g, df, None, corpus.n_docs) for g, _ in fam.cons]
    ms, ptr, rows, wb = device_ms(torch, nat, gi, TC.operands(fam), max(lens), sum(lens), args.reps)
    lists = [pd[tp[t]:tp[t + 1]].astype(np.int64) for t in range(corpus.n_terms)]
    every = np.arange(corpus.n_docs, dtype=np.int64)

    def sat(ids):
        x = lists[ids[0]]
        for t in ids[1:]:
            x = np.intersect1d(x, lists[t], assume_unique=True)
        return x

    def build_tests():
        parts = []
        for groups, _ in fam.cons:
            x, anys = every, None
            for k, ids in groups:
                if k == TC.MUST:
                    x = np.intersect1d(x, sat(ids), assume_unique=True)
                elif k == TC.ANY:
                    anys = sat(ids) if anys is None else np.union1d(anys, sat(ids))
            if anys is not None:
                x = np.intersect1d(x, anys, assume_unique=True)
            for k, ids in groups:
                if k == TC.NOT:
                    x = np.setdiff1d(x, sat(ids), assume_unique=True)
            parts.append(x)
        p = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([x.size for x in parts], out=p[1:])
        return p, np.concatenate(parts)
    tb, tu, (hp, hr) = host_path(torch, eng, build_tests, args.reps)
    assert np.array_equal(hp, ptr) and np.array_equal(hr, rows)
    out["tests"] = {"constraints": len(fam.cons), "docs": corpus.n_docs, "cand_max": max(lens), "rows": int(ptr[-1]),
                    "work_bytes": wb, "device_three_launches": report(ms), "host_set_algebra": report(tb),
                    "host_upload_scopes": report(tu)}

    # ---- UCC-en, 1 168 distinct two-term constraints ----
    chunks = load_chunks_from_dir(str(ROOT / "tests" / "golden" / "corpus"), "law_en.jsonl")
    docs, _ = tokenize_corpus(chunks)
    model = BM25Okapi(docs)
    tp, pd, pt, idf, dl = model.to_csr()
    gi2 = nat.BM25Index(tp, pd, pt, idf, dl, float(model.avgdl))
    eng2 = HybridEngine(None, gi2, None)
    dfs = np.diff(tp)
    mid = np.flatnonzero((dfs >= 20) & (dfs <= 300))
    rng = np.random.default_rng(0)
    seen = set()
    while len(seen) < 1168:
        a, b = (int(x) for x in rng.choice(mid, size=2, replace=False))
        seen.add((min(a, b), max(a, b)))
    pairs = sorted(seen)
    lens2 = [int(min(dfs[a], dfs[b])) for a, b in pairs]
    ms2, ptr2, rows2, wb2 = device_ms(torch, nat, gi2, must_pairs_ops(pairs), max(lens2), sum(lens2), args.reps)
    lists2 = [pd[tp[t]:tp[t + 1]].astype(np.int64) for t in range(len(dfs))]

    def build_ucc():
        parts = [np.intersect1d(lists2[a], lists2[b], assume_unique=True) for a, b in pairs]
        p = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([x.size for x in parts], out=p[1:])
        return p, np.concatenate(parts)
    tb2, tu2, (hp2, hr2) = host_path(torch, eng2, build_ucc, args.reps)
    assert np.array_equal(hp2, ptr2) and np.array_equal(hr2, rows2)
    out["ucc_en"] = {"constraints": len(pairs), "docs": len(docs), "terms": int(len(dfs)), "cand_max": max(lens2),
                     "rows": int(ptr2[-1]), "work_bytes": wb2, "device_three_launches": report(ms2),
                     "host_set_algebra": report(tb2), "host_upload_scopes": report(tu2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

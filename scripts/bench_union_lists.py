"""amdr_union_lists_device: the event time of the union step's three launches (count, scan, write) next to the span step's
(amdr_span_lists_device) TAKEN IN THE SAME PROCESS, at these shapes:

  ucc-en   tests/golden/corpus/law_en.jsonl cut by the index's own tokeniser: 64 distinct prefixes (stems of three to five
           letters that name 2 to 64 vocabulary tokens each, each expansion once) as union items; beside them 64 two-token
           unordered Nears at distance 5 through the span step;
  tiles    the largest shape of tests/test_union_lists_gpu.py: 65 items over 3 x 32 768 + 1 documents (four tiles).

Method: the operands are resident; every step runs once untimed; then --windows windows per step, ALTERNATING between the
two steps, each window --calls back-to-back calls between two events on the stream; the figure of a window is its time per
call, the reported figure the median over the windows (min and max beside it).  Lists are compared with a numpy union
before anything is timed.  Prints ONE JSON line.

    python scripts/bench_union_lists.py [--windows 9] [--calls 50]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))

from bench_phrase_scope import dev_arr, report  # noqa: E402


def window_ms(torch, call, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(torch, steps, windows, calls):
    """{name: [ms per call of each window]} of the steps, one window of each after the other, `windows` times."""
    for call in steps.values():
        call()
    torch.cuda.synchronize()
    out = {name: [] for name in steps}
    for _ in range(windows):
        for name, call in steps.items():
            out[name].append(window_ms(torch, call, calls))
    return out


def union_step(torch, nat, gi, items, rows_cap):
    """(call, read) of the union step over `items` (lists of term ids): read() -> (list_ptr, docs, status)."""
    dev = torch.device("cuda", 0)
    n = len(items)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(it) for it in items], out=ptr[1:])
    ip = dev_arr(torch, ptr, "int64")
    it = dev_arr(torch, np.asarray([t for x in items for t in x], dtype=np.int32), "int32")
    lp = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    dc = torch.zeros(max(rows_cap, 1), dtype=torch.int32, device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    wb = nat.union_lists_plan(n, gi.n_docs)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        gi.union_lists_device(ip.data_ptr(), it.data_ptr(), n, 0, rows_cap, lp.data_ptr(), dc.data_ptr(), st.data_ptr(),
                              work.data_ptr(), wb, stream)

    def read():
        torch.cuda.synchronize()
        p = lp.cpu().numpy()
        return p, dc.cpu().numpy()[:p[-1]], st.cpu().numpy()
    return call, read, wb


def span_step(torch, nat, gi, pairs, dist, bound):
    """(call, read) of the span step over two-token unordered Nears."""
    dev = torch.device("cuda", 0)
    n = len(pairs)
    ops = (np.arange(0, 2 * n + 1, 2, dtype=np.int64), np.asarray(pairs, dtype=np.int32).ravel(),
           np.full(n, 1, dtype=np.int32), np.full(n, dist, dtype=np.int32))
    t = [dev_arr(torch, a, dt) for a, dt in zip(ops, ("int64", "int32", "int32", "int32"))]
    cand_max, rows_cap = int(max(bound)), int(sum(bound))
    lp = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    dc = torch.zeros(max(rows_cap, 1), dtype=torch.int32, device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    wb = nat.span_lists_plan(n, cand_max)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        gi.span_lists_device(*[x.data_ptr() for x in t], n, cand_max, rows_cap, lp.data_ptr(), dc.data_ptr(), st.data_ptr(),
                             work.data_ptr(), wb, stream)

    def read():
        torch.cuda.synchronize()
        p = lp.cpu().numpy()
        return p, dc.cpu().numpy()[:p[-1]], st.cpu().numpy()
    return call, read, wb


def numpy_unions(term_ptr, post_doc, items):
    parts = [np.unique(np.concatenate([post_doc[term_ptr[t]:term_ptr[t + 1]] for t in it] + [np.zeros(0, np.int32)]))
             for it in items]
    p = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([x.size for x in parts], out=p[1:])
    return p, np.concatenate(parts).astype(np.int32)


def pick_prefixes(vocab, count):
    """`count` stems of 3 to 5 letters naming 2 to 64 tokens, each expansion once, in stem order."""
    words = sorted(vocab)
    seen, out = set(), []
    for L in (4, 5, 3):
        for stem in sorted({w[:L] for w in words if len(w) >= L and w.isalpha()}):
            ids = tuple(sorted(vocab[w] for w in words if w.startswith(stem)))
            if 2 <= len(ids) <= 64 and ids not in seen:
                seen.add(ids)
                out.append((stem, list(ids)))
    pick = np.sort(np.random.default_rng(0).choice(len(out), size=count, replace=False))
    return [out[i] for i in pick]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    import torch

    import union_cases as UC
    from legal_rag_amd import _native as nat
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.retrieval.builders.bm25_builder import tokenize_corpus
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    out = {"device": nat.device_name(0), "windows": args.windows, "calls_per_window": args.calls}

    # ---- UCC-en: 64 distinct prefixes beside 64 two-token Nears ----
    chunks = load_chunks_from_dir(str(ROOT / "tests" / "golden" / "corpus"), "law_en.jsonl")
    tdocs, _ = tokenize_corpus(chunks)
    model = BM25Okapi(tdocs)
    tp, pd, pt, idf, dl = model.to_csr()
    gi = nat.BM25Index(tp, pd, pt, idf, dl, float(model.avgdl))
    doc_ptr, tokens = model.token_stream(tdocs)
    gi.set_tokens(doc_ptr, tokens)
    dfs = np.diff(tp)
    n_docs = int(doc_ptr.size - 1)
    prefixes = pick_prefixes(model.vocab(), 64)
    items = [ids for _, ids in prefixes]
    ub = [min(n_docs, int(sum(dfs[t] for t in ids))) for ids in items]
    u_call, u_read, u_wb = union_step(torch, nat, gi, items, sum(ub))
    inside = np.ones(tokens.size - 1, dtype=bool)
    cut = doc_ptr[1:-1]
    inside[cut[(cut > 0) & (cut < tokens.size)] - 1] = False
    a, b = tokens[:-1][inside], tokens[1:][inside]
    ok = (dfs[a] >= 20) & (dfs[a] <= 300) & (dfs[b] >= 20) & (dfs[b] <= 300) & (a != b)
    pairs = np.unique(np.stack([a[ok], b[ok]], axis=1), axis=0)
    pairs = [(int(x), int(y)) for x, y in pairs[np.sort(np.random.default_rng(0).choice(pairs.shape[0], size=64, replace=False))]]
    bound = [int(min(dfs[x], dfs[y])) for x, y in pairs]
    s_call, s_read, s_wb = span_step(torch, nat, gi, pairs, 5, bound)
    u_call(), s_call()
    ptr, docs, status = u_read()
    want_ptr, want_docs = numpy_unions(tp, pd, items)
    assert not status.any() and np.array_equal(ptr, want_ptr) and np.array_equal(docs, want_docs)
    assert not s_read()[2].any()
    ms = alternate(torch, {"union": u_call, "span": s_call}, args.windows, args.calls)
    out["ucc_en"] = {"docs": n_docs, "terms": int(dfs.size), "prefixes": len(items), "stems": [s for s, _ in prefixes][:8],
                     "expanded_terms": int(sum(len(x) for x in items)), "union_rows": int(ptr[-1]), "union_rows_cap": sum(ub),
                     "union_work_bytes": u_wb, "union_step_three_launches": report(ms["union"]),
                     "nears": len(pairs), "near_distance": 5, "span_rows": int(s_read()[0][-1]), "span_work_bytes": s_wb,
                     "span_step_three_launches": report(ms["span"])}

    # ---- four tiles: the largest test shape ----
    T = nat.UNION_TILE
    corpus = UC.edge_corpus(3 * T + 1, T)
    tp2, pd2, pt2, idf2, dl2, avgdl2 = corpus.postings()
    gi2 = nat.BM25Index(tp2, pd2, pt2, idf2, dl2, avgdl2)
    batch = UC.batch(corpus, 65)
    cap = UC.rows_cap(corpus, batch)
    t_call, t_read, t_wb = union_step(torch, nat, gi2, batch, cap)
    t_call()
    ptr, docs, status = t_read()
    want_ptr, want_docs = UC.expected_lists(corpus, batch)
    assert not status.any() and np.array_equal(ptr, want_ptr) and np.array_equal(docs, want_docs)
    ms = alternate(torch, {"union": t_call}, args.windows, args.calls)
    out["tiles"] = {"docs": corpus.n_docs, "items": len(batch), "cells": len(batch) * 4, "rows": int(ptr[-1]), "work_bytes": t_wb,
                    "union_step_three_launches": report(ms["union"])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

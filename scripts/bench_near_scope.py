"""amdr_span_lists_device: the event time of the span step's three launches (count, scan, write) over Nears, beside the
phrase step on the same token pairs (scripts/bench_phrase_scope.py) and the host time of the same lists
made with numpy, at these shapes:

  tests       the largest shape of tests/test_near_scope_gpu.py: the 65 items of tests/near_cases.py (Nears mixed with
              phrases) over the 700-document random corpus;
  ucc-en      tests/golden/corpus/law_en.jsonl cut by the index's own tokeniser (148 101 tokens): the 1 168 distinct token
              pairs of bench_phrase_scope.py as unordered Nears at distance 5 and at distance 255, and as phrases;
  worst case  one document of 4 550 tokens in which every token but the first is an anchor of an ordered Near at distance
              255 that never completes: one wave, len x (n + 1) steps.

The device figures are the medians of --reps timed calls between two events on the stream, after one untimed call; the
operands are resident.  The host figure is the median wall time of a numpy scan per pair: the positions of either token,
each position of the first matched to the nearest positions of the second by a binary search, kept when within the
distance and inside the same document.  Lists are compared before anything is timed.  Prints ONE JSON line.

    python scripts/bench_near_scope.py [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))

from bench_phrase_scope import dev_arr, host_lists, report, timed  # noqa: E402

S_OPS = ("int64", "int32", "int32", "int32")


def span_ms(torch, nat, gi, ops, bound, reps):
    """(span step ms, list_ptr, docs, workspace bytes) of the items `ops` = (ptr, terms, kind, dist)."""
    dev = torch.device("cuda", 0)
    n = int(ops[2].size)
    cand_max, rows_cap = int(max(bound)), int(sum(bound))
    t = [dev_arr(torch, a, dt) for a, dt in zip(ops, S_OPS)]
    lp = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    dc = torch.zeros(max(rows_cap, 1), dtype=torch.int32, device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    wb = nat.span_lists_plan(n, cand_max)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        gi.span_lists_device(*[x.data_ptr() for x in t], n, cand_max, rows_cap, lp.data_ptr(), dc.data_ptr(), st.data_ptr(),
                             work.data_ptr(), wb, stream)
    ms = timed(torch, step, reps)
    assert not st.cpu().numpy().any()
    ptr = lp.cpu().numpy()
    return ms, ptr, dc.cpu().numpy()[:ptr[-1]], wb


def pair_ops(pairs, kind: int, dist: int):
    n = len(pairs)
    return (np.arange(0, 2 * n + 1, 2, dtype=np.int64), np.asarray(pairs, dtype=np.int32).ravel(),
            np.full(n, kind, dtype=np.int32), np.full(n, dist, dtype=np.int32))


def host_near_lists(doc_ptr, tokens, pairs, dist: int):
    """The numpy scan of two-token unordered Nears of different tokens: (list_ptr, docs)."""
    doc_of = np.searchsorted(doc_ptr, np.arange(tokens.size), side="right") - 1
    where = {}
    parts = []
    for a, b in pairs:
        for t in (a, b):
            if t not in where:
                where[t] = np.flatnonzero(tokens == t)
        pa, pb = where[a], where[b]
        j = np.searchsorted(pb, pa)
        hit = np.zeros(pa.size, dtype=bool)
        for k in (j - 1, j):  # the nearest position of b on either side
            ok = (k >= 0) & (k < pb.size)
            q = pb[np.clip(k, 0, pb.size - 1)]
            hit |= ok & (np.abs(q - pa) <= dist) & (doc_of[q] == doc_of[pa])
        parts.append(np.unique(doc_of[pa[hit]]).astype(np.int32))
    p = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([x.size for x in parts], out=p[1:])
    return p, (np.concatenate(parts) if parts else np.zeros(0, np.int32))


def host_ms(fn, reps):
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[1:], out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch

    import near_cases as NC
    import phrase_cases as PC
    from legal_rag_amd import _native as nat
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.retrieval.builders.bm25_builder import tokenize_corpus
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    out = {"device": nat.device_name(0), "reps": args.reps}

    def index_of(corpus):
        tp, pd, pt, idf, dl, avgdl = corpus.postings()
        gi = nat.BM25Index(tp, pd, pt, idf, dl, avgdl)
        gi.set_tokens(*corpus.stream())
        return gi

    # ---- the largest test shape ----
    corpus = PC.rand_corpus()
    gi = index_of(corpus)
    items = NC.rand_items(corpus)
    bound = [NC.driver_len(corpus, it) for it in items]
    ms, ptr, docs, wb = span_ms(torch, nat, gi, NC.operands(items), bound, args.reps)
    want_ptr, want_docs = NC.expected_lists(corpus, items)
    assert np.array_equal(ptr, want_ptr) and np.array_equal(docs, want_docs)
    out["tests"] = {"items": len(items), "docs": corpus.n_docs, "cand_max": max(bound), "rows": int(ptr[-1]), "work_bytes": wb,
                    "span_step_three_launches": report(ms)}

    # ---- UCC-en: the 1 168 pairs of bench_phrase_scope.py, as Nears at two distances and as phrases ----
    chunks = load_chunks_from_dir(str(ROOT / "tests" / "golden" / "corpus"), "law_en.jsonl")
    tdocs, _ = tokenize_corpus(chunks)
    model = BM25Okapi(tdocs)
    tp, pd, pt, idf, dl = model.to_csr()
    gi2 = nat.BM25Index(tp, pd, pt, idf, dl, float(model.avgdl))
    doc_ptr, tokens = model.token_stream(tdocs)
    gi2.set_tokens(doc_ptr, tokens)
    dfs = np.diff(tp)
    inside = np.ones(tokens.size - 1, dtype=bool)
    cut = doc_ptr[1:-1]
    inside[cut[(cut > 0) & (cut < tokens.size)] - 1] = False
    a, b = tokens[:-1][inside], tokens[1:][inside]
    ok = (dfs[a] >= 20) & (dfs[a] <= 300) & (dfs[b] >= 20) & (dfs[b] <= 300) & (a != b)
    pairs = np.unique(np.stack([a[ok], b[ok]], axis=1), axis=0)
    pick = np.sort(np.random.default_rng(0).choice(pairs.shape[0], size=1168, replace=False))
    pairs = [(int(x), int(y)) for x, y in pairs[pick]]
    bound = [int(min(dfs[x], dfs[y])) for x, y in pairs]
    ucc = {"pairs": len(pairs), "docs": int(doc_ptr.size - 1), "tokens": int(tokens.size), "terms": int(dfs.size),
           "cand_max": max(bound), "rows_cap": sum(bound)}
    ms, ptr, docs, wb = span_ms(torch, nat, gi2, pair_ops(pairs, 0, 0), bound, args.reps)
    hp, hd = host_lists(doc_ptr, tokens, [list(p) for p in pairs])
    assert np.array_equal(ptr, hp) and np.array_equal(docs, hd)
    ucc["phrases"] = {"rows": int(ptr[-1]), "span_step_three_launches": report(ms), "work_bytes": wb}
    for dist in (5, 255):
        ms, ptr, docs, wb = span_ms(torch, nat, gi2, pair_ops(pairs, 1, dist), bound, args.reps)
        ms_h, (hp, hd) = host_ms(lambda: host_near_lists(doc_ptr, tokens, pairs, dist), min(args.reps, 5))
        assert np.array_equal(ptr, hp) and np.array_equal(docs, hd)
        ucc[f"near_distance_{dist}"] = {"rows": int(ptr[-1]), "span_step_three_launches": report(ms),
                                        "host_numpy_scan": report(ms_h)}
    out["ucc_en"] = ucc

    # ---- the worst case alone: 4 550 tokens, every one but the first an anchor that scans 255 tokens and finds nothing ----
    worst = PC.SeqCorpus("worst", 2, [[1] + [0] * (NC.LONG_LEN - 1)])
    item = NC.near([0, 1], NC.MAX_DIST, True)
    ms, ptr, docs, wb = span_ms(torch, nat, index_of(worst), NC.operands([item]), [1], args.reps)
    assert ptr.tolist() == [0, 0]
    out["worst_case_4550_tokens_ordered_255"] = {"steps": NC.LONG_LEN * (NC.MAX_DIST + 1), "span_step_three_launches": report(ms)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

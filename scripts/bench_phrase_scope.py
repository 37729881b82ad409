"""amdr_phrase_lists_device and amdr_term_scope_lists_device behind it: the event time of each step's three launches
(count, scan, write), beside the host time of the same lists made with numpy — a window scan of the whole token stream per
phrase — at two shapes:

  tests    the largest shape of tests/test_phrase_scope_gpu.py: the 65 phrases of tests/phrase_cases.py over its
           700-document random corpus, then one constraint per phrase;
  ucc-en   tests/golden/corpus/law_en.jsonl cut by the index's own tokeniser (148 101 tokens): 1 168 distinct two-token
           phrases that occur in the text, each token in 20 .. 300 articles, then one constraint per phrase.

The device figures are the medians of --reps timed calls between two events on the stream, after one untimed call; the
operands are resident (their upload is one pinned copy and is not timed on either side).  The host figure is the median
wall time of the numpy scan: for each phrase, the positions where the stream holds it (L shifted comparisons of the whole
stream), those that cross a document boundary dropped, the rest mapped to documents by a binary search.  Lists and tables
are compared before anything is timed.  Prints ONE JSON line.

    python scripts/bench_phrase_scope.py [--reps 20]
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


def one_must_each(n_terms: int, n_phr: int):
    """The operands of one constraint per phrase: a MUST group holding the phrase's virtual id, no base."""
    return (np.arange(n_phr + 1, dtype=np.int64), np.zeros(n_phr, dtype=np.int32), np.arange(n_phr + 1, dtype=np.int64),
            (n_terms + np.arange(n_phr)).astype(np.int32), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64),
            np.full(n_phr, -1, dtype=np.int32))


def dev_arr(torch, a, dt):
    x = torch.zeros(max(a.size, 1), dtype=getattr(torch, dt), device=torch.device("cuda", 0))
    if a.size:
        x[:a.size].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return x


def timed(torch, call, reps):
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
    return ms


def device_ms(torch, nat, gi, n_terms, phrases, bound, reps):
    """(phrase step ms, term step ms, list_ptr, docs, table ptr, table rows, the two workspaces' bytes)."""
    dev = torch.device("cuda", 0)
    n_phr = len(phrases)
    pp = np.zeros(n_phr + 1, dtype=np.int64)
    np.cumsum([len(p) for p in phrases], out=pp[1:])
    pt = np.asarray([t for p in phrases for t in p], dtype=np.int32)
    cand_max, rows_cap = int(max(bound)), int(sum(bound))
    tp, tt = dev_arr(torch, pp, "int64"), dev_arr(torch, pt, "int32")
    lp = torch.zeros(n_phr + 1, dtype=torch.int64, device=dev)
    dc = torch.zeros(max(rows_cap, 1), dtype=torch.int32, device=dev)
    pst = torch.zeros(n_phr, dtype=torch.int32, device=dev)
    pwb = nat.phrase_lists_plan(n_phr, cand_max)
    pwork = torch.empty(max(pwb, 1), dtype=torch.uint8, device=dev)
    ops = one_must_each(n_terms, n_phr)
    t = [dev_arr(torch, a, dt) for a, dt in zip(ops, T_OPS)]
    sp = torch.zeros(n_phr + 1, dtype=torch.int64, device=dev)
    rw = torch.zeros(max(rows_cap, 1), dtype=torch.int64, device=dev)
    st = torch.zeros(n_phr, dtype=torch.int32, device=dev)
    wb = nat.term_scope_plan(n_phr, cand_max)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def phrase_step():
        gi.phrase_lists_device(tp.data_ptr(), tt.data_ptr(), n_phr, cand_max, rows_cap, lp.data_ptr(), dc.data_ptr(),
                               pst.data_ptr(), pwork.data_ptr(), pwb, stream)

    def term_step():
        gi.term_scope_device([x.data_ptr() for x in t], 0, n_phr, n_phr, cand_max, rows_cap, sp.data_ptr(), rw.data_ptr(),
                             st.data_ptr(), work.data_ptr(), wb, stream, lists=(lp.data_ptr(), dc.data_ptr(), n_phr))
    ms_p = timed(torch, phrase_step, reps)
    ms_t = timed(torch, term_step, reps)
    assert not pst.cpu().numpy().any() and not st.cpu().numpy().any()
    ptr, tptr = lp.cpu().numpy(), sp.cpu().numpy()
    return ms_p, ms_t, ptr, dc.cpu().numpy()[:ptr[-1]], tptr, rw.cpu().numpy()[:tptr[-1]], pwb, wb


def host_lists(doc_ptr, tokens, phrases):
    """The numpy window scan: (list_ptr, docs) of the phrases over the token stream."""
    parts = []
    n = tokens.size
    for ph in phrases:
        L = len(ph)
        hit = tokens[:n - L + 1] == ph[0]
        for j in range(1, L):
            hit &= tokens[j:n - L + 1 + j] == ph[j]
        at = np.flatnonzero(hit)
        d = np.searchsorted(doc_ptr, at, side="right") - 1
        parts.append(np.unique(d[at + L <= doc_ptr[d + 1]]).astype(np.int32))  # (a match stays inside its document)
    p = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([x.size for x in parts], out=p[1:])
    return p, (np.concatenate(parts) if parts else np.zeros(0, np.int32))


def host_ms(doc_ptr, tokens, phrases, reps):
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = host_lists(doc_ptr, tokens, phrases)
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms[1:], out


def report(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def shape(torch, nat, gi, n_terms, df, doc_ptr, tokens, phrases, reps):
    bound = [int(min(df[t] for t in p)) for p in phrases]  # the host's upper bound of each list: both steps' bounds
    ms_p, ms_t, ptr, docs, tptr, trows, pwb, wb = device_ms(torch, nat, gi, n_terms, phrases, bound, reps)
    ms_h, (hp, hd) = host_ms(doc_ptr, tokens, phrases, reps)
    assert np.array_equal(hp, ptr) and np.array_equal(hd, docs) and np.array_equal(tptr, ptr) and np.array_equal(trows, docs)
    return {"phrases": len(phrases), "docs": int(doc_ptr.size - 1), "tokens": int(tokens.size), "cand_max": max(bound),
            "rows_cap": sum(bound), "rows": int(ptr[-1]), "phrase_work_bytes": pwb, "term_work_bytes": wb,
            "phrase_step_three_launches": report(ms_p), "term_step_three_launches": report(ms_t),
            "host_numpy_window_scan": report(ms_h)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch

    import phrase_cases as PC
    from legal_rag_amd import _native as nat
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.retrieval.builders.bm25_builder import tokenize_corpus
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    out = {"device": nat.device_name(0), "reps": args.reps}

    # ---- the largest test shape ----
    corpus = PC.rand_corpus()
    tp, pd, pt, idf, dl, avgdl = corpus.postings()
    gi = nat.BM25Index(tp, pd, pt, idf, dl, avgdl)
    doc_ptr, tokens = corpus.stream()
    gi.set_tokens(doc_ptr, tokens)
    out["tests"] = shape(torch, nat, gi, corpus.n_terms, corpus.df(), doc_ptr, tokens, PC.rand_phrases(corpus), args.reps)

    # ---- UCC-en, 1 168 distinct two-token phrases ----
    chunks = load_chunks_from_dir(str(ROOT / "tests" / "golden" / "corpus"), "law_en.jsonl")
    docs, _ = tokenize_corpus(chunks)
    model = BM25Okapi(docs)
    tp, pd, pt, idf, dl = model.to_csr()
    gi2 = nat.BM25Index(tp, pd, pt, idf, dl, float(model.avgdl))
    doc_ptr2, tokens2 = model.token_stream(docs)
    gi2.set_tokens(doc_ptr2, tokens2)
    dfs = np.diff(tp)
    inside = np.ones(tokens2.size - 1, dtype=bool)
    cut = doc_ptr2[1:-1]
    inside[cut[(cut > 0) & (cut < tokens2.size)] - 1] = False  # a pair that straddles two documents is no phrase of the text
    a, b = tokens2[:-1][inside], tokens2[1:][inside]
    ok = (dfs[a] >= 20) & (dfs[a] <= 300) & (dfs[b] >= 20) & (dfs[b] <= 300)
    pairs = np.unique(np.stack([a[ok], b[ok]], axis=1), axis=0)
    pick = np.sort(np.random.default_rng(0).choice(pairs.shape[0], size=1168, replace=False))
    phrases = [[int(x), int(y)] for x, y in pairs[pick]]
    out["ucc_en"] = dict(shape(torch, nat, gi2, int(len(dfs)), dfs, doc_ptr2, tokens2, phrases, args.reps), terms=int(len(dfs)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

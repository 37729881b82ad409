"""amdr_bm25_marks: the event time of its one kernel (amdr_bm25_marks_kernel_ms, the host twin's own timer) beside the
wall time of the plain-Python restatement of the rule (tests/marks_cases.py) for the same pairs, on UCC-en
(tests/golden/corpus/law_en.jsonl cut by the index's own tokeniser) at two shapes:

  64 x 10     64 questions with 10 hits each;
  1024 x 10   1 024 questions with 10 hits each.

A question is five words drawn from one article (so they occur), all loose, plus the phrase of two adjacent tokens of that
article, its members phrase-only; the weights are the model's idf; the hits are the article itself and nine random ones.
window 48, marks_cap 32.  The outputs of both sides are compared, byte for byte, before anything is reported.  The device
figure is the median over --reps calls after one untimed call; the restatement is run once per shape.  Prints ONE JSON line.

    python scripts/bench_marks.py [--reps 20]
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

WINDOW, CAP, K = 48, 32, 10


def make_queries(MC, rng, docs_ids, idf, nq):
    """(queries, hits [nq, K])."""
    n = len(docs_ids)
    long_enough = [d for d in range(n) if len(docs_ids[d]) >= 8]
    queries, hits = [], np.zeros((nq, K), np.int64)
    for q in range(nq):
        d = long_enough[int(rng.integers(0, len(long_enough)))]
        seq = docs_ids[d]
        words = [int(seq[i]) for i in rng.choice(len(seq), size=5, replace=False)]
        at = int(rng.integers(0, len(seq) - 1))
        table, w = {}, [0.0] * MC.SLOTS
        for t in words + [int(seq[at]), int(seq[at + 1])]:
            if t not in table:
                table[t] = len(table)
                w[table[t]] = float(idf[t])
        loose = 0
        for t in words:
            loose |= 1 << table[t]
        queries.append(MC.MarkQuery(table, loose=loose, seqs=[[table[int(seq[at])], table[int(seq[at + 1])]]], w=tuple(w)))
        hits[q, 0] = d
        hits[q, 1:] = rng.integers(0, n, size=K - 1)
    return queries, hits


def shape(MC, gi, docs_ids, idf, nq, reps):
    rng = np.random.default_rng(nq)
    queries, hits = make_queries(MC, rng, docs_ids, idf, nq)
    ops = MC.operands(queries)
    got = gi.marks(hits, *ops, WINDOW, CAP)  # untimed
    t0 = time.perf_counter()
    want = MC.expected(docs_ids, hits, queries, WINDOW, CAP)
    host_ms = (time.perf_counter() - t0) * 1e3
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), "the kernel and the restatement differ"
    ms = []
    for _ in range(reps):
        gi.marks(hits, *ops, WINDOW, CAP)
        ms.append(gi.marks_kernel_ms())
    tokens = int(sum(len(docs_ids[int(d)]) for d in hits.ravel()))
    return {"pairs": int(hits.size), "hit_tokens": tokens, "marks": int(want[0][:, :, 3].sum()),
            "kernel": {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)},
            "python_restatement_ms": round(host_ms, 1)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import marks_cases as MC
    from legal_rag_amd import _native as nat
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.retrieval.builders.bm25_builder import tokenize_corpus
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    chunks = load_chunks_from_dir(str(ROOT / "tests" / "golden" / "corpus"), "law_en.jsonl")
    docs, _ = tokenize_corpus(chunks)
    model = BM25Okapi(docs)
    tp, pd, pt, idf, dl = model.to_csr()
    gi = nat.BM25Index(tp, pd, pt, idf, dl, float(model.avgdl))
    doc_ptr, tokens = model.token_stream(docs)
    gi.set_tokens(doc_ptr, tokens)
    docs_ids = [tokens[doc_ptr[d]:doc_ptr[d + 1]].tolist() for d in range(len(docs))]
    out = {"device": nat.device_name(0), "reps": args.reps, "docs": len(docs), "tokens": int(tokens.size), "window": WINDOW,
           "marks_cap": CAP}
    for nq in (64, 1024):
        out[f"{nq}x{K}"] = shape(MC, gi, docs_ids, idf, nq, args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""amdr_bm25_add: what an ingest of 30 documents into a resident BM25 index costs, against the path it replaces.

Two shapes:
  ucc    the UCC-en fixture (tests/golden/corpus/law_en.jsonl, tokenised as the incremental builder does): all but the
         last 30 chunks are the index, the last 30 the add.  In place: BM25Okapi.add_documents on an object with a
         resident index (host statistics + the add's CSR + amdr_bm25_add).  Replaced path: to_csr() of the re-fitted
         object plus a new BM25Index (what BM25Retriever.load() does after unpickling; the unpickling itself is not
         counted).
  large  a synthetic index of --docs documents and about --postings postings (Zipfian list lengths over --terms terms,
         generated as arrays): BM25Index.add of 30 random documents.  Replaced path: a new BM25Index from the ready
         arrays only — to_csr() walks every posting in the interpreter and is not run at this size, so the figure is a
         lower bound of what the add replaces.
Times are host wall time, call to return (every call is synchronous), the median of --reps after one untimed call;
`merge_kernel` is the device time of the merge kernel between two events on the handle's stream
(amdr_bm25_add_kernel_ms) against its algorithmic bytes — 8 B read + a 4 B doc_len gather + 16 B written per posting —
and a peak of 8 TB/s.  Prints ONE JSON line.

    python scripts/bench_bm25_add.py [--reps 5] [--docs 1000000] [--postings 100000000] [--terms 200000] [--skip-large]
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

PEAK_BYTES_PER_S = 8e12
BYTES_PER_POSTING = 8 + 4 + 16


def ms_of(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def med(xs):
    return round(statistics.median(xs), 3)


def kernel_report(ms_list, nnz):
    ms = statistics.median(ms_list)
    return {"ms": round(ms, 4), "postings": int(nnz), "algorithmic_bytes": int(nnz) * BYTES_PER_POSTING,
            "TB_per_s": round(nnz * BYTES_PER_POSTING / (ms * 1e-3) / 1e12, 3),
            "fraction_of_8TBps": round(nnz * BYTES_PER_POSTING / (ms * 1e-3) / PEAK_BYTES_PER_S, 3)}


def bench_ucc(nat, reps):
    from legal_rag_amd import text
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    chunks = load_chunks_from_dir(str(ROOT / "tests" / "golden" / "corpus"), "law_en.jsonl")
    tokens = [text.jieba_cut(c.text, text.cfg_mode(None), None) for c in chunks]
    old, new = tokens[:-30], tokens[-30:]
    add_ms, kern_ms, replaced_ms, csr_ms = [], [], [], []
    for rep in range(reps + 1):
        m = BM25Okapi(old)
        g = m.gpu(0)
        m._doc_frequencies()  # the one-time cache is the retriever's, not this add's
        t, _ = ms_of(lambda: m.add_documents(new))
        whole = BM25Okapi(tokens)
        t_csr, csr = ms_of(whole.to_csr)
        t_new, f = ms_of(lambda: nat.BM25Index(*csr, float(whole.avgdl), float(whole.k1), float(whole.b)))
        if rep:  # (the first round warms the device and the allocator)
            add_ms.append(t)
            kern_ms.append(g.add_kernel_ms())
            csr_ms.append(t_csr)
            replaced_ms.append(t_csr + t_new)
        nnz = g.info()[2]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g.read(), f.read()))
        g.close()
        f.close()
    return {"docs": len(old), "added": len(new), "postings": int(nnz), "add_documents_ms": med(add_ms),
            "replaced_to_csr_plus_new_index_ms": med(replaced_ms), "of_which_to_csr_ms": med(csr_ms),
            "merge_kernel": kernel_report(kern_ms, nnz)}


def zipf_index(rng, n_docs, n_terms, postings):
    """Term-major CSR as arrays: list lengths ~ rank^-0.75 scaled to `postings` in all (at most n_docs each), a list's
    documents an arithmetic progression from a random start (ascending, in range)."""
    w = np.arange(1, n_terms + 1) ** -0.75
    dfs = np.minimum(np.maximum((w * (postings / w.sum())).astype(np.int64), 1), n_docs)
    ptr = np.zeros(n_terms + 1, dtype=np.int64)
    np.cumsum(dfs, out=ptr[1:])
    nnz = int(ptr[-1])
    step = (n_docs // dfs).astype(np.int32)
    start = (rng.random(n_terms) * (n_docs - (dfs - 1) * step)).astype(np.int32)
    term_of = np.repeat(np.arange(n_terms, dtype=np.int32), dfs)
    doc = np.arange(nnz, dtype=np.int64)
    doc -= ptr[term_of]
    doc = doc.astype(np.int32)
    doc *= step[term_of]
    doc += start[term_of]
    del term_of
    tf = rng.integers(1, 10, size=nnz, dtype=np.int32)
    return ptr, doc, tf


def random_add(rng, n_terms, n_add, terms_per_doc=120):
    """The added documents' CSR over n_terms + 16 terms (16 new ones behind the table)."""
    V = n_terms + 16
    pairs = set()
    for d in range(n_add):
        ts = np.unique(np.concatenate([np.minimum((rng.zipf(1.2, size=terms_per_doc) - 1), n_terms - 1),
                                       rng.integers(n_terms, V, size=2)]))
        pairs.update((int(t), d) for t in ts)
    pairs = sorted(pairs)
    t = np.asarray([p[0] for p in pairs], dtype=np.int64)
    ptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(t, minlength=V), out=ptr[1:])
    doc = np.asarray([p[1] for p in pairs], dtype=np.int32)
    return ptr, doc, rng.integers(1, 10, size=doc.size, dtype=np.int32)


def bench_large(nat, reps, n_docs, n_terms, postings):
    rng = np.random.default_rng(0)
    ptr, doc, tf = zipf_index(rng, n_docs, n_terms, postings)
    doc_len = rng.integers(20, 400, size=n_docs, dtype=np.int32)
    idf = rng.uniform(0.05, 12.0, size=n_terms)
    t_create, g = ms_of(lambda: nat.BM25Index(ptr, doc, tf, idf, doc_len, 210.0))
    nnz0 = g.info()[2]
    del doc, tf
    add_ms, kern_ms = [], []
    V = n_terms
    for rep in range(reps + 1):
        a_ptr, a_doc, a_tf = random_add(rng, V, 30)
        V = len(a_ptr) - 1
        idf = np.concatenate([idf, rng.uniform(0.05, 12.0, size=V - idf.size)])
        a_len = rng.integers(20, 400, size=30, dtype=np.int32)
        t, _ = ms_of(lambda: g.add(a_ptr, a_doc, a_tf, idf, a_len, 210.0 + rep))
        if rep:
            add_ms.append(t)
            kern_ms.append(g.add_kernel_ms())
    info = g.info()
    g.close()
    return {"docs": n_docs, "terms": n_terms, "postings": int(nnz0), "added_per_call": 30, "add_ms": med(add_ms),
            "replaced_new_index_from_ready_arrays_ms": round(t_create, 1), "merge_kernel": kernel_report(kern_ms, info[2]),
            "info": list(info)}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--postings", type=int, default=100_000_000)
    ap.add_argument("--terms", type=int, default=200_000)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args(argv)
    from legal_rag_amd import _native as nat
    out = {"device": nat.device_name(0), "reps": args.reps, "ucc": bench_ucc(nat, args.reps)}
    if not args.skip_large:
        out["large"] = bench_large(nat, args.reps, args.docs, args.terms, args.postings)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

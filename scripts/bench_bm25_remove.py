"""amdr_bm25_remove: what taking 30 documents out of a resident BM25 index costs, against the path it replaces.

Two shapes:
  ucc    the UCC-en fixture (tests/golden/corpus/law_en.jsonl, tokenised as the incremental builder does): the whole
         fixture is the index, 30 chunks spread over it are removed.  In place: BM25Okapi.remove_documents on an object
         with a resident index (host statistics + the term map + amdr_bm25_remove).  Replaced path: a re-fit of the
         surviving documents' tokens, to_csr() of it and a new BM25Index (re-tokenising and unpickling not counted).
  large  a synthetic index of --docs documents and about --postings postings (Zipfian list lengths over --terms terms,
         generated as arrays): BM25Index.remove of 30 random documents per call with the null term map.  Replaced path: a
         new BM25Index from the ready arrays only — the re-fit and to_csr() walk every posting in the interpreter and are
         not run at this size, so the figure is a lower bound of what the remove replaces.
Times are host wall time, call to return (every call is synchronous), the median of --reps after one untimed call;
`remove_passes` is the summed device time of the remove's passes between events on the handle's stream
(amdr_bm25_remove_kernel_ms) against their algorithmic bytes — count pass: 4 B read + a 4 B doc_new gather + 2 B written
per OLD posting; scatter pass: 10 B read + a 4 B doc_new gather per old posting, a 4 B doc_len gather + 16 B written per
surviving posting — and a peak of 8 TB/s.  Prints ONE JSON line.

    python scripts/bench_bm25_remove.py [--reps 5] [--docs 1000000] [--postings 100000000] [--terms 200000] [--skip-large]
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
sys.path.insert(0, str(ROOT / "scripts"))

PEAK_BYTES_PER_S = 8e12
BYTES_PER_OLD_POSTING = (4 + 4 + 2) + (10 + 4)
BYTES_PER_NEW_POSTING = 4 + 16
N_REMOVE = 30


def ms_of(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def med(xs):
    return round(statistics.median(xs), 3)


def passes_report(ms_list, nnz_old, nnz_new):
    ms = statistics.median(ms_list)
    nbytes = int(nnz_old) * BYTES_PER_OLD_POSTING + int(nnz_new) * BYTES_PER_NEW_POSTING
    return {"ms": round(ms, 4), "postings_before": int(nnz_old), "postings_after": int(nnz_new), "algorithmic_bytes": nbytes,
            "TB_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3), "fraction_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S, 3)}


def bench_ucc(nat, reps):
    from legal_rag_amd import text
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    chunks = load_chunks_from_dir(str(ROOT / "tests" / "golden" / "corpus"), "law_en.jsonl")
    tokens = [text.jieba_cut(c.text, text.cfg_mode(None), None) for c in chunks]
    ids = sorted(np.random.default_rng(0).choice(len(tokens), size=N_REMOVE, replace=False).tolist())
    gone = set(ids)
    left = [t for d, t in enumerate(tokens) if d not in gone]
    rm_ms, kern_ms, replaced_ms, fit_ms, csr_ms = [], [], [], [], []
    for rep in range(reps + 1):
        m = BM25Okapi(tokens)
        g = m.gpu(0)
        m._doc_frequencies()  # the one-time cache is the retriever's, not this removal's
        nnz_old = g.info()[2]
        t, _ = ms_of(lambda: m.remove_documents(ids))
        t_fit, whole = ms_of(lambda: BM25Okapi(left))
        t_csr, csr = ms_of(whole.to_csr)
        t_new, f = ms_of(lambda: nat.BM25Index(*csr, float(whole.avgdl), float(whole.k1), float(whole.b)))
        if rep:  # (the first round warms the device and the allocator)
            rm_ms.append(t)
            kern_ms.append(g.remove_kernel_ms())
            fit_ms.append(t_fit)
            csr_ms.append(t_csr)
            replaced_ms.append(t_fit + t_csr + t_new)
        nnz = g.info()[2]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g.read(), f.read()))
        g.close()
        f.close()
    return {"docs": len(tokens), "removed": len(ids), "terms_before": len(BM25Okapi(tokens).idf), "terms_after": len(whole.idf),
            "remove_documents_ms": med(rm_ms), "replaced_refit_plus_to_csr_plus_new_index_ms": med(replaced_ms),
            "of_which_refit_ms": med(fit_ms), "of_which_to_csr_ms": med(csr_ms),
            "remove_passes": passes_report(kern_ms, nnz_old, nnz)}


def bench_large(nat, reps, n_docs, n_terms, postings):
    from bench_bm25_add import zipf_index
    rng = np.random.default_rng(0)
    ptr, doc, tf = zipf_index(rng, n_docs, n_terms, postings)
    doc_len = rng.integers(20, 400, size=n_docs, dtype=np.int32)
    idf = rng.uniform(0.05, 12.0, size=n_terms)
    t_create, g = ms_of(lambda: nat.BM25Index(ptr, doc, tf, idf, doc_len, 210.0))
    nnz0 = g.info()[2]
    del doc, tf
    rm_ms, kern_ms, before, after = [], [], [], []
    for rep in range(reps + 1):
        n = g.info()[0]
        ids = np.sort(rng.choice(n, size=N_REMOVE, replace=False)).astype(np.int64)
        nnz_old = g.info()[2]
        t, _ = ms_of(lambda: g.remove(ids, idf, 210.0 + rep))
        if rep:
            rm_ms.append(t)
            kern_ms.append(g.remove_kernel_ms())
            before.append(nnz_old)
            after.append(g.info()[2])
    info = g.info()
    g.close()
    return {"docs": n_docs, "terms": n_terms, "postings": int(nnz0), "removed_per_call": N_REMOVE, "remove_ms": med(rm_ms),
            "replaced_new_index_from_ready_arrays_ms": round(t_create, 1),
            "remove_passes": passes_report(kern_ms, statistics.median(before), statistics.median(after)), "info": list(info)}


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

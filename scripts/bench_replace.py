"""amdr_bm25_replace / amdr_dense_replace / amdr_maxsim_replace: the device time of replacing documents in place, beside
each pass's algorithmic bytes, and for the same documents the device time of the path it stands in for — the remove
followed by the add — on ONE index of each kind, in one process.

  bm25    a synthetic index of --docs documents and about --postings postings (Zipfian list lengths over --terms terms):
          30 random documents per call take new term sets (the null term map, 16 new terms offered per call).  replace:
          amdr_bm25_replace_kernel_ms — count pass 4 B read + a 4 B gather + 2 B written per OLD posting; scatter pass 10 B
          read + a 4 B gather per old posting, a 4 B doc_len gather + 16 B written per surviving posting; add pass 8 B read
          + an 8 B id gather + a 4 B doc_len gather + 16 B written per added posting (the searches in the other list not
          counted).  existing path: amdr_bm25_remove_kernel_ms of the same ids + amdr_bm25_add_kernel_ms of the same CSR.
  dense   --rows x --dim: replace of 0.01 % and of 1 % of the rows, scattered (the scatter should scale with n_rep, not n):
          amdr_dense_replace_kernel_ms against 2 x the replaced bytes + 8 B an id.  existing path:
          amdr_dense_remove_kernel_ms of the same rows (the add behind it is a host-to-device copy without a kernel).
  maxsim  --store-docs documents of 1 .. 319 tokens: 1 % of the documents, scattered, take new token rows of other
          lengths: amdr_maxsim_replace_kernel_ms (doc_ptr rebuild + splice) against 2 x the store's bytes afterwards +
          both doc_ptrs + 16 B of scratch a document.  existing path: amdr_maxsim_remove_kernel_ms (the add: no kernel).
Every figure is the median of --reps calls after one untimed call; the spread (min, max) is printed beside it.  A peak of
8 TB/s.  Prints ONE JSON line.

    python scripts/bench_replace.py [--reps 5] [--docs 1000000] [--postings 100000000] [--terms 200000]
                                    [--rows 2000000] [--dim 768] [--store-docs 60000]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

PEAK_BYTES_PER_S = 8e12
N_REP = 30


def report(ms_list, bytes_list=None):
    ms = statistics.median(ms_list)
    out = {"ms": round(ms, 4), "min_ms": round(min(ms_list), 4), "max_ms": round(max(ms_list), 4)}
    if bytes_list is not None:
        nbytes = int(statistics.median(bytes_list))
        out.update(algorithmic_bytes=nbytes, TB_per_s=round(nbytes / (ms * 1e-3) / 1e12, 3),
                   fraction_of_8TBps=round(nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S, 3))
    return out


def bench_bm25(nat, reps, n_docs, n_terms, postings):
    from bench_bm25_add import random_add, zipf_index
    rng = np.random.default_rng(0)
    ptr, doc, tf = zipf_index(rng, n_docs, n_terms, postings)
    doc_len = rng.integers(20, 400, size=n_docs, dtype=np.int32)
    idf = rng.uniform(0.05, 12.0, size=n_terms)
    g = nat.BM25Index(ptr, doc, tf, idf, doc_len, 210.0)
    nnz0 = g.info()[2]
    del doc, tf
    rp_ms, rp_bytes, old_ms, rm_ms, add_ms = [], [], [], [], []
    V = n_terms
    for rep in range(reps + 1):
        a_ptr, a_doc, a_tf = random_add(rng, V, N_REP)
        V = len(a_ptr) - 1
        idf = np.concatenate([idf, rng.uniform(0.05, 12.0, size=V - idf.size)])
        lens = rng.integers(20, 400, size=N_REP, dtype=np.int32)
        n = g.info()[0]
        # the replace, then on the same handle the same documents by the existing path: they leave, and come back behind
        ids = np.sort(rng.choice(n, size=N_REP, replace=False)).astype(np.int64)
        nnz_old = g.info()[2]
        g.replace(ids, a_ptr, a_doc, a_tf, lens, idf, 210.0 + rep)
        nnz_new = g.info()[2]
        t_rp = g.replace_kernel_ms()
        g.remove(ids, idf, 210.5 + rep)
        t_rm = g.remove_kernel_ms()
        g.add(a_ptr, a_doc, a_tf, idf, lens, 210.0 + rep)
        t_add = g.add_kernel_ms()
        if rep:
            kept = nnz_new - int(a_ptr[-1])
            rp_ms.append(t_rp)
            rp_bytes.append(nnz_old * (10 + 14) + kept * 20 + int(a_ptr[-1]) * 36)
            rm_ms.append(t_rm)
            add_ms.append(t_add)
            old_ms.append(t_rm + t_add)
    info = g.info()
    replaces = g.replaces()
    g.close()
    return {"docs": n_docs, "terms": n_terms, "postings": int(nnz0), "replaced_per_call": N_REP,
            "replace_passes": report(rp_ms, rp_bytes), "remove_plus_add_passes": report(old_ms),
            "of_which_remove": report(rm_ms), "of_which_add": report(add_ms), "info": list(info), "replaces": replaces}


def unit_block(rng, rows, d):
    block = rng.standard_normal((min(rows, 1 << 18), d)).astype(np.float32)
    block /= np.linalg.norm(block, axis=1, keepdims=True)
    X = np.empty((rows, d), dtype=np.float32)
    for lo in range(0, rows, block.shape[0]):
        X[lo:lo + block.shape[0]] = block[:min(block.shape[0], rows - lo)]
    return X


def bench_dense(nat, reps, n, d):
    rng = np.random.default_rng(0)
    X = unit_block(rng, n, d)
    g = nat.DenseIndex(X)
    out = {"rows": n, "dim": d, "bytes": n * d * 4}
    for share, name in ((10_000, "0.01 %"), (100, "1 %")):
        n_rep = max(1, n // share)
        R = unit_block(rng, n_rep, d)
        kern, nbytes = [], []
        for rep in range(reps + 1):
            ids = np.sort(rng.choice(n, size=n_rep, replace=False)).astype(np.int64)
            g.replace(ids, R)
            X[ids] = R
            if rep:
                kern.append(g.replace_kernel_ms())
                nbytes.append(2 * n_rep * d * 4 + n_rep * 8)
        out[f"replace_kernel_{name}"] = dict(report(kern, nbytes), rows_replaced=n_rep)
    for lo in (0, n // 2, max(0, n - 1000)):  # the resident rows are the host's edit
        cnt = min(1000, n - lo)
        assert np.array_equal(g.read_rows(lo, cnt).view(np.uint32), X[lo:lo + cnt].view(np.uint32))
    # the existing path's kernel for the 1 % of the last call: the compaction of the whole matrix (the add has no kernel)
    g.remove(ids)
    out["remove_kernel_1 %"] = report([g.remove_kernel_ms()], [2 * (n - ids.size) * d * 4 + ids.size * 8])
    g.close()
    return out


def bench_maxsim(nat, reps, n_docs):
    rng = np.random.default_rng(0)
    lens = rng.integers(1, 320, size=n_docs)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    D = unit_block(rng, int(ptr[-1]), 128)
    g = nat.MaxSimIndex(D, ptr)
    n_rep = max(1, n_docs // 100)
    kern, nbytes = [], []
    for rep in range(reps + 1):
        ids = np.sort(rng.choice(n_docs, size=n_rep, replace=False)).astype(np.int64)
        new_lens = rng.integers(1, 320, size=n_rep)
        new_ptr = np.concatenate([[0], np.cumsum(new_lens)]).astype(np.int64)
        g.replace(ids, unit_block(rng, int(new_ptr[-1]), 128), new_ptr)
        if rep:
            kern.append(g.replace_kernel_ms())
            nbytes.append(2 * g.info()[1] * 512 + (n_rep + 1) * 16 + 2 * (n_docs + 1) * 8 + n_docs * 16)
    info = g.info()
    g.remove(ids)
    rm = report([g.remove_kernel_ms()], [2 * g.info()[1] * 512 + ids.size * 8 + (n_docs + 1 + g.info()[0] + 1) * 8])
    g.close()
    return {"docs": n_docs, "tokens": int(ptr[-1]), "bytes": int(ptr[-1]) * 512, "docs_replaced_per_call": n_rep,
            "tokens_after": int(info[1]), "replace_kernel": report(kern, nbytes), "remove_kernel_same_documents": rm}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--postings", type=int, default=100_000_000)
    ap.add_argument("--terms", type=int, default=200_000)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--store-docs", type=int, default=60_000)
    args = ap.parse_args(argv)
    from legal_rag_amd import _native as nat
    out = {"device": nat.device_name(0), "reps": args.reps,
           "bm25": bench_bm25(nat, args.reps, args.docs, args.terms, args.postings),
           "dense": bench_dense(nat, args.reps, args.rows, args.dim), "maxsim": bench_maxsim(nat, args.reps, args.store_docs)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

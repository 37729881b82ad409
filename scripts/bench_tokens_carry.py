"""The carrying BM25 updates (amdr_bm25_add_carry / _remove_carry / _replace_carry): what keeping the resident token stream
current costs on the device, against what an update cost without it.

A synthetic corpus of its own making (--docs documents of 10 .. 90 tokens, Zipfian over --terms words; nothing outside the
repository is read) is fitted, put on the device and given its token stream once.  Then ONE carrying add, ONE carrying
remove and ONE carrying replace of --edit documents each run through BM25Okapi.*_documents(carry_tokens=True), and for
each the script prints
  carry_kernel_ms     amdr_bm25_carry_kernel_ms: the event time of the carry passes (the scan of the new lengths and the
                      pass over the new tokens)
  algorithmic_bytes   of those passes: per NEW token 4 B read + 4 B written, + a 4 B gather of the term map where the
                      call has one (remove, replace); per new document 4 B read + 8 B written (the widened length) and
                      8 B read + 8 B written (the scan)
  d2d_copy_ms         the event time of a device-to-device copy with the same traffic in the same process: a buffer of
                      algorithmic_bytes / 2 (a copy reads and writes every byte), the median of --reps after one untimed copy
and once, at the end,
  rebuild_ms          the wall time of what an update cost before: BM25Okapi.token_stream over ALL documents plus
                      set_tokens (cutting the chunk texts again, which the retriever also does, is not counted: a lower
                      bound), after checking that the carried stream IS that stream, array for array.
Prints ONE JSON line.

    python scripts/bench_tokens_carry.py [--docs 100000] [--terms 50000] [--edit 30] [--reps 5]
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
BYTES_PER_DOC = (4 + 8) + (8 + 8)


def make_docs(rng, n, words):
    lens = rng.integers(10, 91, size=n)
    ids = np.minimum(rng.zipf(1.2, size=int(lens.sum())) - 1, len(words) - 1)
    out, at = [], 0
    for k in lens.tolist():
        out.append([words[t] for t in ids[at:at + k].tolist()])
        at += k
    return out


def d2d_copy_ms(nbytes, reps):
    import torch
    dev = torch.device("cuda", 0)
    a = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def report(g, wall_ms, with_map, reps):
    n_docs = g.info()[0]
    n_tok = g.tokens_info()[1]
    ms = g.carry_kernel_ms()
    nbytes = n_tok * (8 + (4 if with_map else 0)) + n_docs * BYTES_PER_DOC
    copy_ms = d2d_copy_ms(nbytes // 2, reps)
    return {"docs_after": n_docs, "tokens_after": n_tok, "update_wall_ms": round(wall_ms, 3), "carry_kernel_ms": round(ms, 4),
            "algorithmic_bytes": nbytes, "TB_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3) if ms > 0 else None,
            "fraction_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S, 4) if ms > 0 else None,
            "d2d_copy_ms": round(copy_ms, 4), "carry_over_copy": round(ms / copy_ms, 2) if copy_ms > 0 else None}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--terms", type=int, default=50_000)
    ap.add_argument("--edit", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    from legal_rag_amd import _native as nat
    from legal_rag_amd.bm25_model import BM25Okapi
    rng = np.random.default_rng(0)
    words = [f"w{i}" for i in range(args.terms)]
    docs = make_docs(rng, args.docs, words)
    m = BM25Okapi(docs)
    g = m.gpu(0)
    m._doc_frequencies()  # the one-time cache is the retriever's, not an update's
    g.set_tokens(*m.token_stream(docs))
    out = {"device": nat.device_name(0), "docs": args.docs, "terms": len(m.idf), "tokens": g.tokens_info()[1],
           "edit_documents": args.edit}

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    added = make_docs(rng, args.edit, words + [f"new{i}" for i in range(8)])
    out["add"] = report(g, timed(lambda: m.add_documents(added, carry_tokens=True)), False, args.reps)
    docs = docs + added
    gone = sorted(rng.choice(len(docs), size=args.edit, replace=False).tolist())
    out["remove"] = report(g, timed(lambda: m.remove_documents(gone, carry_tokens=True)), True, args.reps)
    docs = [d for i, d in enumerate(docs) if i not in set(gone)]
    rows = sorted(rng.choice(len(docs), size=args.edit, replace=False).tolist())
    amended = make_docs(rng, args.edit, words + [f"amended{i}" for i in range(8)])
    out["replace"] = report(g, timed(lambda: m.replace_documents(rows, amended, carry_tokens=True)), True, args.reps)
    for r, d in zip(rows, amended):
        docs[r] = d
    assert m.gpu(0) is g and g.tokens_info()[0] and g.info()[3] == 1 and g.info()[5] == 1 and g.replaces() == 1
    # what every one of the three cost before: the stream made again from all documents (and it is the carried one)
    t = time.perf_counter()
    doc_ptr, tokens = m.token_stream(docs)
    t_stream = (time.perf_counter() - t) * 1e3
    got_ptr, got_tok = g.read_tokens()
    assert np.array_equal(got_ptr, doc_ptr) and np.array_equal(got_tok, tokens), "the carried stream is not the rebuilt one"
    t_set = timed(lambda: g.set_tokens(doc_ptr, tokens))
    out["rebuild_ms"] = {"token_stream": round(t_stream, 1), "set_tokens": round(t_set, 1), "sum": round(t_stream + t_set, 1)}
    g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

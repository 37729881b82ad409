"""amdr_dense_remove / amdr_maxsim_remove: what taking 1 % of the rows, scattered, out of a resident store costs, against
the only alternative before these calls existed — destroy the handle and create a new one from a host copy of the survivors.

Two stores:
  dense   --rows x --dim fp32 rows (default 10 000 000 x 768: the synth10m matrix of bench.py, 30.7 GB), one seeded block of
          unit rows tiled over the matrix (the copy does not look at values).
  maxsim  --docs documents of 1 .. 319 unit-norm 128-d tokens (default 591: the seeded synthetic store of
          scripts/bench_maxsim_add.py, the size of the UCC-en store of bench.py's ucc_colbert), and the same at
          --docs-large (default 60 000 documents, about 4.9 GB of token rows) so that the copy is measured outside the
          256 MiB Infinity Cache.
Per store: `remove_ms` is the host wall time of the call, call to return (it is synchronous), the median of --reps calls
after one untimed one, each removing 1 % of the rows then resident, at random; `remove_kernel` is the device time between
events on the handle's stream (amdr_*_remove_kernel_ms: dense the compaction kernel, maxsim the doc_ptr rebuild + the
compaction kernel) against the passes' algorithmic bytes — every surviving byte read once and written once, the removal
list, and for maxsim both doc_ptrs — and a peak of 8 TB/s; `replaced_destroy_plus_create_ms` is measured once, in the same
process, on the survivors of the last remove (the host copy is made before the clock starts: the reload the call replaces
reads it from a file).  After the last remove the resident rows are compared with the host's filter.  Prints ONE JSON line.

    python scripts/bench_store_remove.py [--reps 3] [--rows 10000000] [--dim 768] [--docs 591] [--docs-large 60000]
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


def ms_of(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def kernel_report(ms_list, bytes_list):
    ms, nbytes = statistics.median(ms_list), int(statistics.median(bytes_list))
    return {"ms": round(ms, 4), "algorithmic_bytes": nbytes, "TB_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3),
            "fraction_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S, 3)}


def scattered(rng, n):
    return np.sort(rng.choice(n, size=max(1, n // 100), replace=False)).astype(np.int64)


def bench_dense(nat, reps, n, d):
    rng = np.random.default_rng(0)
    block = rng.standard_normal((min(n, 1 << 18), d)).astype(np.float32)
    block /= np.linalg.norm(block, axis=1, keepdims=True)
    X = np.empty((n, d), dtype=np.float32)
    for lo in range(0, n, block.shape[0]):
        X[lo:lo + block.shape[0]] = block[:min(block.shape[0], n - lo)]
    X[:, 0] += np.arange(n, dtype=np.float32) * np.float32(1e-9)  # (rows tell their place)
    t_first, g = ms_of(lambda: nat.DenseIndex(X))
    alive = np.arange(n, dtype=np.int64)  # old row of every resident row
    wall, kern, nbytes = [], [], []
    for rep in range(reps + 1):
        m = g.ntotal
        ids = scattered(rng, m)
        t, _ = ms_of(lambda: g.remove(ids))
        alive = np.delete(alive, ids)
        if rep:
            wall.append(t)
            kern.append(g.remove_kernel_ms())
            nbytes.append(2 * (m - ids.size) * d * 4 + ids.size * 8)
    m = g.ntotal
    assert m == alive.size
    for lo in (0, m // 2, max(0, m - 1000)):  # the resident rows are the host's filter
        cnt = min(1000, m - lo)
        assert np.array_equal(g.read_rows(lo, cnt).view(np.uint32), X[alive[lo:lo + cnt]].view(np.uint32))
    # the replaced path: the survivors compacted on the host (in place, before the clock), destroy, create
    for lo in range(0, m, 1 << 20):
        hi = min(lo + (1 << 20), m)
        X[lo:hi] = X[alive[lo:hi]]
    t0 = time.perf_counter()
    g.close()
    f = nat.DenseIndex(X[:m])
    t_replaced = (time.perf_counter() - t0) * 1e3
    f.close()
    return {"rows": n, "dim": d, "bytes": n * d * 4, "removed_per_call": "1 % of the resident rows, scattered",
            "rows_after": int(m), "remove_ms": round(statistics.median(wall), 3), "remove_kernel": kernel_report(kern, nbytes),
            "replaced_destroy_plus_create_ms": round(t_replaced, 1), "first_create_ms": round(t_first, 1)}


def bench_maxsim(nat, reps, n_docs):
    rng = np.random.default_rng(0)
    lens = rng.integers(1, 320, size=n_docs)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    block = rng.standard_normal((min(int(ptr[-1]), 1 << 18), 128)).astype(np.float32)
    block /= np.linalg.norm(block, axis=1, keepdims=True)
    D = np.empty((int(ptr[-1]), 128), dtype=np.float32)
    for lo in range(0, D.shape[0], block.shape[0]):
        D[lo:lo + block.shape[0]] = block[:min(block.shape[0], D.shape[0] - lo)]
    t_first, g = ms_of(lambda: nat.MaxSimIndex(D, ptr))
    alive = np.arange(n_docs, dtype=np.int64)
    wall, kern, nbytes = [], [], []
    for rep in range(reps + 1):
        m = g.info()[0]
        ids = scattered(rng, m)
        t, _ = ms_of(lambda: g.remove(ids))
        alive = np.delete(alive, ids)
        if rep:
            wall.append(t)
            kern.append(g.remove_kernel_ms())
            nbytes.append(2 * g.info()[1] * 512 + ids.size * 8 + (m + 1 + g.info()[0] + 1) * 8)
    keep = np.zeros(n_docs, dtype=bool)
    keep[alive] = True
    left_D = np.ascontiguousarray(D[np.repeat(keep, lens)])
    left_ptr = np.concatenate([[0], np.cumsum(lens[keep])]).astype(np.int64)
    rd, rp = g.read()
    assert np.array_equal(rp, left_ptr) and np.array_equal(rd.view(np.uint32), left_D.view(np.uint32))
    info, stats = g.info(), g.stats()
    t0 = time.perf_counter()
    g.close()
    f = nat.MaxSimIndex(left_D, left_ptr)
    t_replaced = (time.perf_counter() - t0) * 1e3
    assert f.info()[:2] == info[:2] and f.stats() == stats
    f.close()
    return {"docs": n_docs, "tokens": int(ptr[-1]), "bytes": int(ptr[-1]) * 512,
            "removed_per_call": "1 % of the resident documents, scattered", "docs_after": int(info[0]), "tokens_after": int(info[1]),
            "remove_ms": round(statistics.median(wall), 3), "remove_kernel": kernel_report(kern, nbytes),
            "replaced_destroy_plus_create_ms": round(t_replaced, 1), "first_create_ms": round(t_first, 1)}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--docs", type=int, default=591)
    ap.add_argument("--docs-large", type=int, default=60_000)
    args = ap.parse_args(argv)
    from legal_rag_amd import _native as nat
    out = {"device": nat.device_name(0), "reps": args.reps}
    out["maxsim"] = bench_maxsim(nat, args.reps, args.docs)
    print("maxsim:", json.dumps(out["maxsim"]), file=sys.stderr, flush=True)  # (progress; the result is the last line)
    if args.docs_large > 0:
        out["maxsim_large"] = bench_maxsim(nat, args.reps, args.docs_large)
        print("maxsim_large:", json.dumps(out["maxsim_large"]), file=sys.stderr, flush=True)
    if args.rows > 0:
        out["dense"] = bench_dense(nat, args.reps, args.rows, args.dim)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""amdr_maxsim_add on a store of the UCC-en token store's size: what an ingest of 30 documents costs.

A seeded synthetic store — 591 documents of 1 .. 319 unit-norm tokens (about 95 k tokens, the size of the UCC-en store) —
is created, then 30-document parts of the same kind are appended: the first add outgrows the capacity (new buffers,
device copies of D and both images), the following ones fit.  Times are host wall time of `MaxSimIndex.add`, call to
return (the call is synchronous).  Prints ONE JSON line.

    python scripts/bench_maxsim_add.py [--reps 5]
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


def part(rng, n_docs, max_len=320):
    lens = rng.integers(1, max_len, size=n_docs)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    X = rng.standard_normal((int(ptr[-1]), 128)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X, ptr


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    from legal_rag_amd import _native as nat
    rng = np.random.default_rng(0)
    base = part(rng, 591)
    idx = nat.MaxSimIndex(*base)
    idx.search(base[0][:32][None], 10)  # the device is warm before anything is timed

    def timed(p):
        t = time.perf_counter()
        idx.add(*p)
        return (time.perf_counter() - t) * 1e3

    first = part(rng, 30)
    grow_ms = timed(first)
    cap = idx.info()[2]
    fits = [part(rng, 30) for _ in range(args.reps)]
    fit_ms = [timed(p) for p in fits]
    info = idx.info()
    assert info[2] == cap and info[5] == 1, info  # the later adds fitted; no whole-store conversion
    print(json.dumps({"device": nat.device_name(0), "store_tokens": int(base[1][-1]), "store_docs": 591,
                      "add_with_growth": {"docs": 30, "tokens": int(first[1][-1]), "ms": round(grow_ms, 3)},
                      "add_in_capacity": {"docs": 30, "tokens": [int(p[1][-1]) for p in fits],
                                          "ms": [round(x, 3) for x in fit_ms]},
                      "info": list(info)}))


if __name__ == "__main__":
    main()

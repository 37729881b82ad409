"""amdr_vocab_match_device: the event time of the step's three launches (count, scan, write) and the wall time of its
host-pointer twin, next to what a caller does without it — the Python expansion of the same patterns over the same
vocabulary (Fuzzy.fits / Wildcard.fits of retrieval/terms.py on every token) — TAKEN IN THE SAME PROCESS, at these shapes:

  ucc-en     tests/golden/corpus/law_en.jsonl cut by the index's own tokeniser; the stems of the facet benchmark
             (scripts/bench_facets.py, up to 1 168 distinct ones) turned into Fuzzy(stem, edits=1);
  synthetic  10^6 distinct tokens of 3 to 14 letters; 1 pattern and 64 patterns (Fuzzy edits 1 and 2 and Wildcards, mixed).

Method: the operands are resident; every side runs once untimed; then --windows windows per side, ALTERNATING between the
sides, a device window --calls back-to-back calls between two events on the stream, a twin or host window one call under
perf_counter; the figure of a window is its time per call, the reported figure the median over the windows (min and max
beside it).  The Python side is timed on the first --host-patterns patterns of a shape and reported per pattern as well
(host_ms_per_pattern): the loop is linear in the patterns.  On UCC-en the device results of every pattern timed on the host
are compared with the plain evaluator of tests/vocab_match_cases.py before anything is timed, and on every shape with the
Python side's; the twin's results are compared with the device form's for ALL patterns.  On the synthetic shapes the Python
side runs once: the comparison run is its window.
Prints ONE JSON line.

    python scripts/bench_vocab_match.py [--windows 5] [--calls 20] [--host-patterns 16] [--synthetic 1000000]
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

from bench_phrase_scope import dev_arr, report  # noqa: E402
from bench_union_lists import window_ms  # noqa: E402


def device_step(torch, nat, index, members, cap):
    """(call, read, work bytes) of the device step over `members` (Wildcards / Fuzzys)."""
    dev = torch.device("cuda", 0)
    cp, ptr, kind, arg = nat.VocabIndex.pack_patterns([m.native_pattern() for m in members])
    n = len(members)
    t = [dev_arr(torch, cp.view(np.int32), "int32"), dev_arr(torch, ptr, "int64"), dev_arr(torch, kind, "int32"),
         dev_arr(torch, arg, "int32")]
    ids = torch.zeros(n * cap, dtype=torch.int32, device=dev)
    dist = torch.zeros(n * cap, dtype=torch.uint8, device=dev)
    n_match = torch.zeros(n, dtype=torch.int64, device=dev)
    wb = nat.vocab_match_plan(index.n_terms, n)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        index.match_device(*[x.data_ptr() for x in t], n, int(cp.size), cap, ids.data_ptr(), dist.data_ptr(), n_match.data_ptr(),
                           work.data_ptr(), wb, stream)

    def read():
        torch.cuda.synchronize()
        return ids.cpu().numpy().reshape(n, cap), dist.cpu().numpy().reshape(n, cap), n_match.cpu().numpy()
    return call, read, wb, (cp, ptr, kind, arg)


def python_side(tokens, members):
    """[[term ids a member names]] by the package's own host rule, token by token."""
    return [[i for i, t in enumerate(tokens) if m.fits(t)] for m in members]


def wall_ms(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def shape(torch, nat, tokens, members, cap, args, host_patterns, host_windows, VC):
    """One shape.  VC: the plain evaluator, or None — the synthetic shapes are compared with the Python side alone (the
    evaluator's full-matrix loop over 10^6 tokens costs what that side costs, and the tests compare the two)."""
    from legal_rag_amd.retrieval.terms import Wildcard
    index = nat.VocabIndex(tokens, device=0)
    call, read, wb, ops = device_step(torch, nat, index, members, cap)
    call()
    ids, dist, n_match = read()
    host_members = members[:host_patterns]
    ms = {"device": [], "twin": [], "host": []}
    t0 = time.perf_counter()
    want = python_side(tokens, host_members)
    first_host = (time.perf_counter() - t0) * 1e3
    if VC is not None:
        keys = [("w", m.pattern) if isinstance(m, Wildcard) else ("f", m.token, m.edits) for m in host_members]
        ev = VC.evaluate(tokens, keys, cap)
    for p in range(len(host_members)):  # the evaluator first, then the Python side
        if VC is not None:
            assert np.array_equal(ids[p], ev[0][p]) and np.array_equal(dist[p], ev[1][p]) and n_match[p] == ev[2][p], members[p]
        assert n_match[p] == len(want[p]) and ids[p, :min(cap, len(want[p]))].tolist() == want[p][:cap], members[p]
    twin = index.match(*ops, cap)
    assert np.array_equal(twin[0], ids) and np.array_equal(twin[1], dist) and np.array_equal(twin[2], n_match)
    if host_windows == 0:
        ms["host"].append(first_host)  # (a Python loop has nothing to warm up: the comparison run is the window)
    for w in range(args.windows):
        ms["device"].append(window_ms(torch, call, args.calls))
        ms["twin"].append(wall_ms(lambda: index.match(*ops, cap)))
        if w < host_windows:
            ms["host"].append(wall_ms(lambda: python_side(tokens, host_members)))
    host = report(ms["host"])
    out = {"terms": len(tokens), "patterns": len(members), "cells": len(members) * max(1, -(-len(tokens) // nat.VOCAB_TILE_TERMS)),
           "item_cap": cap, "work_bytes": wb, "matches": int(n_match.sum()), "widest": int(n_match.max()),
           "device_three_launches": report(ms["device"]), "twin_wall": report(ms["twin"]),
           "host_patterns_timed": len(host_members), "host_python_loop": host,
           "host_ms_per_pattern": round(host["ms"] / len(host_members), 4)}
    out["host_ms_all_patterns_linear"] = round(out["host_ms_per_pattern"] * len(members), 2)
    index.close()
    return out


def synthetic_tokens(n, seed=0):
    rng = np.random.default_rng(seed)
    seen = {}
    while len(seen) < n:
        lens = rng.integers(3, 15, size=n // 2)
        letters = rng.integers(0, 26, size=int(lens.sum())).astype(np.uint8) + ord("a")
        text = letters.tobytes().decode("ascii")
        at = 0
        for L in lens.tolist():
            seen.setdefault(text[at:at + L])
            at += L
            if len(seen) == n:
                break
    return list(seen)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-windows", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-patterns", type=int, default=16)
    ap.add_argument("--synthetic", type=int, default=1_000_000)
    args = ap.parse_args()
    import torch

    import vocab_match_cases as VC
    from bench_facets import N_QUESTIONS, stems
    from legal_rag_amd import _native as nat
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.retrieval.builders.bm25_builder import tokenize_corpus
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    from legal_rag_amd.retrieval.terms import PREFIX_MAX_TERMS, Fuzzy, Wildcard
    out = {"device": nat.device_name(0), "windows": args.windows, "calls_per_window": args.calls, "tile_terms": nat.VOCAB_TILE_TERMS}

    # ---- UCC-en: the facet benchmark's stems as Fuzzy(stem, edits=1) ----
    chunks = load_chunks_from_dir(str(ROOT / "tests" / "golden" / "corpus"), "law_en.jsonl")
    tdocs, _ = tokenize_corpus(chunks)
    model = BM25Okapi(tdocs)
    tokens = list(model.vocab())
    members = [Fuzzy(s, edits=1) for s in stems(model.vocab(), N_QUESTIONS)]
    out["ucc_en"] = shape(torch, nat, tokens, members, 64, args, args.host_patterns, args.host_windows, VC)

    # ---- synthetic: 10^6 tokens, 1 and 64 patterns ----
    tokens = synthetic_tokens(args.synthetic)
    rng = np.random.default_rng(1)
    base = [tokens[int(i)] for i in rng.integers(0, len(tokens), size=64)]
    members = []
    for j, w in enumerate(base):
        w = w if len(w) > 3 else w + "ab"
        members.append(Fuzzy(w[:2] + w[3:], edits=1) if j % 4 == 0 else Fuzzy(w, edits=2) if j % 4 == 1 else
                       Wildcard(w[:3] + "*") if j % 4 == 2 else Wildcard("*" + w[1:4] + "?" + w[5:] if len(w) > 5 else w[0] + "?" + w[2:]))
    members = list(dict.fromkeys(members))
    out["synthetic_1"] = shape(torch, nat, tokens, members[:1], PREFIX_MAX_TERMS, args, 1, 0, None)
    out["synthetic_64"] = shape(torch, nat, tokens, members, PREFIX_MAX_TERMS, args, min(4, args.host_patterns), 0, None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

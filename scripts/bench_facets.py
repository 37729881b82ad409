"""amdr_facet_counts_device behind the constraint resolvers, next to what a caller does without it, at two shapes:

  ucc-en     tests/golden/corpus/law_en.jsonl cut by the index's own tokeniser; up to 1 168 (the bench question count)
             distinct single-Prefix constraints, counted by section and article_id, top 10.  Device: HybridEngine.term_scopes
             + facet_counts enqueued back to back on one stream (events around --calls of them, the operands' staging copy
             and the outputs' copy into pinned memory included).  Without it: the host twins amdr_union_lists and
             amdr_term_scope for the whole batch (they synchronise and copy every qualifying row back), then np.bincount and
             a sort per constraint and field (host clock).
  synthetic  one scope of 10^6 rows of a 2 x 10^6-row list over 10^3 codes, top 10.  Device: the call alone on a resident
             table (events).  Without it: the rows copied back from the device, np.bincount of their codes and the sort
             (host clock around work that ends synchronised).

Every device result is compared with the numpy result before anything is timed.  Each figure is the median over --windows
windows (min and max beside it), the two sides alternating.  Prints ONE JSON line.

    python scripts/bench_facets.py [--windows 9] [--calls 20]
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

N_QUESTIONS = 1168
TOP = 10


def report(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5)}


def device_window(torch, call, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def host_window(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def alternate(torch, device_call, host_call, windows, calls):
    device_call(), host_call()
    torch.cuda.synchronize()
    dev, host = [], []
    for _ in range(windows):
        dev.append(device_window(torch, device_call, calls))
        host.append(host_window(host_call))
    return dev, host


def stems(vocab, count):
    """Up to `count` distinct stems of 3 to 6 letters that name 2 to 64 vocabulary tokens, each expansion once."""
    words = sorted(w for w in vocab if w.isalpha())
    seen, out = set(), []
    for L in (4, 5, 3, 6):
        for stem in sorted({w[:L] for w in words if len(w) >= L}):
            ids = tuple(w for w in words if w.startswith(stem))
            if 2 <= len(ids) <= 64 and ids not in seen:
                seen.add(ids)
                out.append(stem)
    return out[:count]


def host_counts(rows_of, columns, n_codes):
    """What a caller computes from rows copied back: per constraint and field np.bincount and the (count, code) order."""
    out = []
    for rows in rows_of:
        per_field = []
        for col, nc in zip(columns, n_codes):
            c = col[rows]
            named = c[(c >= 0) & (c < nc)]
            per = np.bincount(named, minlength=nc)
            have = np.flatnonzero(per)
            order = have[np.lexsort((have, -per[have]))][:TOP]
            per_field.append((order, per[order], have.size, int(c.size - named.size)))
        out.append((rows.size, per_field))
    return out


def same(got, want):
    total, missing, distinct, code, count = got
    for p, (n, per_field) in enumerate(want):
        if total[p] != n:
            return False
        for f, (order, cnt, d, miss) in enumerate(per_field):
            k = order.size
            if (distinct[p, f], missing[p, f]) != (d, miss) or code[p, f, :k].tolist() != order.tolist() \
                    or count[p, f, :k].tolist() != cnt.tolist() or (code[p, f, k:] != -1).any():
                return False
    return True


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    import torch

    from legal_rag_amd import _native as nat
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.retrieval.builders.bm25_builder import tokenize_corpus
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    from legal_rag_amd.retrieval.engine import HybridEngine
    from legal_rag_amd.retrieval.scope import ScopeResolver
    from legal_rag_amd.retrieval.terms import Prefix, Terms, pack
    assert torch.cuda.is_available(), "bench_facets.py needs the GPU (no fallback)"
    dev = torch.device("cuda", 0)
    out = {"device": nat.device_name(0), "windows": args.windows, "calls_per_window": args.calls, "top": TOP}

    # ---- UCC-en: single-Prefix constraints, counted by section and article ----
    chunks = load_chunks_from_dir(str(ROOT / "tests" / "golden" / "corpus"), "law_en.jsonl")
    tdocs, _ = tokenize_corpus(chunks)
    model = BM25Okapi(tdocs)
    tp, pd, pt, idf, dl = model.to_csr()
    gi = nat.BM25Index(tp, pd, pt, idf, dl, float(model.avgdl))
    fields = ("section", "article_id")
    cols, values = ScopeResolver(chunks).code_columns(fields)
    n_codes = [len(v) for v in values]
    picked = stems(model.vocab(), N_QUESTIONS)
    pairs = [(None, Terms(all_of=[Prefix(s)])) for s in picked]
    tt = pack(pairs, model.vocab(), model._doc_frequencies(), int(model.corpus_size), None, model.sorted_vocab())
    assert tt.n_cons == len(picked) and tt.n_phr == tt.n_near == tt.n_cspan == 0
    eng = HybridEngine(None, gi, None, device=0)
    fetch = []

    def device_call():
        table, _ = eng.term_scopes(tt)
        fetch[:] = [eng.facet_counts(table, cols, n_codes, TOP)]

    host_out = []

    def host_call():
        lp, docs, st = gi.union_lists(*tt.union_ops, tt.union_rows_cap)
        sp, rows, status = gi.term_scope(tt.ops, tt.cand_max, tt.rows_cap, lists=(lp, docs))
        host_out[:] = [host_counts([rows[sp[p]:sp[p + 1]] for p in range(tt.n_cons)], cols, n_codes)]
    device_call(), host_call()
    assert same(fetch[0](), host_out[0]), "device and host counts differ on UCC-en"
    d_ms, h_ms = alternate(torch, device_call, host_call, args.windows, args.calls)
    rows_total = int(sum(n for n, _ in host_out[0]))
    out["ucc_en"] = {"docs": len(chunks), "constraints": tt.n_cons, "unions": tt.n_union, "fields": dict(zip(fields, n_codes)),
                     "qualifying_rows": rows_total, "cand_max": int(tt.cand_max),
                     "device_term_scopes_plus_facet_counts": report(d_ms), "host_twins_plus_bincount": report(h_ms)}

    # ---- synthetic: one scope of 10^6 rows over 10^3 codes ----
    rng = np.random.default_rng(0)
    n_rows, n_scope, nc = 2_000_000, 1_000_000, 1000
    rows = np.sort(rng.choice(n_rows, size=n_scope, replace=False)).astype(np.int64)
    codes = rng.integers(0, nc, size=(1, n_rows)).astype(np.int32)
    codes[0, rng.random(n_rows) < 0.05] = -1
    sp_d = torch.tensor([0, n_scope], dtype=torch.int64, device=dev)
    rows_d, codes_d = torch.from_numpy(rows).to(dev), torch.from_numpy(codes).to(dev)
    table = (sp_d, rows_d, None, 1, n_scope)

    def synth_device():
        fetch[:] = [eng.facet_counts(table, codes_d, [nc], TOP)]

    def synth_host():
        host_out[:] = [host_counts([rows_d.cpu().numpy()], codes, [nc])]
    synth_device(), synth_host()
    assert same(fetch[0](), host_out[0]), "device and host counts differ on the synthetic scope"
    d_ms, h_ms = alternate(torch, synth_device, synth_host, args.windows, args.calls)
    out["synthetic"] = {"rows_in_list": n_rows, "rows_in_scope": n_scope, "codes": nc, "tiles": -(-n_scope // nat.FACET_TILE_ROWS),
                        "device_facet_counts": report(d_ms), "rows_copied_back_plus_bincount": report(h_ms)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

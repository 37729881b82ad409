"""amdr_unit_spans_device (Within: same sentence, same paragraph) at two shapes, and what the break flags cost:

  ucc-en     tests/golden/corpus/law_en.jsonl cut by the index's own tokeniser, the break flags by retrieval/units.py.  The
             first two known tokens of each of the 1 168 evaluation questions as one Within constraint (the four kinds in
             turn), packed as ONE batch, resolved and counted on the device: HybridEngine.term_scopes (the unit step and the
             term step, six launches) between two events, and the unit step's three launches alone.  Beside it the Python
             evaluator (Within.within over the same documents, host clock).  The device counts are compared with the
             evaluator's before anything is timed.
  flags      ensure_breaks' work after a one-article replace (one text cut, one concatenation of the cached flags, the
             upload of 1 B per token) next to a full re-cut of the corpus (host clock; both end synchronised).
  synthetic  10^6 documents of 50 tokens over 200 terms with a sentence break every 12 tokens on average, 64 two-token
             items: the unit step's three launches (events), set against the count kernel's algorithmic bytes — 5 B per
             token of the surviving documents (the conjunction's), each read once.

Each figure is the median over --windows windows (min and max beside it).  Prints ONE JSON line.

    python scripts/bench_unit_spans.py [--windows 9] [--calls 20] [--no-synthetic]
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


def report(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5)}


def device_windows(torch, call, windows, calls):
    call()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def host_windows(call, windows):
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def dev_arr(torch, a, dtype):
    t = torch.zeros(max(int(np.size(a)), 1), dtype=getattr(torch, dtype), device="cuda:0")
    if np.size(a):
        t[:np.size(a)].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def unit_step(torch, nat, gi, ops, n, cand_max, rows_cap):
    """(call, read) of amdr_unit_spans_device over plain-token items on resident operands."""
    o = [dev_arr(torch, x, dt) for x, dt in zip(ops, ("int64", "int32", "int32"))]
    lp = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
    dc = torch.zeros(max(rows_cap, 1), dtype=torch.int32, device="cuda:0")
    st = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda:0")
    wb = nat.unit_spans_plan(n, cand_max)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        gi.unit_spans_device(*[x.data_ptr() for x in o], n, 0, 0, 0, 0, 0, cand_max, rows_cap, lp.data_ptr(), dc.data_ptr(),
                             st.data_ptr(), work.data_ptr(), wb, stream)

    def read():
        torch.cuda.synchronize()
        return lp.cpu().numpy(), dc.cpu().numpy(), st.cpu().numpy()
    return call, read, wb


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-synthetic", action="store_true")
    args = ap.parse_args()
    import torch

    from legal_rag_amd import _native as nat
    from legal_rag_amd import text
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.evaluation import synthetic_queries
    from legal_rag_amd.retrieval.builders.bm25_builder import tokenize_corpus
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    from legal_rag_amd.retrieval.engine import HybridEngine
    from legal_rag_amd.retrieval.terms import Terms, Within, pack
    from legal_rag_amd.retrieval.units import break_flags
    assert torch.cuda.is_available(), "bench_unit_spans.py needs the GPU (no fallback)"
    out = {"device": nat.device_name(0), "windows": args.windows, "calls_per_window": args.calls}

    # ---- UCC-en ----
    chunks = load_chunks_from_dir(str(ROOT / "tests" / "golden" / "corpus"), "law_en.jsonl")
    tdocs, _ = tokenize_corpus(chunks)
    model = BM25Okapi(tdocs)
    tp, pd, pt, idf, dl = model.to_csr()
    gi = nat.BM25Index(tp, pd, pt, idf, dl, float(model.avgdl))
    doc_ptr, tokens = model.token_stream(tdocs)
    gi.set_tokens(doc_ptr, tokens)
    flags = [break_flags(c.text, toks, True)[0] for c, toks in zip(chunks, tdocs)]
    gi.set_breaks(np.concatenate(flags))
    vocab = model.vocab()
    withins = []
    for i, (q, _, _) in enumerate(synthetic_queries(chunks, seed=0)):
        known = list(dict.fromkeys(t for t in text.tokenize_en(q) if t in vocab))[:2]
        if len(known) == 2:
            withins.append(Within(*known, unit="paragraph" if i & 2 else "sentence", ordered=bool(i & 1)))
    tt = pack([(None, Terms(all_of=[w])) for w in withins], vocab, model._doc_frequencies(), int(model.corpus_size))
    eng = HybridEngine(None, gi, None, device=0)
    held = []

    def chain():
        held[:] = [eng.term_scopes(tt)]
    chain()
    torch.cuda.synchronize()
    table, status = held[0]
    assert not status.cpu().numpy().any()
    counts = np.diff(table[0].cpu().numpy())[np.asarray(tt.qscope)]
    brk = [f.tolist() for f in flags]

    def evaluator():
        return [sum(1 for toks, b in zip(tdocs, brk) if w.within(toks, b)) for w in tt.units]
    want = evaluator()
    by_unit = {w: n for w, n in zip(tt.units, want)}
    assert counts.tolist() == [by_unit[w] for w in withins], "device and evaluator counts differ on UCC-en"
    u_call, u_read, u_wb = unit_step(torch, nat, gi, tt.unit_ops, tt.n_unit, tt.unit_cand_max, tt.unit_rows_cap)
    u_call()
    assert np.diff(u_read()[0]).tolist() == want and not u_read()[2].any()
    out["ucc_en"] = {"docs": len(chunks), "tokens": int(tokens.size), "questions_with_two_known_tokens": len(withins),
                     "distinct_unit_items": tt.n_unit, "constraints": tt.n_cons, "unit_cand_max": int(tt.unit_cand_max),
                     "qualifying_rows": int(sum(want)), "unit_work_bytes": u_wb,
                     "unit_step_three_launches": report(device_windows(torch, u_call, args.windows, args.calls)),
                     "term_scopes_unit_and_term_steps": report(device_windows(torch, chain, args.windows, args.calls)),
                     "python_evaluator": report(host_windows(evaluator, 3))}

    # ---- the flags: one article re-cut against the whole corpus ----
    def full_recut():
        fl = [break_flags(c.text, text.tokenize_en(c.text), True)[0] for c in chunks]
        gi.set_breaks(np.concatenate(fl))

    longest = int(np.argmax([len(t) for t in tdocs]))

    def one_article():
        cached = list(flags)
        cached[longest] = break_flags(chunks[longest].text, text.tokenize_en(chunks[longest].text), True)[0]
        gi.set_breaks(np.concatenate(cached))
    out["flags"] = {"tokens": int(tokens.size), "longest_article_tokens": len(tdocs[longest]),
                    "one_article_cut_concatenate_upload": report(host_windows(one_article, args.windows)),
                    "full_recut_and_upload": report(host_windows(full_recut, args.windows))}

    # ---- synthetic ----
    if not args.no_synthetic:
        rng = np.random.default_rng(0)
        n_docs, per, V, n_items = 1_000_000, 50, 200, 64
        stream = rng.integers(0, V, size=n_docs * per, dtype=np.int32)
        sbrk = (rng.random(stream.size) < 1 / 12).astype(np.uint8)
        sbrk[(sbrk == 1) & (rng.random(stream.size) < 0.25)] = 3
        s_ptr = np.arange(0, n_docs * per + 1, per, dtype=np.int64)
        key = stream.astype(np.int64) * n_docs + np.repeat(np.arange(n_docs, dtype=np.int64), per)
        uniq, tf = np.unique(key, return_counts=True)  # (term, doc) ascending: the term-major CSR
        s_tp = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(np.bincount((uniq // n_docs).astype(np.int64), minlength=V), out=s_tp[1:])
        sgi = nat.BM25Index(s_tp, (uniq % n_docs).astype(np.int32), tf.astype(np.int32), np.ones(V), np.full(n_docs, per, np.int32),
                            float(per))
        sgi.set_tokens(s_ptr, stream)
        sgi.set_breaks(sbrk)
        pairs = [(int(a), int(b)) for a, b in rng.choice(V, size=(n_items, 2), replace=False)]
        has = np.zeros((V, n_docs), dtype=bool)
        has[stream, np.repeat(np.arange(n_docs), per)] = True
        survivors = [int(np.count_nonzero(has[a] & has[b])) for a, b in pairs]
        dfs = np.diff(s_tp)
        bound = [int(min(dfs[a], dfs[b])) for a, b in pairs]
        ops = (np.arange(0, 2 * n_items + 1, 2, dtype=np.int64), np.asarray(pairs, np.int32).ravel(),
               (np.arange(n_items) % 4).astype(np.int32))
        s_call, s_read, s_wb = unit_step(torch, nat, sgi, ops, n_items, max(bound), int(sum(bound)))
        s_call()
        lp, dc, st = s_read()
        assert not st.any()
        # item 0 against numpy: the sentence ids of both tokens' positions meet
        unit_id = np.cumsum((sbrk & 1) | (np.arange(stream.size) % per == 0))
        a, b = pairs[0]
        want0 = np.unique(np.intersect1d(unit_id[stream == a], unit_id[stream == b], assume_unique=False))
        docs0 = np.unique(np.searchsorted(unit_id, want0, side="left") // per)
        assert dc[lp[0]:lp[1]].tolist() == docs0.tolist(), "the synthetic list of item 0 differs from numpy"
        ms = device_windows(torch, s_call, args.windows, max(args.calls // 4, 3))
        nbytes = 5 * per * int(sum(survivors))
        med = statistics.median(ms)
        out["synthetic"] = {"docs": n_docs, "tokens": int(stream.size), "terms": V, "items": n_items, "cand_max": max(bound),
                            "surviving_documents": int(sum(survivors)), "rows": int(lp[-1]), "work_bytes": s_wb,
                            "algorithmic_bytes": nbytes, "unit_step_three_launches": report(ms),
                            "algorithmic_gb_per_s": round(nbytes / med / 1e6, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

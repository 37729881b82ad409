"""amdr_class_spans_device: the event time of the class step's three launches (count, scan, write) next to the span step's
(amdr_span_lists_device) TAKEN IN THE SAME PROCESS on the same pairs, at this shape:

  ucc-en   tests/golden/corpus/law_en.jsonl cut by the index's own tokeniser: the 64 two-token unordered Nears at distance 5
           of §4.19 / §4.20 through the span step; beside them the 64 two-slot NearOf(Prefix, Prefix, distance=5) whose stems
           are those tokens cut short (a stem names the token and what else starts with it), the classes' lists written once
           by the union step into the array the class step continues.

Method: the operands are resident; every step runs once untimed; then --windows windows per step, ALTERNATING between the
steps, each window --calls back-to-back calls between two events on the stream; the figure of a window is its time per call,
the reported figure the median over the windows (min and max beside it).  The lists are compared with NearOf.within over
the articles' own tokens before anything is timed.  Prints ONE JSON line.

    python scripts/bench_class_span.py [--windows 9] [--calls 50]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))

from bench_phrase_scope import dev_arr, report  # noqa: E402
from bench_union_lists import alternate, span_step  # noqa: E402


def members_of(pairs, words, vocab):
    """Per pair two members whose token sets are equal or disjoint and of which one at least names two tokens or more (the
    item is then a class span, not a plain Near): Prefix of each token less its last 2, 3, 4 or 1 letters (three letters at
    least), the first cut that gives such a pair."""
    from legal_rag_amd.retrieval.terms import Prefix
    ordered = sorted(vocab)
    ids = lambda stem: frozenset(vocab[w] for w in ordered if w.startswith(stem))  # noqa: E731
    out = []
    for a, b in pairs:
        for cut in (2, 3, 4, 1):
            sa, sb = (w[:max(3, len(w) - cut)] for w in (words[a], words[b]))
            A, B = ids(sa), ids(sb)
            if (A == B or not A & B) and max(len(A), len(B)) >= 2:
                out.append((Prefix(sa), Prefix(sb)))
                break
        else:  # (one token is a stem of the other whatever the cut, 'i' and 'including'): the shorter one stays a plain token
            short, long_ = sorted((words[a], words[b]), key=len)
            fits = [st for st in (long_[:max(3, len(long_) - cut)] for cut in (2, 3, 4, 1, 0)) if vocab[short] not in ids(st)]
            wide = [st for st in fits if len(ids(st)) >= 2] or fits
            m = Prefix(wide[0]) if wide else long_  # (nothing fits: the plain Near of the pair)
            out.append((m, short) if long_ == words[a] else (short, m))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    import torch

    from legal_rag_amd import _native as nat
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.retrieval.builders.bm25_builder import tokenize_corpus
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    from legal_rag_amd.retrieval.terms import NearOf, Terms, pack
    dev = torch.device("cuda", 0)
    out = {"device": nat.device_name(0), "windows": args.windows, "calls_per_window": args.calls}

    chunks = load_chunks_from_dir(str(ROOT / "tests" / "golden" / "corpus"), "law_en.jsonl")
    tdocs, _ = tokenize_corpus(chunks)
    model = BM25Okapi(tdocs)
    tp, pd, pt, idf, dl = model.to_csr()
    gi = nat.BM25Index(tp, pd, pt, idf, dl, float(model.avgdl))
    doc_ptr, tokens = model.token_stream(tdocs)
    gi.set_tokens(doc_ptr, tokens)
    dfs = np.diff(tp)
    vocab = model.vocab()
    words = {i: w for w, i in vocab.items()}
    # the pairs of scripts/bench_union_lists.py: adjacent tokens of 20 to 300 articles each
    inside = np.ones(tokens.size - 1, dtype=bool)
    cut = doc_ptr[1:-1]
    inside[cut[(cut > 0) & (cut < tokens.size)] - 1] = False
    a, b = tokens[:-1][inside], tokens[1:][inside]
    ok = (dfs[a] >= 20) & (dfs[a] <= 300) & (dfs[b] >= 20) & (dfs[b] <= 300) & (a != b)
    pairs = np.unique(np.stack([a[ok], b[ok]], axis=1), axis=0)
    pairs = [(int(x), int(y)) for x, y in pairs[np.sort(np.random.default_rng(0).choice(pairs.shape[0], size=64, replace=False))]]
    bound = [int(min(dfs[x], dfs[y])) for x, y in pairs]
    s_call, s_read, s_wb = span_step(torch, nat, gi, pairs, 5, bound)

    members = members_of(pairs, words, vocab)
    items = [NearOf(ma, mb, distance=5) for ma, mb in members]
    tt = pack([(None, Terms(all_of=[it])) for it in items], vocab, model._doc_frequencies(), int(model.corpus_size), None,
              model.sorted_vocab())
    n_u, n_c, n_s = tt.n_union, tt.n_cspan, tt.n_phr + tt.n_near
    assert n_c >= len(pairs) // 2 and tt.n_phr == 0  # (a pair whose members name one token each stays a plain Near)
    first = len(vocab) + n_s
    c_ptr, c_slots, c_kind, c_dist = tt.cspan_ops
    c_slots = np.where(c_slots >= first, c_slots - n_s, c_slots)  # the unions alone stand before: cls_first = 0
    ops = [dev_arr(torch, x, dt) for x, dt in zip((c_ptr, c_slots, c_kind, c_dist), ("int64", "int32", "int32", "int32"))]
    up, ut = dev_arr(torch, tt.union_ops[0], "int64"), dev_arr(torch, tt.union_ops[1], "int32")
    cap = tt.union_rows_cap + tt.cspan_rows_cap
    lp = torch.zeros(n_u + n_c + 1, dtype=torch.int64, device=dev)
    dc = torch.zeros(max(cap, 1), dtype=torch.int32, device=dev)
    st = torch.zeros(n_u + n_c, dtype=torch.int32, device=dev)
    u_wb, c_wb = nat.union_lists_plan(n_u, gi.n_docs), nat.class_spans_plan(n_c, tt.cspan_cand_max)
    u_work = torch.empty(max(u_wb, 1), dtype=torch.uint8, device=dev)
    c_work = torch.empty(max(c_wb, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def u_call():
        gi.union_lists_device(up.data_ptr(), ut.data_ptr(), n_u, 0, cap, lp.data_ptr(), dc.data_ptr(), st.data_ptr(),
                              u_work.data_ptr(), u_wb, stream)

    def c_call():
        gi.class_spans_device(*[x.data_ptr() for x in ops], n_c, up.data_ptr(), ut.data_ptr(), n_u, 0, n_u, tt.cspan_cand_max, cap,
                              lp.data_ptr(), dc.data_ptr(), st.data_ptr() + 4 * n_u, c_work.data_ptr(), c_wb, stream)

    def both():
        u_call()
        c_call()
    both(), s_call()
    torch.cuda.synchronize()
    got_ptr, got_docs = lp.cpu().numpy(), dc.cpu().numpy()
    assert not st.cpu().numpy().any() and not s_read()[2].any()
    rows = 0
    for c, item in enumerate(tt.cspans):  # against the reference, before anything is timed
        want = [d for d, toks in enumerate(tdocs) if item.within(toks)]
        assert got_docs[got_ptr[n_u + c]:got_ptr[n_u + c + 1]].tolist() == want, item
        rows += len(want)
    ms = alternate(torch, {"class": c_call, "span": s_call, "union_and_class": both}, args.windows, args.calls)
    out["ucc_en"] = {"docs": int(doc_ptr.size - 1), "terms": int(dfs.size), "pairs": len(pairs), "class_spans": n_c,
                     "members": [repr(m) for m in members[:4]], "classes": n_u, "class_member_ids": int(tt.union_ops[1].size),
                     "class_rows": int(got_ptr[n_u]), "class_span_rows": rows, "class_span_cand_max": int(tt.cspan_cand_max),
                     "class_work_bytes": c_wb, "class_step_three_launches": report(ms["class"]),
                     "union_and_class_six_launches": report(ms["union_and_class"]),
                     "nears": len(pairs), "near_distance": 5, "span_rows": int(s_read()[0][-1]), "span_work_bytes": s_wb,
                     "span_step_three_launches": report(ms["span"])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

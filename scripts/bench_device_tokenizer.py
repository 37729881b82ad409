"""The BM25 query side of the headline step on the host and on the device.

UCC-en, 1 168 synthetic queries tiled 32 x = 37 376 per step (bench.py's headline batch), dense + BM25 + fusion top-10.
Prints ONE JSON line with the median over timed windows (ms per step) of:
  host_tokeniser          Tokenizer.encode (pointer views -> amdr_tokenizer_encode_ptrs on the worker pool) alone
  host_text_in_step       host tokeniser + pinned H2D of the CSR + kernels (bench.py --full's with_tokenisation)
  pack_h2d_device_tok     pointer views + amdr_tokenizer_pack into pinned memory + ONE H2D + the device tokeniser
  device_text_in_step     the same + channels + fusion, eager
  device_text_in_graph    bytes already in the captured step's buffers: graph replay of tokeniser + channels + fusion
  resident_csr_step       the headline: term-id CSR resident in HBM, kernels only (the reference point)
and whether the device CSR and the fused ids equal the host path's.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` with --steps small (a run of its own; tracing slows the host).

    python scripts/bench_device_tokenizer.py [--steps 20] [--windows 5] [--repeat 32]
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--repeat", type=int, default=32)
    a = ap.parse_args()

    import torch

    import bench
    from legal_rag_amd import _native

    if not torch.cuda.is_available():
        raise SystemExit("bench_device_tokenizer: no GPU (this script measures the device path; nothing to fall back to)")
    dev = torch.device("cuda", 0)
    W = bench.build_corpus("en")
    R = bench.Resident(torch, W, 0, rep=a.repeat)
    K = 10
    params = _native.make_fuse_params(min_final_score=0.2)
    texts = [q for q, _, _ in W["queries"]] * a.repeat
    nq = len(texts)
    tok = _native.Tokenizer(list(W["bm"].vocab().keys()))
    eng = R.eng
    eng.tokenizer = _native.DeviceTokenizer(tok, device=0)
    ptrs, lens, total, _, keep = _native.utf8_views(texts)
    eng.reserve(nq, K, int(R.q_ptr_h[-1]), bytes_max=total)

    def timed(step):
        return bench.window_stats(bench.timed_windows(torch, None, 1, dev, step, a.steps, a.warmup, a.windows), a.steps)

    last = {}

    def resident():
        last["res"] = R.search_batch(params, K)

    def host_tok():
        tok.encode(texts)

    def host_step():
        ti, tp, _ = tok.encode(texts)
        qp_d, qt_d = eng.upload_csr(tp, ti if ti.size else np.zeros(1, np.int32))
        last["host"] = eng.search_batch(params, K, q_emb=R.q_emb, q_terms=qt_d, q_ptr=qp_d)

    def dev_tok():
        p, l_, t, _, k_ = _native.utf8_views(texts)
        blob_d, offs_d = eng.upload_text(p, l_, t)
        last["csr"] = eng.tokenize_device(blob_d, offs_d)

    def dev_step():
        p, l_, t, _, k_ = _native.utf8_views(texts)
        blob_d, offs_d = eng.upload_text(p, l_, t)
        last["dev"] = eng.search_batch(params, K, q_emb=R.q_emb, q_text=(blob_d, offs_d))

    out = {"workload": "UCC-en dense+BM25 hybrid top-10, text-in", "queries_per_step": nq, "blob_bytes": total}
    out["resident_csr_step"] = timed(resident)
    ref_ids = last["res"].ids.clone()
    out["host_tokeniser"] = timed(host_tok)
    out["host_text_in_step"] = timed(host_step)
    out["pack_h2d_device_tok"] = timed(dev_tok)
    tt, tp, tf = last["csr"]
    torch.cuda.synchronize()
    ti, tph, _ = tok.encode(texts)
    out["device_csr_equals_host"] = bool(np.array_equal(tp.cpu().numpy(), tph)
                                         and np.array_equal(tt[: len(ti)].cpu().numpy(), ti))
    out["device_text_in_step"] = timed(dev_step)
    torch.cuda.synchronize()
    out["device_fused_ids_equal_resident"] = bool(torch.equal(last["dev"].ids, ref_ids))

    # the captured text-in step: the bytes sit in the graph's own input buffers (a caller writes them there)
    blob_d, offs_d = eng.upload_text(ptrs, lens, total)
    blob_g, offs_g = blob_d.clone(), offs_d.clone()
    graph, gres = eng.capture(params, K, q_emb=R.q_emb, q_text=(blob_g, offs_g))
    out["device_text_in_graph"] = timed(graph.replay)
    torch.cuda.synchronize()
    out["graph_fused_ids_equal_resident"] = bool(torch.equal(gres.ids, ref_ids))
    t0 = time.perf_counter()
    for _ in range(20):
        _native.utf8_views(texts)
    out["utf8_views_ms"] = (time.perf_counter() - t0) / 20 * 1e3
    med = {k: v["median"] for k, v in out.items() if isinstance(v, dict)}
    out["medians_ms"] = med
    out["queries_per_s"] = {k: nq / (v * 1e-3) for k, v in med.items() if k.endswith(("step", "graph"))}
    del keep
    print(json.dumps(out))


if __name__ == "__main__":
    main()

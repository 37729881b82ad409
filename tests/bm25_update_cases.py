"""What the tests of amdr_bm25_add and amdr_bm25_remove share (test_bm25_add_gpu.py, test_bm25_remove_gpu.py and the two
test_bm25_*_rule_host.py): generated documents, the handle of a fitted model, the comparisons of an updated handle with a
freshly created one through every entry point, and the build of a host check program.  A plain module, not a conftest."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

LENS = (1, 2, 5, 17, 40, 90)
SEARCHES = ((1, 1), (7, 10), (9, 17), (24, 80))  # (nq, k)
N_ZIPF = 400
CSRC = Path(__file__).resolve().parent.parent / "legal-rag_amd" / "csrc"


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


def make_docs(rng, n, lead=lambda i: ()):
    """n token lists: "all" in every one (the first term: its list is postings 0 .. n-1), Zipfian terms z0 .. z399 with
    tf 1-9, lengths from LENS; lead(i) -> the tokens that follow "all" in document i."""
    docs = []
    for i in range(n):
        head = ["all"] + list(lead(i))
        want = max(int(rng.choice(LENS)), len(head))
        doc = list(head)
        while len(doc) < want:
            z = min(int(rng.zipf(1.3)) - 1, N_ZIPF - 1)
            doc.extend([f"z{z}"] * int(rng.integers(1, 10)))
        docs.append(doc[:want])
    return docs


def fit(docs):
    from legal_rag_amd.bm25_model import BM25Okapi
    return BM25Okapi(docs)


def index_of(nat, model):
    term_ptr, post_doc, post_tf, idf, doc_len = model.to_csr()
    return nat.BM25Index(term_ptr, post_doc, post_tf, idf, doc_len, float(model.avgdl), float(model.k1), float(model.b))


def same_arrays(a, b):
    assert len(a) == len(b)
    for j, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"array {j} differs"


def queries_for(rng, V, n=24):
    """Term-id queries: unknown ids, repeats, the term of every document (id 0) and the last (newest) terms among them."""
    qs = [[int(t) for t in rng.integers(-1, V, size=int(rng.integers(0, 13)))] for _ in range(n)]
    qs[0] = [0, V - 1, 0, -1, max(V - 2, 0)]
    qs[1] = []
    qs[2] = [V - 1]
    return qs


def same_pair(a, b, what):
    (sa, ia), (sb, ib) = a, b
    assert np.array_equal(ia, ib), what
    assert sa.tobytes() == sb.tobytes(), what


def assert_same_results(nat, g, f, qs, at):
    """at: the document id where the update happened — the seam of an add (the first added document) or the closed gap of
    a remove (the new id of the first survivor behind a removed document); the scope holds documents of both sides."""
    import torch
    dev = torch.device("cuda", 0)
    n = g.n_docs
    for nq, k in SEARCHES:
        same_pair(g.search(qs[:nq], k), f.search(qs[:nq], k), ("search", nq, k))
    assert g.get_scores(qs).tobytes() == f.get_scores(qs).tobytes()
    # "_device" search inside a reserve: no workspace grows
    qt_h, qp_h = nat.BM25Index.pack_queries(qs)
    qt, qp = torch.from_numpy(qt_h).to(dev), torch.from_numpy(qp_h).to(dev)
    out = []
    for h in (g, f):
        h.reserve(24, 80, int(qt_h.size))
        for nq, k in SEARCHES:
            s = torch.empty((nq, k), dtype=torch.float64, device=dev)
            i = torch.empty((nq, k), dtype=torch.int64, device=dev)
            g0 = nat.workspace_growths()
            h.search_device(qt.data_ptr(), qp.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
            assert nat.workspace_growths() == g0, ("search_device grew a workspace", nq, k)
            torch.cuda.synchronize()
            out.append((s.cpu().numpy(), i.cpu().numpy()))
    half = len(out) // 2
    for j in range(half):
        same_pair(out[j], out[half + j], ("search_device", SEARCHES[j]))
        same_pair(out[j], g.search(qs[:SEARCHES[j][0]], SEARCHES[j][1]), ("search_device against search", SEARCHES[j]))
    at = min(max(at, 0), n - 1)
    rows = np.asarray(sorted({0, max(at - 2, 0), max(at - 1, 0), at, min(at + 1, n - 1), n - 1}), dtype=np.int64)
    ws = nat.ScopeWorkspace()
    table = (np.asarray([0, rows.size], dtype=np.int64), rows, [0] * 7)
    a, b = (ws.bm25_search(h, qs[:7], *table, 4) for h in (g, f))
    ws.close()
    same_pair(a, b, "scoped search")
    assert set(a[1][0].tolist()) - {-1} <= set(rows.tolist())


def assert_same_serving_step(nat, g, f, qs, d=64):
    """HybridEngine.search_batch of 1-4 queries (amdr_hybrid_small_device on <= 2 048 documents: ONE launch)."""
    import torch
    from test_hybrid_small_gpu import _run, _same
    from legal_rag_amd.retrieval.engine import HybridEngine
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(g.n_docs)
    X = rng.standard_normal((g.n_docs, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    eg, ef = (HybridEngine(nat.DenseIndex(X), h, None) for h in (g, f))
    params = nat.make_fuse_params(method="weighted_sum", min_final_score=0.0)
    for nq, k in ((1, 10), (3, 5)):
        if k > g.n_docs:
            k = g.n_docs
        q = rng.standard_normal((nq, d)).astype(np.float32)
        qt_h, qp_h = nat.BM25Index.pack_queries(qs[:nq])
        Q = torch.from_numpy(q).to(dev)
        qt = torch.from_numpy(np.concatenate([qt_h, np.zeros(1, np.int32)])).to(dev)
        qp = torch.from_numpy(qp_h).to(dev)
        a, b = _run(eg, params, k, Q, qt, qp, True), _run(ef, params, k, Q, qt, qp, True)
        _same(a, b, ("serving step", nq, k))
        same_pair((a["bm25_scores"], a["bm25_ids"]), g.search(qs[:nq], k), ("serving step against search", nq, k))


def build_check_program(tmp_path_factory, name):
    """csrc/<name>.cpp as a program of its own: compiled for the host alone with the address and undefined-behaviour
    sanitizers (host flags only: no device code is built), by the compiler that builds the library."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (Path(hipcc).exists() or shutil.which(hipcc)):
        pytest.fail(f"{hipcc} not found: the host check is compiled with the compiler that builds the library")
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                    "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", str(CSRC / f"{name}.cpp"), "-o", str(exe)],
                   check=True, cwd=str(CSRC))
    return exe

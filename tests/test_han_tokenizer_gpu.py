"""The Han modes of the BM25 query tokeniser on the device (csrc/tokenize.hip over csrc/tokenize_rule.hpp): the CSR of
amdr_tokenizer_encode_device is amdr_tokenizer_encode's for the same bytes — term ids, q_ptr and flags — in the "char"
and the "dict" mode, within the reserve it allocates nothing and can be captured, and HybridRetriever with
query_tokenizer="device" returns for Han queries what query_tokenizer="host" returns, bit for bit."""
import copy
import ctypes as C

import numpy as np
import pytest

import han_adversary as H
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def host_csr(tok, blob: bytes, offs):
    """amdr_tokenizer_encode on (blob, offs): (term_ids, q_ptr, needs_segmenter)."""
    from legal_rag_amd import _native
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    nq = len(offs) - 1
    cap = max(len(blob), 1)
    terms = np.full(cap, -7, dtype=np.int32)
    q_ptr = np.zeros(nq + 1, dtype=np.int64)
    flags = np.zeros(max(nq, 1), dtype=np.int32)
    buf = C.create_string_buffer(blob, max(len(blob), 1))
    rc = _native.load().amdr_tokenizer_encode(tok._h, buf, offs.ctypes.data, nq, terms.ctypes.data, cap,
                                               q_ptr.ctypes.data, flags.ctypes.data)
    assert rc == 0, _native.load().amdr_last_error()
    return terms[: int(q_ptr[-1])], q_ptr, flags[:nq]


def on_device(blob: bytes, offs):
    import torch
    dev = torch.device("cuda", 0)
    nq, cap = len(offs) - 1, max(len(blob), 1)
    b = torch.zeros(cap, dtype=torch.uint8, device=dev)
    if blob:
        b[: len(blob)] = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    o = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).to(dev)
    terms = torch.full((cap,), -7, dtype=torch.int32, device=dev)
    q_ptr = torch.full((nq + 1,), -9, dtype=torch.int64, device=dev)
    flags = torch.full((nq,), -9, dtype=torch.int32, device=dev)
    return b, o, terms, q_ptr, flags


def device_csr(dtok, blob: bytes, offs):
    import torch
    b, o, terms, q_ptr, flags = on_device(blob, offs)
    dtok.reserve(max(len(offs) - 1, 1), max(len(blob), 1))
    dtok.encode_device(b, o, terms, q_ptr, flags, n_bytes=len(blob))
    torch.cuda.synchronize()
    qp = q_ptr.cpu().numpy()
    return terms.cpu().numpy()[: int(qp[-1])], qp, flags.cpu().numpy()


def assert_same(pair, texts):
    tok, dtok = pair
    blob, offs = H.pack(texts)
    ht, hp, hf = host_csr(tok, blob, offs)
    dt, dp, df = device_csr(dtok, blob, offs)
    assert np.array_equal(dp, hp), np.flatnonzero(dp != hp)[:5]
    assert np.array_equal(df, hf), np.flatnonzero(df != hf)[:5]
    assert np.array_equal(dt, ht), np.flatnonzero(dt != ht)[:5]
    assert not hf.any()  # a Han mode flags nothing
    return ht, hp


@pytest.fixture(scope="module")
def law():
    """The fixture corpus, its n-gram dictionary, and per mode (host tokeniser, device copy) over the vocabulary of the
    first 200 chunks cut in that mode plus every key of the fuzz and known-answer dictionaries (so that hits of every
    length occur in the fuzz as well)."""
    from legal_rag_amd import _native, text
    from legal_rag_amd.bm25_model import BM25Okapi
    texts = H.law_zh_texts()
    d = text.load_han_dict(H.ngram_dict_lines(texts))
    extra = [ln.split()[0] for ln in H.fuzz_dict_lines() + H.KNOWN_DICT_LINES] + list("，。 \n") + ["\r\n", "3.5%", "C++"]
    pairs = {}
    for mode, dd in (("char", None), ("dict", d)):
        bm = BM25Okapi([text.han_cut(t, mode, dd) for t in texts[:200]])
        tok = _native.Tokenizer(list(bm.vocab().keys()) + extra, han=dd if mode == "dict" else "char")
        pairs[mode] = (tok, _native.DeviceTokenizer(tok, device=0))
    sents = H.law_zh_sentences(texts, 300)
    return dict(texts=texts, d=d, pairs=pairs, sents=sents)


def fuzz_pair():
    """(host, device) in the dictionary mode over the FUZZ dictionary (exact ties, word buffers), its keys as vocabulary."""
    from legal_rag_amd import _native, text
    d = text.load_han_dict(H.fuzz_dict_lines())
    tok = _native.Tokenizer(list(d.lfreq) + list("aB3，"), han=d)
    return tok, _native.DeviceTokenizer(tok, device=0)


@pytest.mark.parametrize("mode", ["char", "dict"])
def test_device_equals_host_on_adversary_fuzz_and_corpus(law, mode):
    pair = law["pairs"][mode]
    assert_same(pair, H.adversary_texts() + [s for s, _ in H.KNOWN_DICT_ANSWERS])
    assert_same(pair, H.fuzz_texts())
    ht, hp = assert_same(pair, law["sents"])
    assert (ht >= 0).mean() > 0.5 and hp[-1] > 3000  # real hits, not only -1
    if mode == "dict":
        assert (np.diff(hp) < [len(s) for s in law["sents"]]).mean() > 0.9  # words of several characters were cut
        fp = fuzz_pair()
        try:
            ht, _ = assert_same(fp, H.fuzz_texts())  # the dictionary with exact ties and word buffers
            assert (ht >= 0).mean() > 0.5
            assert_same(fp, H.adversary_texts())
        finally:
            fp[1].close()


@pytest.mark.parametrize("mode", ["char", "dict"])
@pytest.mark.parametrize("nq", [1, 255, 256, 257])
def test_batch_sizes_around_the_block_edge(law, mode, nq):
    assert_same(law["pairs"][mode], law["sents"][:nq])


@pytest.mark.parametrize("mode", ["char", "dict"])
def test_unstaged_block_mixed_batch_and_one_long_run(law, mode):
    pair = law["pairs"][mode]
    # 256 queries of about 70 Han characters: the first block's text exceeds the 32 KiB LDS stage and is read from HBM
    run = "".join("".join(law["texts"][:200]).split())
    long_qs = [run[37 * i: 37 * i + 66 + i % 9] for i in range(256)]
    assert len(H.pack(long_qs)[0]) > 32768 * 1.5 and all(len(q) >= 66 for q in long_qs)
    assert_same(pair, long_qs)
    assert_same(pair, long_qs + law["sents"][:100])  # an unstaged block followed by a staged one
    mixed = []
    for i, s in enumerate(law["sents"][:120]):
        mixed += [s, "", "buyer of goods, rate 3.5% C++", " "][: 1 + i % 4]
    assert_same(pair, mixed)
    assert_same(pair, [H.LONG_HAN_RUN])
    assert_same(pair, ["", "", ""])


@pytest.mark.parametrize("mode", ["char", "dict"])
def test_reserve_is_checked_and_nothing_grows_within_it(law, mode):
    import torch
    from legal_rag_amd import _native
    tok, _ = law["pairs"][mode]
    dtok = _native.DeviceTokenizer(tok, device=0)
    try:
        blob, offs = H.pack(law["sents"][:100])
        b, o, terms, q_ptr, flags = on_device(blob, offs)
        dtok.reserve(100, len(blob))
        g0 = _native.workspace_growths()
        dtok.encode_device(b, o, terms, q_ptr, flags, n_bytes=len(blob))
        small, so = H.pack(law["sents"][:7])
        sb, so_d, st, sp, sf = on_device(small, so)
        dtok.encode_device(sb, so_d, st, sp, sf, n_bytes=len(small))
        assert _native.workspace_growths() == g0  # read before anything is synchronised
        torch.cuda.synchronize()
        assert q_ptr.cpu().numpy().tolist() == host_csr(tok, blob, offs)[1].tolist()
        # beyond the reserve: refused, nothing enqueued
        big, bo = H.pack(law["sents"][:101])
        bb, bo_d, bt, bp, bf = on_device(big, bo)
        with pytest.raises(_native.NativeError, match=r"status -1.*exceed the reserve"):
            dtok.encode_device(bb, bo_d, bt, bp, bf, n_bytes=len(big))
        more, mo = H.pack(law["sents"][100:200])
        assert len(more) != len(blob)
        dtok2 = _native.DeviceTokenizer(tok, device=0)
        dtok2.reserve(100, len(more) - 1)
        mb, mo_d, mt, mp, mf = on_device(more, mo)
        with pytest.raises(_native.NativeError, match=r"status -1.*exceed the reserve"):
            dtok2.encode_device(mb, mo_d, mt, mp, mf, n_bytes=len(more))
        dtok2.close()
        torch.cuda.synchronize()
        for t, p, f in ((bt, bp, bf), (mt, mp, mf)):
            assert bool((t == -7).all() and (p == -9).all() and (f == -9).all())
    finally:
        dtok.close()


@pytest.mark.parametrize("mode", ["char", "dict"])
def test_captured_replay_gives_the_eager_result(law, mode):
    """One linear stream, no parallel branches: the four launches of one encode call."""
    import torch
    from legal_rag_amd import _native
    tok, _ = law["pairs"][mode]
    dtok = _native.DeviceTokenizer(tok, device=0)
    try:
        qa, qb = law["sents"][:200], law["sents"][100:300]
        cap = max(len(H.pack(qa)[0]), len(H.pack(qb)[0])) + 64
        blob, offs = H.pack(qa)
        b, o, terms, q_ptr, flags = on_device(blob + b"\0" * (cap - len(blob)), offs)
        dtok.reserve(200, cap)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        g0 = _native.workspace_growths()
        with torch.cuda.graph(g, stream=side):
            dtok.encode_device(b, o, terms, q_ptr, flags, n_bytes=cap)
        assert _native.workspace_growths() == g0

        def replay():
            terms.fill_(-7)
            q_ptr.fill_(-9)
            flags.fill_(-9)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            qp = q_ptr.cpu().numpy()
            return terms.cpu().numpy()[: int(qp[-1])], qp, flags.cpu().numpy()

        for qs in (qa, qb):  # the second batch's bytes go INTO the captured buffers
            nb, no = H.pack(qs)
            b.copy_(torch.from_numpy(np.frombuffer(nb + b"\0" * (cap - len(nb)), dtype=np.uint8).copy()))
            o.copy_(torch.from_numpy(no))
            dt, dp, df = replay()
            ht, hp, hf = host_csr(tok, nb, no)
            assert np.array_equal(dp, hp) and np.array_equal(dt, ht) and np.array_equal(df, hf)
    finally:
        dtok.close()


# ---- HybridRetriever over a Han index ------------------------------------------------------------------------------------
def same_arrays(a, b):
    for key in ("rows", "count", "channel_mask", "zh_exact"):
        if not np.array_equal(a[key], b[key]):
            return False
    if "values" in a and not np.array_equal(a["values"].view(np.int64), b["values"].view(np.int64)):
        return False
    return np.array_equal(a["scores"].view(np.int64), b["scores"].view(np.int64))


def dump(hits):
    return [[(h.chunk.id, h.score, h.rank, h.source, sorted((h.score_breakdown or {}).items(), key=str)) for h in hs]
            for hs in hits]


@pytest.mark.parametrize("mode", ["char", "dict"])
def test_retriever_device_tokeniser_equals_host_on_han_queries(law, mode, tmp_path, monkeypatch):
    from legal_rag_amd import text
    from legal_rag_amd.config import AppConfig
    from legal_rag_amd.retrieval.bm25_retriever import BM25Retriever
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    monkeypatch.setattr(text, "HAVE_JIEBA", False)
    monkeypatch.setattr(text, "_custom_cut", None)
    cfg = AppConfig.for_data_dir(str(tmp_path), "zh")
    cfg.retrieval.encoder_backend = "hashing"
    cfg.retrieval.enable_rerank = False
    cfg.retrieval.enable_colbert = False
    cfg.retrieval.zh_tokenizer = mode
    if mode == "dict":
        p = tmp_path / "dict.txt"
        p.write_text("\n".join(H.ngram_dict_lines(law["texts"])), encoding="utf-8")
        cfg.retrieval.zh_dict_file = str(p)
    chunks = load_chunks_from_dir(str(GOLDEN / "corpus"), "law_zh.jsonl")[:200]
    build_faiss_index(cfg, chunks)
    build_bm25_index(cfg, chunks)
    r = HybridRetriever(copy.deepcopy(cfg))
    qs = H.law_zh_sentences([c.text for c in chunks], 64, seed=8)
    assert all(text.contains_han(q) for q in qs)
    host = r.search_batch_arrays(qs, top_k=10)
    assert r.bm25.index_tokenizer == mode
    host_lean = r.search_batch_arrays(qs, top_k=10, values=False)
    host_hits = r.search_batch(qs, top_k=10)
    assert not host["zh_exact"].any() and (host["count"] > 0).all()
    r.cfg.retrieval.query_tokenizer = "device"
    real = BM25Retriever.term_ids_batch

    def no_host(self, questions):
        raise AssertionError("the host tokeniser ran for a batch the device decides")
    monkeypatch.setattr(BM25Retriever, "term_ids_batch", no_host)
    assert same_arrays(r.search_batch_arrays(qs, top_k=10), host)
    assert same_arrays(r.search_batch_arrays(qs, top_k=10, values=False), host_lean)
    assert dump(r.search_batch(qs, top_k=10)) == dump(host_hits)
    monkeypatch.setattr(BM25Retriever, "term_ids_batch", real)
    # the per-query search(): the same hits.  A single query takes the GEMV form of the dense scan, a batch the MFMA form:
    # the fp32 dot products are summed in another order, so dense-derived values agree to rounding (2e-5, the bound
    # tests/test_api_gpu.py::test_search_batch_equals_single_queries uses) and two hits whose fused scores lie that close
    # may swap places; the BM25 side is fp64 and agrees bit for bit
    r.cfg.retrieval.query_tokenizer = "host"
    for q, got in zip(qs, host_hits):
        exp = r.search(q, top_k=10)
        assert len(got) == len(exp) and np.allclose([h.score for h in got], [h.score for h in exp], rtol=0, atol=2e-5)
        by_id = {h.chunk.id: h for h in exp}
        for i, (g, e) in enumerate(zip(got, exp)):
            assert g.score_breakdown["zh_exact"] is False and e.score_breakdown["zh_exact"] is False
            assert g.chunk.id == e.chunk.id or abs(g.score - e.score) <= 2e-5, (q, i)
            if g.chunk.id in by_id:
                assert g.score_breakdown["bm25_norm"] == by_id[g.chunk.id].score_breakdown["bm25_norm"]

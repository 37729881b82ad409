"""The BM25 query tokeniser on the device (csrc/tokenize.hip, amdr_tokenizer_encode_device): the CSR it writes is
amdr_tokenizer_encode's for the SAME byte blob, term for term; the text-in step of HybridEngine (eager and captured) and
HybridRetriever with query_tokenizer="device" give the host path's results bit for bit."""
import copy
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

HAN = "第四百九十五条"
SPACES = ["　", "\xa0", " ", " ", " ", " ", " ", " ", "\x85", "\x1c", "\x0b", "\x0c"]


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


def device_csr(dtok, blob: bytes, offs, *, stream=None):
    import torch
    dev = torch.device("cuda", 0)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    nq = len(offs) - 1
    b = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev) if blob else torch.zeros(0, dtype=torch.uint8,
                                                                                                       device=dev)
    o = torch.from_numpy(offs).to(dev)
    cap = max(len(blob), 1)
    terms = torch.full((cap,), -7, dtype=torch.int32, device=dev)
    q_ptr = torch.full((nq + 1,), -9, dtype=torch.int64, device=dev)
    flags = torch.full((nq,), -9, dtype=torch.int32, device=dev)
    dtok.reserve(max(nq, 1), max(len(blob), 1))
    dtok.encode_device(b, o, terms, q_ptr, flags, stream=stream)
    torch.cuda.synchronize()
    qp = q_ptr.cpu().numpy()
    return terms.cpu().numpy()[: int(qp[-1])], qp, flags.cpu().numpy()


def pack(texts):
    enc = [t.encode("utf-8", "surrogatepass") if isinstance(t, str) else t for t in texts]
    offs = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum([len(e) for e in enc], out=offs[1:])
    return b"".join(enc), offs


def assert_same(tok, dtok, blob, offs):
    ht, hp, hf = host_csr(tok, blob, offs)
    dt, dp, df = device_csr(dtok, blob, offs)
    assert dp[0] == 0
    assert np.array_equal(dp, hp), np.flatnonzero(dp != hp)[:5]
    assert np.array_equal(df, hf), np.flatnonzero(df != hf)[:5]
    assert np.array_equal(dt, ht), np.flatnonzero(dt != ht)[:5]
    return ht, hp, hf


@pytest.fixture(scope="module")
def ucc():
    from legal_rag_amd import _native, text
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.evaluation import synthetic_queries
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    chunks = load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")
    bm = BM25Okapi([text.tokenize_en(c.text) for c in chunks])
    # the index vocabulary plus the tokens only the query-side rule produces (capitals, marks, blanks), so that the
    # comparison sees hits of every length, not only -1
    vocab = list(bm.vocab().keys()) + ["What", "UCC", " ", "§", "(", ")", "C++", "AT&T", "--", "3.5%", "\r\n", "é", "　"]
    tok = _native.Tokenizer(vocab)
    dtok = _native.DeviceTokenizer(tok, device=0)
    qs = [q for q, _, _ in synthetic_queries(chunks, seed=0)]
    return dict(chunks=chunks, bm=bm, tok=tok, dtok=dtok, qs=qs)


def test_ucc_queries_and_the_tiled_headline_batch(ucc):
    qs = ucc["qs"]
    assert len(qs) == 1168
    ht, hp, hf = assert_same(ucc["tok"], ucc["dtok"], *pack(qs))
    assert (ht >= 0).mean() > 0.5 and not hf.any()
    assert_same(ucc["tok"], ucc["dtok"], *pack(qs * 32))  # 37 376 queries: the bench step


def test_every_seventh_chunk_text(ucc):
    assert_same(ucc["tok"], ucc["dtok"], *pack([c.text for c in ucc["chunks"][::7]]))


def test_native_cases_of_the_host_rule(ucc):
    from test_text import NATIVE_CASES
    assert_same(ucc["tok"], ucc["dtok"], *pack(NATIVE_CASES))
    for q in NATIVE_CASES:  # one query per call as well
        assert_same(ucc["tok"], ucc["dtok"], *pack([q]))


def test_seeded_fuzz_with_han_emoji_and_unicode_spaces(ucc):
    rng = np.random.default_rng(11)
    alphabet = (list("abcXYZ0159") + list("+#&._%-") * 2 + list(" \t\n\r") + ["\r\n", "§", "é", "(", ")", ",", "C++",
                "AT&T", "c#", "What", "3.5%", "合", "\U0001F600", "一", "鿕", "鿖", "䷿"] + SPACES)
    texts = ["".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=int(rng.integers(0, 40)))) for _ in range(3000)]
    _, _, hf = assert_same(ucc["tok"], ucc["dtok"], *pack(texts))
    assert hf.any() and not hf.all()


def test_raw_bytes_malformed_utf8_and_nuls(ucc):
    rng = np.random.default_rng(5)
    pieces = [b"\xff", b"\xc3", b"\xe4\xb8", b"\xf0\x9f\x98", b"\x80\x80", b"\0", b"a\0b", b"\xe4\xb8\x80", b" ", b"C++",
              b"\xc2\xa0", b"\xe3\x80\x80", b"ok", b"1.5%", b"\r\n", b"\xed\xa0\x80", b"\xf8\x88\x80\x80\x80"]
    texts = [b"".join(pieces[i] for i in rng.integers(0, len(pieces), size=int(rng.integers(0, 25)))) for _ in range(2000)]
    texts += [bytes(rng.integers(0, 256, size=int(n), dtype=np.uint8)) for n in rng.integers(0, 200, size=500)]
    texts += [b"abc\xe4", b"\xe4", b"\xf0\x9f", b"x\xc3"]  # a sequence cut by the END of the query
    assert_same(ucc["tok"], ucc["dtok"], *pack(texts))


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 255, 256, 257, 513])
def test_batch_sizes(ucc, nq):
    qs = (ucc["qs"] * 2)[:nq]
    blob, offs = pack(qs)
    ht, hp, hf = assert_same(ucc["tok"], ucc["dtok"], blob, offs)
    assert len(hp) == nq + 1 and hp[0] == 0


def test_one_100kb_query_among_short_ones(ucc):
    rng = np.random.default_rng(2)
    words = ucc["qs"][:50]
    big = " ".join(words[i] for i in rng.integers(0, 50, size=2000)).encode()[:100_000]
    assert len(big) == 100_000
    assert_same(ucc["tok"], ucc["dtok"], *pack(ucc["qs"][:100] + [big] + ucc["qs"][100:200]))
    assert_same(ucc["tok"], ucc["dtok"], *pack([big + HAN.encode()]))  # a Han character at its very end: flagged, no terms


def test_empty_and_whitespace_only_queries(ucc):
    texts = ["", " ", "   ", "\t\r\n", "\r\n\r\n", "", "　　", "".join(SPACES), "", "x", ""]
    ht, hp, hf = assert_same(ucc["tok"], ucc["dtok"], *pack(texts))
    assert hp[1] == 0 and not hf.any()
    assert_same(ucc["tok"], ucc["dtok"], *pack([""] * 300))


# ---- vocabulary edge cases -------------------------------------------------------------------------------------------
def fnv(b: bytes) -> int:
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return (h ^ (h >> 32)) & 0xFFFFFFFF


def vocab_case(vocab, texts):
    from legal_rag_amd import _native
    tok = _native.Tokenizer(vocab)
    dtok = _native.DeviceTokenizer(tok, device=0)
    try:
        return assert_same(tok, dtok, *pack(texts))
    finally:
        dtok.close()


def test_empty_vocabulary_gives_minus_one_everywhere(ucc):
    ht, _, _ = vocab_case([], ucc["qs"][:300])
    assert len(ht) and (ht == -1).all()


def test_repeated_one_byte_multibyte_and_long_terms(ucc):
    long1, long2 = "L" * 65, "x" * 300
    vocab = ["a", "buyer", "a", "§", "buyer", "é", "合同", long1, long2, long1, " ", "C++", "-", "é"]
    texts = ["a buyer § é a", f"{long1} {long2} {long1}x C++ -- -", "é§é"]
    ht, hp, _ = vocab_case(vocab, texts)
    first = {}
    for i, w in enumerate(vocab):
        first.setdefault(w, i)
    assert ht[hp[0]:hp[1]].tolist() == [first["a"], first[" "], first["buyer"], first[" "], first["§"], first[" "],
                                        first["é"], first[" "], first["a"]]
    assert ht[hp[1]] == first[long1] and ht[hp[1] + 2] == first[long2]


def test_vocabulary_with_long_probe_chains(ucc):
    # 64 terms -> a table of 128 slots: 48 of them hash to ONE slot, so lookups walk chains of up to 48 entries
    rng = np.random.default_rng(9)
    same, other = [], []
    while len(same) < 48 or len(other) < 16:
        w = "".join(chr(97 + int(c)) for c in rng.integers(0, 26, size=int(rng.integers(2, 9))))
        if w in same or w in other:
            continue
        if fnv(w.encode()) & 127 == 5:
            if len(same) < 48:
                same.append(w)
        elif len(other) < 16:
            other.append(w)
    vocab = same + other
    texts = [" ".join(rng.permutation(vocab + ["zz", "nothere", "q"]).tolist()) for _ in range(64)]
    ht, _, _ = vocab_case(vocab, texts)
    assert (ht >= 0).sum() > 64 * 60


# ---- argument checks -----------------------------------------------------------------------------------------------------
def test_capacity_and_reserve_are_checked_and_nothing_is_written(ucc):
    import torch
    from legal_rag_amd import _native
    dev = torch.device("cuda", 0)
    blob, offs = pack(ucc["qs"][:100])
    dtok = _native.DeviceTokenizer(ucc["tok"], device=0)
    b = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    o = torch.from_numpy(offs).to(dev)

    def outs(cap):
        return (torch.full((cap,), -7, dtype=torch.int32, device=dev), torch.full((101,), -9, dtype=torch.int64, device=dev),
                torch.full((100,), -9, dtype=torch.int32, device=dev))

    def untouched(t, p, f):
        torch.cuda.synchronize()
        return bool((t == -7).all() and (p == -9).all() and (f == -9).all())

    t, p, f = outs(len(blob))
    with pytest.raises(_native.NativeError, match=r"status -1.*reserve"):
        dtok.encode_device(b, o, t, p, f)  # before any reserve
    dtok.reserve(100, len(blob))
    t, p, f = outs(len(blob) - 1)
    with pytest.raises(_native.NativeError, match=r"status -1.*capacity"):
        dtok.encode_device(b, o, t, p, f)
    assert untouched(t, p, f)
    dtok2 = _native.DeviceTokenizer(ucc["tok"], device=0)
    dtok2.reserve(99, len(blob))
    t, p, f = outs(len(blob))
    with pytest.raises(_native.NativeError, match=r"status -1.*exceed the reserve"):
        dtok2.encode_device(b, o, t, p, f)  # nq = 100 > 99
    assert untouched(t, p, f)
    dtok3 = _native.DeviceTokenizer(ucc["tok"], device=0)
    dtok3.reserve(100, len(blob) - 1)
    with pytest.raises(_native.NativeError, match=r"status -1.*exceed the reserve"):
        dtok3.encode_device(b, o, t, p, f)  # n_bytes above the reserve
    assert untouched(t, p, f)
    dtok3.close()
    dtok.encode_device(b, o, t, p, f)
    torch.cuda.synchronize()
    assert p.cpu().numpy().tolist() == host_csr(ucc["tok"], blob, offs)[1].tolist()
    dtok.close()
    dtok2.close()


# ---- the text-in step of the engine, eager and captured ------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(ucc):
    import torch
    from legal_rag_amd import _native
    from legal_rag_amd.encoders import HashingEmbedder
    from legal_rag_amd.retrieval.engine import HybridEngine
    emb = HashingEmbedder(dim=768)
    X = emb.encode([c.text for c in ucc["chunks"]])
    dense = _native.DenseIndex(X, device=0)
    bm25 = ucc["bm"].gpu(0)
    tok = _native.Tokenizer(list(ucc["bm"].vocab().keys()))
    eng = HybridEngine(dense, bm25, None, device=0, tokenizer=_native.DeviceTokenizer(tok, device=0))
    Q = torch.from_numpy(emb.encode_queries(ucc["qs"])).cuda()
    return eng, tok, Q


def host_step(eng, tok, params, k, q_emb, texts):
    import torch
    t, p, _ = tok.encode(texts)
    return eng.search_batch(params, k, q_emb=q_emb, q_terms=torch.from_numpy(t if t.size else np.zeros(1, np.int32)).cuda(),
                            q_ptr=torch.from_numpy(p).cuda())


def same_result(a, b):
    import torch
    torch.cuda.synchronize()
    for x, y in ((a.ids, b.ids), (a.vals, b.vals), (a.mask, b.mask), (a.count, b.count), (a.bm25_ids, b.bm25_ids),
                 (a.bm25_scores, b.bm25_scores)):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)  # bits, NaN padding included
        if not np.array_equal(x, y):
            return False
    return True


def texts_on_device(texts, size=None):
    import torch
    blob, offs = pack(texts)
    b = torch.zeros(max(size or len(blob), 1), dtype=torch.uint8, device="cuda")
    if blob:
        b[: len(blob)] = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    return b, torch.from_numpy(offs).cuda()


def test_text_in_step_eager_and_on_a_side_stream(engine, ucc):
    import torch
    from legal_rag_amd import _native
    eng, tok, Q = engine
    params = _native.make_fuse_params(min_final_score=0.2)
    for nq in (1, 3, 300):  # the one-launch serving form (<= 4 queries) and the batched one
        qs = ucc["qs"][:nq]
        ref = host_step(eng, tok, params, 10, Q[:nq].contiguous(), qs)
        ref_c = [x.clone() for x in (ref.ids, ref.vals, ref.mask, ref.count, ref.bm25_ids, ref.bm25_scores)]
        got = eng.search_batch(params, 10, q_emb=Q[:nq].contiguous(), q_text=texts_on_device(qs))
        assert same_result(got, type(got)(*ref_c[:4], bm25_ids=ref_c[4], bm25_scores=ref_c[5])), nq
        assert not got.needs_segmenter.cpu().numpy().any()
    s = torch.cuda.Stream()
    qs = ucc["qs"][300:700]
    ref = host_step(eng, tok, params, 10, Q[300:700].contiguous(), qs)
    ref_c = [x.clone() for x in (ref.ids, ref.vals, ref.mask, ref.count, ref.bm25_ids, ref.bm25_scores)]
    blob, offs = texts_on_device(qs)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = eng.search_batch(params, 10, q_emb=Q[300:700].contiguous(), q_text=(blob, offs))
    s.synchronize()
    assert same_result(got, type(got)(*ref_c[:4], bm25_ids=ref_c[4], bm25_scores=ref_c[5]))
    # a Han query: flagged, no BM25 terms (what the host tokeniser's CSR gives it too)
    t, p, f = eng.tokenize_device(*texts_on_device(["buyer", HAN + " buyer", "seller"]))
    torch.cuda.synchronize()
    assert f.cpu().tolist() == [0, 1, 0] and p.cpu().tolist()[1] == p.cpu().tolist()[2]


def test_captured_text_in_step_replays_new_bytes(engine, ucc):
    import torch
    from legal_rag_amd import _native
    eng, tok, Q = engine
    params = _native.make_fuse_params(min_final_score=0.2)
    nq = 512
    qa, qb = ucc["qs"][:nq], ucc["qs"][600:600 + nq]
    cap = max(len(pack(qa)[0]), len(pack(qb)[0])) + 64
    blob, offs = texts_on_device(qa, cap)
    q_emb = Q[:nq].clone()
    graph, res = eng.capture(params, 10, q_emb=q_emb, q_text=(blob, offs))

    def replayed(stream=None):
        # the graph's outputs are the engine's buffers, which an eager step also writes: poison them, replay, copy out
        for t in (res.ids, res.vals, res.mask, res.count, res.bm25_ids, res.bm25_scores):
            t.fill_(-3)
        torch.cuda.synchronize()
        if stream is None:
            graph.replay()
        else:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                graph.replay()
            stream.synchronize()
        torch.cuda.synchronize()
        got = [x.clone() for x in (res.ids, res.vals, res.mask, res.count, res.bm25_ids, res.bm25_scores)]
        return type(res)(*got[:4], bm25_ids=got[4], bm25_scores=got[5])

    got = replayed()
    assert same_result(got, host_step(eng, tok, params, 10, Q[:nq].contiguous(), qa))
    # another batch's bytes INTO the same buffers, then replay
    nb, no = texts_on_device(qb, cap)
    blob.copy_(nb)
    offs.copy_(no)
    q_emb.copy_(Q[600:600 + nq])
    got = replayed()
    assert not same_result(got, host_step(eng, tok, params, 10, Q[:nq].contiguous(), qa))  # a different batch indeed
    assert same_result(got, host_step(eng, tok, params, 10, Q[600:600 + nq].contiguous(), qb))
    # ... and replayed on a non-default stream
    assert same_result(replayed(torch.cuda.Stream()), host_step(eng, tok, params, 10, Q[600:600 + nq].contiguous(), qb))


# ---- HybridRetriever with query_tokenizer = "device" ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def ucc_index(tmp_path_factory):
    from legal_rag_amd.config import AppConfig
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.colbert_builder import build_colbert_index
    from legal_rag_amd.retrieval.builders.faiss_builder import build_faiss_index
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    data = tmp_path_factory.mktemp("data")
    cfg = AppConfig.for_data_dir(str(data), "en")
    cfg.retrieval.encoder_backend = "hashing"
    cfg.retrieval.enable_rerank = False
    chunks = load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl")[:200]
    build_faiss_index(cfg, chunks)
    build_bm25_index(cfg, chunks)
    build_colbert_index(cfg, chunks)
    return cfg, chunks


def dump(hits):
    return [[(h.chunk.id, h.score, h.rank, h.source, sorted((h.score_breakdown or {}).items(), key=str)) for h in hs]
            for hs in hits]


def same_arrays(a, b):
    for key in ("rows", "count", "channel_mask", "zh_exact"):
        if not np.array_equal(a[key], b[key]):
            return False
    if "values" in a and not np.array_equal(a["values"].view(np.int64), b["values"].view(np.int64)):
        return False
    return np.array_equal(a["scores"].view(np.int64), b["scores"].view(np.int64))


@pytest.mark.parametrize("colbert", [False, True])
def test_retriever_device_tokeniser_equals_host(ucc_index, ucc, colbert, monkeypatch):
    from legal_rag_amd.retrieval.bm25_retriever import BM25Retriever
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    cfg, _ = ucc_index
    cfg2 = copy.deepcopy(cfg)
    cfg2.retrieval.enable_colbert = colbert
    r = HybridRetriever(cfg2)
    qs = ucc["qs"][:400] + ["What is § 2-314?", "rate of 3.5% p.a. (a) C++", "x", "é—ü　z", "\U0001F600 goods"]
    host = r.search_batch_arrays(qs, top_k=10)
    host_lean = r.search_batch_arrays(qs, top_k=10, values=False)
    host_hits = dump(r.search_batch(qs[:60], top_k=10))
    r.cfg.retrieval.query_tokenizer = "device"
    real = BM25Retriever.term_ids_batch

    def no_host(self, questions):
        raise AssertionError("the host tokeniser ran for a batch the device decides")
    monkeypatch.setattr(BM25Retriever, "term_ids_batch", no_host)
    assert same_arrays(r.search_batch_arrays(qs, top_k=10), host)
    assert same_arrays(r.search_batch_arrays(qs, top_k=10, values=False), host_lean)
    assert dump(r.search_batch(qs[:60], top_k=10)) == host_hits
    monkeypatch.setattr(BM25Retriever, "term_ids_batch", real)
    # the single-query call keeps the host tokeniser (one launch; an extra launch costs more than it saves)
    calls = []
    monkeypatch.setattr(BM25Retriever, "term_ids_batch", lambda self, q: calls.append(len(q)) or real(self, q))
    r.search(qs[0], top_k=10)
    assert calls == [1]


def test_retriever_mixed_han_batch_and_registered_segmenter_take_the_host_path(ucc_index, ucc, monkeypatch):
    from legal_rag_amd import text
    from legal_rag_amd.retrieval.bm25_retriever import BM25Retriever
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    cfg, _ = ucc_index
    cfg2 = copy.deepcopy(cfg)
    cfg2.retrieval.enable_colbert = False
    cfg2.retrieval.zh_tokenizer = "char"
    monkeypatch.setattr(text, "HAVE_JIEBA", False)
    monkeypatch.setattr(text, "_custom_cut", None)
    r = HybridRetriever(cfg2)
    qs = ucc["qs"][:100] + [HAN + " buyer", "合同 contract"]
    host = r.search_batch_arrays(qs, top_k=10)
    host_hits = dump(r.search_batch(qs, top_k=10))
    assert not host["zh_exact"][-1] and host["zh_exact"][:100].all()
    real = BM25Retriever.term_ids_batch
    calls = []
    monkeypatch.setattr(BM25Retriever, "term_ids_batch", lambda self, q: calls.append(len(q)) or real(self, q))
    r.cfg.retrieval.query_tokenizer = "device"
    assert same_arrays(r.search_batch_arrays(qs, top_k=10), host)
    assert dump(r.search_batch(qs, top_k=10)) == host_hits
    assert calls == [len(qs), len(qs)]  # a Han query anywhere: the whole batch takes today's host path
    # a registered segmenter sees every query, Han or not
    r.cfg.retrieval.query_tokenizer = "host"
    text.register_tokenizer(lambda s: text.jieba_cut_restated(s), "mine")
    try:
        host = r.search_batch_arrays(qs[:100], top_k=10)
        r.cfg.retrieval.query_tokenizer = "device"
        calls.clear()
        assert same_arrays(r.search_batch_arrays(qs[:100], top_k=10), host)
        assert calls == [100]
    finally:
        text.register_tokenizer(None)

"""The Han modes of the BM25 tokenisers on the host: the specification (text.load_han_dict, text.dict_cut,
text.jieba_cut_restated) against its known answers, the native host tokeniser (_native.Tokenizer(han=), csrc/tokenize.cpp
over csrc/tokenize_rule.hpp) against the specification token for token, and BM25Retriever's routing.  No GPU."""
import math

import numpy as np
import pytest

import han_adversary as H


@pytest.fixture(autouse=True)
def no_segmenter(monkeypatch):
    """The stand-ins apply when neither jieba nor a registered segmenter exists."""
    from legal_rag_amd import text
    monkeypatch.setattr(text, "HAVE_JIEBA", False)
    monkeypatch.setattr(text, "_custom_cut", None)
    monkeypatch.delenv("LEGALRAG_ZH_TOKENIZER", raising=False)


@pytest.fixture(scope="module")
def known():
    from legal_rag_amd import text
    return text.load_han_dict(H.KNOWN_DICT_LINES)


@pytest.fixture(scope="module")
def fuzz():
    from legal_rag_amd import text
    return text.load_han_dict(H.fuzz_dict_lines()), H.fuzz_texts()


@pytest.fixture(scope="module")
def law():
    from legal_rag_amd import text
    texts = H.law_zh_texts()
    return texts, text.load_han_dict(H.ngram_dict_lines(texts))


# ---- the specification -----------------------------------------------------------------------------------------------------
def test_known_answers_of_the_specification(known):
    from legal_rag_amd import text
    assert known.total == H.KNOWN_TOTAL
    for s, want in H.KNOWN_DICT_ANSWERS:
        assert text.dict_cut(s, known) == want, s
    for s, want in H.KNOWN_CHAR_ANSWERS:
        assert text.jieba_cut_restated(s) == want, s
    st = {}
    assert text.dict_cut("人民", known, st) == ["人", "民"] and st == {"bufword": 1}
    st = {}
    text.dict_cut("第3.5%条 C++法律", known, st)
    assert st == {"finalseg": 1, "words": 2}
    for s, want in H.KNOWN_DICT_ANSWERS:  # every token is a piece of the text, in order
        assert "".join(want) == s


def test_dictionary_parser(tmp_path):
    from legal_rag_amd import text
    d = text.load_han_dict(["合同法 3 n", "", "   ", "合同 5", "合同法 7", "条款\t0", "人 2 nr extra"])
    assert d.lfreq == {"合同法": 7, "合": 0, "合同": 5, "条款": 0, "条": 0, "人": 2}  # a later line wins; prefixes at 0
    assert d.total == 3 + 5 + 7 + 0 + 2  # every line counts, the replaced one too
    assert d.logw["合同"] == math.log(5) - math.log(17) and "合" not in d.logw and "条款" not in d.logw
    assert d.logw_unknown == 0.0 - math.log(17)
    p = tmp_path / "dict.txt"
    p.write_text("合同 5\n法律 6 n\n", encoding="utf-8")
    assert text.load_han_dict(str(p)).lfreq == text.load_han_dict(p).lfreq == {"合同": 5, "合": 0, "法律": 6, "法": 0}
    with pytest.raises(ValueError, match="line 2"):
        text.load_han_dict(["合同 5", "法律"])
    with pytest.raises(ValueError, match="line 1"):
        text.load_han_dict(["合同 n"])
    with pytest.raises(ValueError, match="line 1"):
        text.load_han_dict(["合同 -5"])
    with pytest.raises(ValueError, match="total"):
        text.load_han_dict(["合同 0", "法律 0"])
    with pytest.raises(ValueError, match="total"):
        text.load_han_dict([])


def test_empty_dictionary_is_the_character_rule(fuzz):
    from legal_rag_amd import text
    empty = text.HanDict({}, 1)
    for s in H.adversary_texts() + fuzz[1]:
        if not any(w in s for w in text._ASCII_DICT_WORDS):
            assert text.dict_cut(s, empty) == text.jieba_cut_restated(s), s


def test_modes_ids_and_precedence(known, tmp_path, monkeypatch):
    from legal_rag_amd import text
    assert text.resolve_mode("dict") == "dict" and text.resolve_mode("DICT ") == "dict" and text.resolve_mode("x") == "jieba"
    assert text.tokenizer_id("dict") == "dict" and text.tokenizer_id("char") == "char"
    assert text.tokenizer_id(None) == "jieba-restated-ascii"
    monkeypatch.setenv("LEGALRAG_ZH_TOKENIZER", "dict")
    assert text.resolve_mode(None) == "dict"
    p = tmp_path / "dict.txt"
    p.write_text("\n".join(H.KNOWN_DICT_LINES), encoding="utf-8")
    assert text.jieba_cut("合同法律", None, str(p)) == ["合同", "法律"]
    assert text.jieba_cut("abc C++", "dict", str(p)) == text.jieba_cut_restated("abc C++")  # no Han: the exact rule
    with pytest.raises(ValueError, match="zh_dict_file"):
        text.jieba_cut("合同法律", "dict", None)
    with pytest.raises(ValueError, match="zh_dict_file"):
        text.require_dict("dict", None)
    # a registered segmenter wins
    text.register_tokenizer(lambda s: ["<" + s + ">"], "mine")
    try:
        assert text.jieba_cut("合同法律", "dict", str(p)) == ["<合同法律>"] and text.tokenizer_id("dict") == "mine"
        text.require_dict("dict", None)  # nothing to require: the segmenter cuts
    finally:
        text.register_tokenizer(None)


# ---- the native host tokeniser against the specification ----------------------------------------------------------------------
def both(d):
    from legal_rag_amd import _native
    return _native.Tokenizer([], han="char"), _native.Tokenizer([], han=d)


def assert_native_is_spec(texts, d):
    from legal_rag_amd import text
    tc, td = both(d)
    for s in texts:
        assert tc.cut_han(s) == text.jieba_cut_restated(s), ("char", s)
        assert td.cut_han(s) == text.han_cut(s, "dict", d), ("dict", s)
        if text.contains_han(s):
            assert td.cut_han(s) == text.dict_cut(s, d), ("dict", s)


def test_native_known_answers(known):
    from legal_rag_amd import _native
    tc, td = both(known)
    assert (tc.han_mode, td.han_mode, _native.Tokenizer([]).han_mode) == (1, 2, 0)
    for s, want in H.KNOWN_DICT_ANSWERS:
        assert td.cut_han(s) == want, s
    for s, want in H.KNOWN_CHAR_ANSWERS:
        assert tc.cut_han(s) == want, s
    flag = _native.Tokenizer([])
    assert flag.cut_han("合同 buyer") is None and flag.cut_han("a buyer") == ["a", " ", "buyer"]
    with pytest.raises(ValueError):
        _native.Tokenizer([], han="dict")  # the dictionary mode takes the dictionary itself


def test_native_adversary_list(known, fuzz):
    adv = H.adversary_texts()
    assert "" in adv and "合" in adv and any(len(s.encode()) == 3000 for s in adv)
    assert_native_is_spec(adv, known)
    assert_native_is_spec(adv, fuzz[0])


def test_native_fuzz_reaches_ties_and_word_buffers(fuzz):
    from legal_rag_amd import text
    d, texts = fuzz
    assert len(texts) == 2000 and 40 <= len(d.lfreq) <= 60
    st = {}
    for s in texts:
        text.dict_cut(s, d, st)
    assert st["ties"] >= 20 and st["bufword"] >= 20 and st["finalseg"] >= 20 and st["words"] >= 20, st
    assert_native_is_spec(texts, d)


def test_native_fixture_corpus(law):
    texts, d = law
    assert len(texts) > 1000 and len(d.logw) == 400
    assert_native_is_spec(texts, d)


# ---- the CSR ---------------------------------------------------------------------------------------------------------------------
def test_encode_gives_the_csr_of_the_specification(law):
    from legal_rag_amd import _native, text
    from legal_rag_amd.bm25_model import BM25Okapi
    texts, d = law
    qs = H.law_zh_sentences(texts, 300) + ["", "buyer of goods", "第3.5%条 C++法律", "合", "x"] + H.law_zh_sentences(texts, 300, 4)
    for mode, dd in (("char", None), ("dict", d)):
        bm = BM25Okapi([text.han_cut(t, mode, dd) for t in texts[:200]])
        tok = _native.Tokenizer(list(bm.vocab().keys()), han=dd if mode == "dict" else "char")
        terms, q_ptr, flags = tok.encode(qs)
        want = [np.asarray(bm.term_ids(text.han_cut(q, mode, dd)), dtype=np.int32) for q in qs]
        assert not flags.any()
        assert q_ptr.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
        assert np.array_equal(terms, np.concatenate(want))
        assert (terms >= 0).mean() > 0.5  # the comparison sees hits, not only -1
        # the default mode: Han queries flagged, no terms
        flag = _native.Tokenizer(list(bm.vocab().keys()))
        t0, p0, f0 = flag.encode(qs)
        han = np.array([text.contains_han(q) for q in qs])
        assert np.array_equal(f0, han) and (np.diff(p0)[han] == 0).all() and (np.diff(p0)[~han] == np.diff(q_ptr)[~han]).all()


def test_set_han_rejects_bad_arguments(known):
    from legal_rag_amd import _native
    tok = _native.Tokenizer(["a"])
    keys, logw, word, unknown = known.native_tables()
    for bad in (float("nan"), float("inf"), -float("inf")):
        lw = logw.copy()
        lw[3] = bad
        with pytest.raises(_native.NativeError, match=r"status -1.*finite"):
            tok.set_han(2, keys, lw, word, unknown)
    with pytest.raises(_native.NativeError, match=r"status -1.*finite"):
        tok.set_han(2, keys, logw, word, float("nan"))
    with pytest.raises(_native.NativeError, match=r"status -1.*needs keys"):
        tok.set_han(2)
    with pytest.raises(_native.NativeError, match=r"status -1.*bad mode"):
        tok.set_han(3)
    assert tok.han_mode == 0  # a refused call leaves the handle as it was
    tok.set_han(2, keys, logw, word, unknown)
    assert tok.han_mode == 2 and tok.cut_han("合同法律") == ["合同", "法律"]
    tok.set_han(1)
    assert tok.han_mode == 1 and tok.cut_han("合同") == ["合", "同"]


# ---- BM25Retriever's routing -----------------------------------------------------------------------------------------------------
class _Cfg:
    class retrieval:
        bm25_index_file = "unused"
        device = 0
        zh_tokenizer = "jieba"
        zh_dict_file = None


def retriever(mode, law, tmp_path):
    """A BM25Retriever over the first 200 chunks, as load() leaves it for an index recorded as built in `mode` (no GPU:
    the postings are never uploaded)."""
    from legal_rag_amd import text
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.retrieval.bm25_retriever import BM25Retriever
    texts, d = law
    cfg = _Cfg()
    cfg.retrieval = type("R", (), dict(vars(_Cfg.retrieval)))()
    cfg.retrieval.zh_tokenizer = mode
    if mode == "dict":
        p = tmp_path / "dict.txt"
        p.write_text("\n".join(H.ngram_dict_lines(texts)), encoding="utf-8")
        cfg.retrieval.zh_dict_file = str(p)
    r = BM25Retriever(cfg)
    r.bm25 = BM25Okapi([text.han_cut(t, mode, d) for t in texts[:200]])
    r.index_tokenizer = mode
    r.load = lambda: None
    return r


@pytest.mark.parametrize("mode", ["char", "dict"])
def test_term_ids_batch_cuts_han_queries_natively(mode, law, tmp_path, monkeypatch):
    r = retriever(mode, law, tmp_path)
    qs = H.law_zh_sentences(law[0], 40) + ["buyer of goods", "", "C++ 3.5%", "合同 contract", None, "é—ü　z"]
    want = [np.asarray(r.bm25.term_ids(r.tokenize_query(q or "")), dtype=np.int32) for q in qs]
    han = np.array([bool(q) and any("一" <= c <= "鿕" for c in q) for q in qs])
    assert han.sum() == 41
    monkeypatch.setattr(type(r), "tokenize_query", lambda self, q: pytest.fail("a Han query took per-query Python"))
    terms, q_ptr, exact = r.term_ids_batch(qs)
    assert q_ptr.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert np.array_equal(terms, np.concatenate(want))
    assert np.array_equal(exact, ~han)
    assert (terms >= 0).sum() > 200
    # the device path takes the batch, with the same exactness
    txt = r.device_text_batch(qs)
    assert txt is not None and np.array_equal(txt[4], ~han) and txt[2] == sum(len((q or "").encode()) for q in qs)
    assert r.han_key() in ("char",) or r.han_key()[0] == "dict"


def test_dict_index_without_a_dictionary_file_raises(law, tmp_path):
    r = retriever("dict", law, tmp_path)
    r.cfg.retrieval.zh_dict_file = None
    with pytest.raises(ValueError, match="zh_dict_file"):
        r.term_ids_batch(["合同法律"])
    with pytest.raises(ValueError, match="zh_dict_file"):
        r.tokenize_query("合同法律")


def test_registered_segmenter_and_other_indexes_keep_their_routing(law, tmp_path, monkeypatch):
    from legal_rag_amd import text
    r = retriever("char", law, tmp_path)
    qs = ["合同 contract", "buyer", "人民法院"]
    seen = []
    text.register_tokenizer(lambda s: seen.append(s) or text.jieba_cut_restated(s), "mine")
    try:
        assert r.han_mode() == "flag" and r.device_text_batch(qs) is None
        calls = []
        real = type(r).tokenize_query
        monkeypatch.setattr(type(r), "tokenize_query", lambda self, q: calls.append(q) or real(self, q))
        terms, q_ptr, exact = r.term_ids_batch(qs)
        # every query takes the per-query route; on a "char" index a Han query keeps the index's own stand-in
        assert calls == qs and seen == ["buyer"]
        r.index_tokenizer = "mine"
        r.term_ids_batch(qs)
        assert seen == ["buyer"] + qs  # ... and on any other index every query goes to the segmenter
        monkeypatch.setattr(type(r), "tokenize_query", real)
    finally:
        text.register_tokenizer(None)
    # the config alone opts in on an index recorded otherwise: a Han query keeps the per-query route
    r.index_tokenizer = "jieba-restated-ascii"
    assert r.han_mode() == "flag" and r.device_text_batch(qs) is None
    terms, q_ptr, exact = r.term_ids_batch(qs)
    assert exact.tolist() == [False, True, False]
    want = [r.bm25.term_ids(text.jieba_cut_restated(q)) for q in qs]
    assert terms.tolist() == [i for w in want for i in w]


def test_builders_record_the_dict_id(law, tmp_path):
    from legal_rag_amd import text
    from legal_rag_amd.retrieval.builders.bm25_builder import tokenize_corpus
    from legal_rag_amd.schemas import LawChunk
    texts, d = law
    p = tmp_path / "dict.txt"
    p.write_text("\n".join(H.ngram_dict_lines(texts)), encoding="utf-8")
    chunks = [LawChunk(id=str(i), law_name="law", article_no=str(i), article_id=str(i), text=t, lang="zh") for i, t in enumerate(texts[:20])]
    docs, tok_id = tokenize_corpus(chunks, "dict", str(p))
    assert tok_id == "dict" and docs == [text.dict_cut(t, d) for t in texts[:20]]
    with pytest.raises(ValueError, match="zh_dict_file"):
        tokenize_corpus(chunks, "dict", None)
    from legal_rag_amd.config import RetrievalConfig
    assert RetrievalConfig().zh_dict_file is None and RetrievalConfig(zh_tokenizer="dict").zh_tokenizer == "dict"

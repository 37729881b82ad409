"""Scopes on the host: Scope / ScopeResolver on the two fixture corpora, the table the scoped kernels take, the exports
of the scoped search in the header and in the binding, and the host-only workspace arithmetic (no GPU needed)."""
import inspect
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT


def _chunks(name):
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    return load_chunks_from_dir(str(GOLDEN / "corpus"), name)


@pytest.fixture(scope="module")
def zh():
    return _chunks("law_zh.jsonl")


@pytest.fixture(scope="module")
def en():
    return _chunks("law_en.jsonl")


def _brute(chunks, **want):
    return np.asarray([i for i, c in enumerate(chunks) if all(getattr(c, f) == v for f, v in want.items())], dtype=np.int64)


def _runs(rows):
    return 1 + int(np.count_nonzero(np.diff(rows) != 1)) if rows.size else 0


def test_scope_is_a_hashable_value():
    from legal_rag_amd.retrieval.scope import Scope
    a = Scope(section="2Part X", article_ids=["2-314", "2-315"])
    b = Scope(section="2Part X", article_ids=("2-315", "2-314"))
    assert a == b and hash(a) == hash(b) and len({a, b, Scope()}) == 2
    assert Scope().unrestricted and not a.unrestricted
    assert Scope(chunk_ids="x").chunk_ids == frozenset({"x"})  # a bare string is one id, not its characters
    with pytest.raises(Exception):
        a.section = "other"  # frozen


def test_resolver_zh_chapters_come_in_several_runs(zh):
    from legal_rag_amd.retrieval.scope import Scope, ScopeResolver
    res = ScopeResolver(zh)
    chapters = sorted({c.chapter for c in zh if c.chapter})
    assert len(chapters) == 79
    sizes, split = [], 0
    for ch in chapters:
        rows = res.rows(Scope(chapter=ch))
        assert rows.dtype == np.int64 and np.array_equal(rows, _brute(zh, chapter=ch))
        assert np.all(np.diff(rows) > 0)  # ascending, unique
        sizes.append(rows.size)
        split += _runs(rows) > 1
    assert 4 <= min(sizes) and max(sizes) <= 56 and sum(sizes) == sum(1 for c in zh if c.chapter)
    assert split > 0  # the chapters of the fixture are not contiguous row ranges


def test_resolver_en_sections_and_anded_fields(en):
    from legal_rag_amd.retrieval.scope import Scope, ScopeResolver
    res = ScopeResolver(en)
    sections = sorted({c.section for c in en if c.section})
    assert len(sections) == 48  # (and the chunks without a section)
    sizes = [res.rows(Scope(section=s)).size for s in sections]
    assert 3 <= min(sizes) and max(sizes) <= 42 and sum(sizes) == sum(1 for c in en if c.section)
    for s in sections[:5]:
        assert np.array_equal(res.rows(Scope(section=s)), _brute(en, section=s))
    # the given fields are ANDed
    sec = sections[7]
    in_sec = res.rows(Scope(section=sec))
    arts = [en[int(in_sec[0])].article_id, en[int(in_sec[-1])].article_id, en[0].article_id]
    both = res.rows(Scope(section=sec, article_ids=arts, law_name=en[0].law_name))
    exp = [i for i in in_sec.tolist() if en[i].article_id in arts]
    assert both.tolist() == exp and 0 < both.size < in_sec.size
    assert res.rows(Scope(section=sec, law_name="no such law")).size == 0
    ids = [en[5].id, en[3].id, en[5].id]
    assert res.rows(Scope(chunk_ids=ids)).tolist() == [3, 5]
    assert res.rows(Scope()).tolist() == list(range(len(en)))  # no field: the whole list


def test_resolver_unknown_value_is_empty_and_results_are_cached(en):
    from legal_rag_amd.retrieval.scope import Scope, ScopeResolver, resolver_for
    res = ScopeResolver(en)
    assert res.rows(Scope(section="no such section")).size == 0
    assert res.rows(Scope(article_ids=["nope"])).size == 0
    s = Scope(section=en[0].section)
    first = res.rows(s)
    assert res.rows(Scope(section=en[0].section)) is first  # cached per (equal) scope
    assert not first.flags.writeable
    assert resolver_for(en) is resolver_for(en)


def test_table_stores_equal_scopes_once(en):
    from legal_rag_amd.retrieval.scope import Scope, ScopeResolver
    res = ScopeResolver(en)
    secs = sorted({c.section for c in en if c.section})
    a, b, none = Scope(section=secs[0]), Scope(section=secs[1]), Scope(section="nothing")
    scope_ptr, rows, qscope, rows_max = res.table([a, b, Scope(section=secs[0]), none, b])
    assert scope_ptr.dtype == np.int64 and rows.dtype == np.int64 and qscope.dtype == np.int32
    assert qscope.tolist() == [0, 1, 0, 2, 1] and scope_ptr.size == 4 and scope_ptr[0] == 0
    ra, rb = res.rows(a), res.rows(b)
    assert rows.tolist() == ra.tolist() + rb.tolist() and scope_ptr.tolist() == [0, ra.size, ra.size + rb.size] + [ra.size + rb.size]
    assert rows_max == max(ra.size, rb.size)
    scope_ptr, rows, qscope, rows_max = res.table([])
    assert scope_ptr.tolist() == [0] and rows.size == 0 and qscope.size == 0 and rows_max == 0


NEW_EXPORTS = ["amdr_scope_create", "amdr_scope_reserve", "amdr_scope_workspace_plan", "amdr_scope_plan_info",
               "amdr_scope_dense_search_device", "amdr_scope_bm25_search_device", "amdr_scope_maxsim_search_device",
               "amdr_scope_dense_search", "amdr_scope_bm25_search", "amdr_scope_maxsim_search", "amdr_scope_destroy"]


def test_every_new_export_is_in_the_header_and_in_signatures():
    from legal_rag_amd import _native
    header = (ROOT / "include" / "amdretrieval.h").read_text(encoding="utf-8")
    declared = set(re.findall(r"\b(amdr_scope_\w+)\s*\(", header))
    assert declared == set(NEW_EXPORTS)
    assert "typedef struct amdr_scope amdr_scope_t;" in header
    for name in NEW_EXPORTS:
        assert name in _native.SIGNATURES and name in _native.EXPORTS, name
    lib = _native.load()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
    assert _native.ScopeWorkspace._destroy == "amdr_scope_destroy"


def test_scope_workspace_plan_reserve_covers_every_call_inside_it(monkeypatch):
    from legal_rag_amd import _native
    for pin in (None, "64", "1", "100000"):
        if pin is None:
            monkeypatch.delenv("AMDR_SCOPE_SLAB", raising=False)
        else:
            monkeypatch.setenv("AMDR_SCOPE_SLAB", pin)
        for nq_max, k_max, rows_res in ((1, 10, 28), (8, 256, 300), (1168, 10, 56), (4096, 64, 5000)):
            res0, _ = _native.scope_workspace_plan(nq_max, k_max, rows_res, 1, 1, 0)
            for nq in sorted({1, 2, nq_max // 2 or 1, nq_max}):
                for k in sorted({1, 9, k_max}):
                    for rows in sorted({0, 1, 63, 64, 65, 256, 257, 1024, 1025, rows_res}):
                        if rows > rows_res or k > k_max or nq > nq_max:
                            continue
                        res, used = _native.scope_workspace_plan(nq_max, k_max, rows_res, nq, k, rows)
                        assert res == res0
                        assert all(u <= r for u, r in zip(used, res)), (pin, nq_max, k_max, rows_res, nq, k, rows, res, used)
    monkeypatch.delenv("AMDR_SCOPE_SLAB", raising=False)
    # a scope inside one slab writes the final lists directly: no workspace at all
    assert _native.scope_workspace_plan(4, 10, 64, 4, 10, 64) == ((0, 0, 0), (0, 0, 0))
    # dense slabs hold 256 rows, BM25 1 024, MaxSim 64: 300 rows span 2 / 1 / 5
    (d, b, m), _ = _native.scope_workspace_plan(3, 10, 300, 1, 1, 1)
    assert d > 0 and b == 0 and m > d


def test_public_interface_takes_scopes_keyword_only():
    from legal_rag_amd.retrieval.by_lang_retriever import ByLangRetriever
    from legal_rag_amd.retrieval.engine import HybridEngine
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    for fn, name in ((HybridRetriever.search, "scope"), (HybridRetriever.search_dense, "scope"),
                     (HybridRetriever.search_bm25, "scope"), (HybridRetriever.search_colbert, "scope"),
                     (HybridRetriever.search_batch, "scopes"), (HybridRetriever.search_batch_arrays, "scopes"),
                     (ByLangRetriever.search, "scope"), (HybridEngine.search_batch, "scopes")):
        p = inspect.signature(fn).parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn
    assert inspect.signature(HybridEngine.reserve).parameters["rows_max"].default == 0
    for name in ("upload_scopes", "dense_topk_scoped", "bm25_topk_scoped", "colbert_topk_scoped"):
        assert callable(getattr(HybridEngine, name))


def test_graph_decision_with_a_scope_raises_before_any_device_work(en):
    from types import SimpleNamespace
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    from legal_rag_amd.retrieval.scope import Scope
    r = HybridRetriever.__new__(HybridRetriever)
    dec = [SimpleNamespace(mode="GRAPH_AUGMENTED"), None]
    with pytest.raises(ValueError, match="graph"):
        r._split_scopes(2, [Scope(section=en[0].section), None], dec, en, "search_batch")
    plain, scoped, empty = r._split_scopes(3, [None, Scope(section=en[0].section), Scope(section="nothing")],
                                           [dec[0], None, None], en, "search_batch")
    assert (plain, scoped, empty) == ([0], [1], [2])
    with pytest.raises(ValueError):
        r._split_scopes(2, [None], None, en, "search_batch")

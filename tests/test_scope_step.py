"""The scoped step as one call, on the host: the exports of amdr_hybrid_scope_device / amdr_hybrid_scope_plan in the header
and in the binding, and the host-only arithmetic that says when the one-launch form (scope_hybrid_kernel) applies and how
much LDS it takes (no GPU needed)."""
import re

import pytest

from conftest import ROOT

STEP_EXPORTS = {"amdr_hybrid_scope_device": "PPPPPP" + "PPPil" * 2 + "iii" + "PPP" + "PPiP" + "PPPP" + "PPPP" + "P",
                "amdr_hybrid_scope_plan": "iiiillPP"}


def test_the_step_exports_are_in_the_header_the_binding_and_the_library():
    from legal_rag_amd import _native
    header = (ROOT / "include" / "amdretrieval.h").read_text(encoding="utf-8")
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(amdr_[a-z0-9_]+)\s*\(", header))
    lib = _native.load()
    for name, kinds in STEP_EXPORTS.items():
        assert name in declared, name
        assert name in _native.EXPORTS and _native.SIGNATURES[name] == kinds, name
        assert hasattr(lib, name), name
    assert callable(_native.ScopeWorkspace.hybrid) and callable(_native.hybrid_scope_plan)


def test_the_header_cites_the_reference_lines_of_the_neighbouring_entries():
    header = (ROOT / "include" / "amdretrieval.h").read_text(encoding="utf-8")
    at = header.index("int amdr_hybrid_scope_device(")
    comment = header[header.rindex("/*", 0, at):at]
    assert "hybrid_retriever.py:282-384" in comment


@pytest.fixture
def plan(monkeypatch):
    from legal_rag_amd import _native
    monkeypatch.delenv("AMDR_SCOPE_SLAB", raising=False)
    monkeypatch.delenv("AMDR_SCOPE_FUSED", raising=False)
    return _native.hybrid_scope_plan


def test_plan_applies_inside_one_slab_and_32_candidates(plan):
    for args in ((1, 10, 10, 0, 28, 28), (1168, 10, 10, 10, 256, 1024), (37, 16, 16, 0, 256, 1024), (1, 1, 1, 0, 0, 0),
                 (5, 20, 12, 0, 65, 65), (2, 1, 1, 30, 1, 1)):
        fused, lds = plan(*args)
        assert fused, args
        assert 0 < lds <= 64 * 1024, (args, lds)


def test_plan_does_not_apply_beyond_a_slab_or_32_candidates(plan, monkeypatch):
    for args in ((1, 10, 10, 0, 257, 28),    # 257 dense rows: two dense slabs
                 (1, 10, 10, 0, 28, 1025),   # 1 025 BM25 documents: two BM25 slabs
                 (1, 17, 16, 0, 28, 28),     # kd + kb = 33
                 (1, 10, 10, 13, 28, 28)):   # kd + kb + kc = 33
        assert plan(*args) == (False, 0), args
    monkeypatch.setenv("AMDR_SCOPE_SLAB", "64")  # the pin holds for both channels
    assert plan(1, 10, 10, 0, 64, 64)[0]
    assert plan(1, 10, 10, 0, 65, 64) == (False, 0) and plan(1, 10, 10, 0, 64, 65) == (False, 0)
    monkeypatch.delenv("AMDR_SCOPE_SLAB")
    monkeypatch.setenv("AMDR_SCOPE_FUSED", "0")  # pinned off
    assert plan(1, 10, 10, 0, 28, 28) == (False, 0)
    monkeypatch.setenv("AMDR_SCOPE_FUSED", "1")
    assert plan(1, 10, 10, 0, 28, 28)[0]


def test_plan_lds_is_the_two_pieces_side_by_side(plan, monkeypatch):
    """dense: 4 wave lists of cap C32 + 4 counts; BM25: a slab of fp64 scores, 4 wave lists of cap C64, 4 counts, the token
    table (3 x 32 x 8 B + 8); cap = 128 for every depth the packed fusion takes.  The slab pin shrinks the score region."""
    dense = 4 * 128 * 8 + 16
    bm25 = lambda slab: slab * 8 + 4 * 128 * 16 + 16 + 3 * 32 * 8 + 8  # noqa: E731
    for kd, kb in ((1, 1), (10, 10), (16, 16), (20, 12)):
        assert plan(1, kd, kb, 0, 28, 28)[1] == dense + bm25(1024)
    monkeypatch.setenv("AMDR_SCOPE_SLAB", "64")
    assert plan(1, 10, 10, 0, 28, 28)[1] == dense + bm25(64)


def test_plan_refuses_bad_sizes(plan):
    from legal_rag_amd import _native
    for args in ((0, 10, 10, 0, 28, 28), (1, 0, 10, 0, 28, 28), (1, 10, 0, 0, 28, 28), (1, 10, 10, -1, 28, 28),
                 (1, 10, 10, 0, -1, 28), (1, 257, 10, 0, 28, 28)):
        with pytest.raises(_native.NativeError):
            plan(*args)


def test_engine_routes_the_scoped_step_through_one_call():
    import inspect
    from legal_rag_amd.retrieval.engine import HybridEngine
    assert callable(HybridEngine.hybrid_scoped)
    src = inspect.getsource(HybridEngine.search_batch)
    assert "hybrid_scoped" in src

"""Facets on the host: the plain evaluator of tests/facet_cases.py on written-out cases, ScopeResolver.codes (first-appearance
order, None -> -1, the cache), the validation of Facets, and the decoding of the kernel's arrays.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

import facet_cases as FC


def test_the_evaluator_on_written_out_cases():
    # six rows; chapter codes 0 0 1 - 1 2 (row 3 has none)
    codes = np.array([[0, 0, 1, -1, 1, 2]], dtype=np.int32)
    scope_ptr = np.array([0, 6, 6, 9], dtype=np.int64)
    rows = np.array([0, 1, 2, 3, 4, 5, 2, 3, 5], dtype=np.int64)
    total, missing, distinct, code, count = FC.evaluate(scope_ptr, rows, codes, [3], 2)
    assert total.tolist() == [6, 0, 3] and missing.tolist() == [[1], [0], [1]] and distinct.tolist() == [[3], [0], [2]]
    # codes 0 and 1 tie at two rows: the smaller code first; code 2 falls behind the cut; the empty scope is all padding
    assert code.tolist() == [[[0, 1]], [[-1, -1]], [[1, 2]]] and count.tolist() == [[[2, 2]], [[0, 0]], [[1, 1]]]
    assert (total.dtype, missing.dtype, distinct.dtype, code.dtype, count.dtype) == (np.int64, np.int64, np.int32, np.int32, np.int64)
    # a code outside [0, n_codes) is a row without a value; a row outside [0, n_rows) is counted nowhere
    total, missing, distinct, code, count = FC.evaluate([0, 5], [0, 2, 5, 6, -1], codes, [2], 3)
    assert total.tolist() == [3] and missing.tolist() == [[1]] and code.tolist() == [[[0, 1, -1]]] and count.tolist() == [[[1, 1, 0]]]
    # two fields of different widths in one call
    two = np.array([[0, 0, 1, -1, 1, 2], [5, 5, 5, 5, 0, 0]], dtype=np.int32)
    total, missing, distinct, code, count = FC.evaluate([0, 6], np.arange(6), two, [3, 6], 2)
    assert missing.tolist() == [[1, 0]] and distinct.tolist() == [[3, 2]]
    assert code.tolist() == [[[0, 1], [5, 0]]] and count.tolist() == [[[2, 2], [4, 2]]]


def test_the_families_hold_what_they_promise():
    fam = FC.families()
    assert len(fam) == len(FC.WIDTHS) + 10
    for name, c in fam.items():
        lens = np.diff(c["scope_ptr"])
        assert c["codes"].dtype == np.int32 and c["codes"].shape[0] == len(c["n_codes"]) and 1 <= c["top"] <= FC.MAX_TOP, name
        for p in range(lens.size):  # strictly ascending inside [0, n_rows)
            r = c["rows"][c["scope_ptr"][p]:c["scope_ptr"][p + 1]]
            assert (np.diff(r) > 0).all() and (r.size == 0 or (r[0] >= 0 and r[-1] < c["codes"].shape[1])), name
        if name not in ("ties",):
            assert tuple(lens) == FC.LENGTHS, name
    total, missing, distinct, code, count = FC.evaluate(**FC.ties_case())
    assert code[0, 0].tolist() == list(range(7)) and count[0, 0].tolist() == [6] * 7 and distinct[0, 0] == 40
    assert code[1, 0].tolist() == list(range(7)) and count[1, 0].tolist() == [1] * 7
    total, missing, distinct, code, count = FC.evaluate(**fam["hot-bin"])
    assert (distinct[1:] == 1).all() and (count[1:, :, 0] == total[1:, None]).all() and (code[1:, 1, 0] == FC.B + 8).all()
    total, missing, distinct, code, count = FC.evaluate(**fam["all-missing"])
    assert (missing == total[:, None]).all() and (distinct == 0).all() and (code == -1).all() and (count == 0).all()
    total, missing, distinct, code, count = FC.evaluate(**fam["stray-codes"])
    assert (missing[2:] > 0).all() and (missing + count.sum(axis=2) <= total[:, None]).all()
    total, missing, distinct, code, count = FC.evaluate(**fam["padded"])
    assert (distinct[:, 0] <= 3).all() and (code[:, 0, 3:] == -1).all() and (count[:, 0, 3:] == 0).all()
    total, missing, distinct, code, count = FC.evaluate(**fam["all-distinct"])
    assert (distinct[:, 0] == total).all() and (count[-1, 0] == 1).all() and (np.diff(code[-1, 0]) > 0).all()


def _chunk(i, law="UCC", chapter=None, section=None, article=None):
    return SimpleNamespace(id=f"c{i}", law_name=law, chapter=chapter, section=section, article_id=article)


def test_resolver_codes_number_values_by_first_appearance_and_none_is_minus_one():
    from legal_rag_amd.retrieval.scope import FACET_FIELDS, ScopeResolver
    chunks = [_chunk(0, chapter="Sales", article="2-101"), _chunk(1, chapter="Leases", section="Part 1", article="2A-101"),
              _chunk(2, chapter="Sales", section="Part 2", article="2-201"), _chunk(3), _chunk(4, chapter="General", article=7),
              _chunk(5, chapter="Leases", section="Part 1", article="2A-102")]
    res = ScopeResolver(chunks)
    assert FACET_FIELDS == ("law_name", "chapter", "section", "article_id")
    codes, values = res.codes("chapter")
    assert codes.dtype == np.int32 and codes.tolist() == [0, 1, 0, -1, 2, 1] and values == ["Sales", "Leases", "General"]
    assert res.codes("section")[0].tolist() == [-1, 0, 1, -1, -1, 0] and res.codes("section")[1] == ["Part 1", "Part 2"]
    assert res.codes("law_name")[0].tolist() == [0] * 6 and res.codes("law_name")[1] == ["UCC"]
    assert res.codes("article_id")[0].tolist() == [0, 1, 2, -1, 3, 4] and res.codes("article_id")[1][3] == "7"  # values are str
    # cached beside the row cache, read-only
    assert res.codes("chapter") is res.codes("chapter") and res.codes("chapter")[0] is codes
    with pytest.raises(ValueError):
        codes[0] = 5
    for bad in ("id", "text", "", "Chapter"):
        with pytest.raises(ValueError, match="not a facet field"):
            res.codes(bad)
    # the operand of the kernel: one field-major array per tuple of fields, cached as well
    cols, vals = res.code_columns(("chapter", "law_name"))
    assert cols.dtype == np.int32 and cols.flags.c_contiguous and cols.tolist() == [[0, 1, 0, -1, 2, 1], [0] * 6]
    assert vals == [["Sales", "Leases", "General"], ["UCC"]] and res.code_columns(("chapter", "law_name"))[0] is cols
    assert res.code_columns(("law_name", "chapter"))[0].tolist() == [[0] * 6, [0, 1, 0, -1, 2, 1]]
    # an empty list, and a field no chunk carries
    empty = ScopeResolver([])
    assert empty.codes("chapter")[0].shape == (0,) and empty.codes("chapter")[1] == [] and empty.code_columns(("chapter",))[0].shape == (1, 0)
    assert ScopeResolver([_chunk(0), _chunk(1)]).codes("section")[0].tolist() == [-1, -1]


def test_facets_validation():
    from legal_rag_amd.retrieval.facets import MAX_TOP, Facets
    assert Facets() == Facets(by=("chapter",), top=10) and MAX_TOP == FC.MAX_TOP
    assert Facets(by=["law_name", "section"]).by == ("law_name", "section") and hash(Facets(by=["chapter"])) == hash(Facets())
    with pytest.raises(Exception):
        Facets().top = 3  # frozen
    for by in ((), []):
        with pytest.raises(ValueError, match="no field"):
            Facets(by=by)
    for by in (("id",), ("chapter", "text"), ("Chapter",)):
        with pytest.raises(ValueError, match="not a facet field"):
            Facets(by=by)
    with pytest.raises(ValueError, match="twice"):
        Facets(by=("chapter", "section", "chapter"))
    for by in ("chapter", None, 3, (3,), ("chapter", None)):
        with pytest.raises(TypeError):
            Facets(by=by)
    for top in (0, -1, 65, 1000):
        with pytest.raises(ValueError, match="top"):
            Facets(top=top)
    for top in (True, 2.0, "3", None):
        with pytest.raises(TypeError):
            Facets(top=top)
    assert Facets(top=1).top == 1 and Facets(top=64).top == 64


def test_build_decodes_the_kernel_arrays_in_its_order():
    from legal_rag_amd.retrieval.facets import FacetCounts, Facets, build
    spec = Facets(by=("chapter", "law_name"), top=2)
    codes = np.array([[0, 0, 1, -1, 1, 2], [0] * 6], dtype=np.int32)
    got = FC.evaluate([0, 6, 6, 9], [0, 1, 2, 3, 4, 5, 2, 3, 5], codes, [3, 1], 2)
    out = build(spec, [["Sales", "Leases", "General"], ["UCC"]], *got)
    assert all(isinstance(o, FacetCounts) for o in out) and [o.total for o in out] == [6, 0, 3]
    assert list(out[0].fields) == ["chapter", "law_name"]
    assert out[0].fields["chapter"].values == [("Sales", 2), ("Leases", 2)]
    assert (out[0].fields["chapter"].distinct, out[0].fields["chapter"].missing) == (3, 1)
    assert out[0].fields["law_name"].values == [("UCC", 6)] and out[0].fields["law_name"].missing == 0
    assert out[1].fields["chapter"].values == [] and out[1].fields["chapter"].distinct == 0
    assert out[2].fields["chapter"].values == [("Leases", 1), ("General", 1)] and out[2].fields["chapter"].missing == 1

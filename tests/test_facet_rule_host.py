"""Host check of the rules of amdr_facet_counts (csrc/facet_rule.hpp: a tile's part of a scope, a row's bin, the counter
layout, the order key and the padding, the argument and table validation) through csrc/check_facets.cpp: a program of its
own, compiled for the host alone with the address and undefined-behaviour sanitizers (host flags only: no device code is
built) and run as a child process (no GPU, nothing loaded into Python).  It walks tiles and bins as the kernels do, on arrays
of exactly the promised sizes — the histogram of one block among them — and compares every output with a naive count."""
import subprocess

import pytest

import facet_cases as FC
from bm25_update_cases import build_check_program

FAMILIES = tuple(f"n_codes={w}" for w in FC.WIDTHS) + ("same", "distinct", "none", "stray", "fields", "ties", "many")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_facets")


def test_facet_rule_families_written_out_cases_and_validation(program):
    from legal_rag_amd import _native
    assert "amdr_facet_counts_device" in _native.EXPORTS and "amdr_facet_counts" in _native.EXPORTS
    assert "amdr_facet_plan" in _native.EXPORTS
    assert (_native.FACET_TILE_ROWS, _native.FACET_LDS_BINS, _native.FACET_MAX_TOP) == (FC.T, FC.B, FC.MAX_TOP)
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("facet rule ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert "FAIL" not in r.stdout
    assert r.stdout.count("family ok") == len(FAMILIES)
    for name in FAMILIES:
        assert r.stdout.count(f"facets {name}:") == 1, name
    assert r.stdout.count("written-out ok") == 1 and r.stdout.count("validate ok") == 1


def test_the_header_exports_the_shape_constants_the_rule_uses():
    import re
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    header = (root / "include" / "amdretrieval.h").read_text()
    rule = (root / "legal-rag_amd" / "csrc" / "facet_rule.hpp").read_text()
    for name, const, want in (("AMDR_FACET_TILE_ROWS", "kFcTile", FC.T), ("AMDR_FACET_LDS_BINS", "kFcBins", FC.B),
                              ("AMDR_FACET_MAX_TOP", "kFcMaxTop", FC.MAX_TOP)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == want
        assert int(re.search(rf"constexpr int {const} = (\d+);", rule).group(1)) == want


def test_facet_plan_is_the_counter_bytes():
    from legal_rag_amd import _native
    assert _native.facet_plan(3, [3, 5]) == 3 * (4 + 6) * 4
    assert _native.facet_plan(0, [7]) == 0 and _native.facet_plan(70_000, [0]) == 70_000 * 4
    assert _native.facet_plan(2, [FC.B + 1] * 8) == 2 * 8 * (FC.B + 2) * 4
    for n_cons, n_codes in ((-1, [3]), (1, []), (1, [1] * 9), (1, [-1]), (1, [2 ** 31])):
        with pytest.raises(_native.NativeError):
            _native.facet_plan(n_cons, n_codes)

"""Host check of the rules of amdr_unit_spans (csrc/unit_span_rule.hpp: an item's shape, one round decided from the ballots
of the unit starts and of every slot, the carry of the open unit, the validation) through csrc/check_unit_span.cpp: a
program of its own, compiled for the host alone with the address and undefined-behaviour sanitizers (host flags only: no
device code is built) and run as a child process (no GPU, nothing loaded into Python).  It resolves generated items tile by
tile and round by round as the kernels do, on arrays of exactly the promised sizes — the tokens and the break bytes of one
round among them — behind lists that stand before, and compares the lists with a naive scan of every unit that decides the
unordered form by a bipartite matching."""
import subprocess

import pytest

from bm25_update_cases import build_check_program

SIZES = (40, 300, 900)   # documents: one tile, two tiles, four tiles of the longest driver
COUNTS = (1, 2, 65)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_unit_span")


def test_unit_span_rule_families_written_out_cases_and_validation(program):
    from legal_rag_amd import _native
    assert "amdr_unit_spans_device" in _native.EXPORTS
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("unit span rule ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert "FAIL" not in r.stdout
    assert r.stdout.count("family ok") == len(SIZES) * len(COUNTS)
    for n in SIZES:
        for k in COUNTS:
            assert r.stdout.count(f"unit spans n={n} count={k}:") == 1, (n, k)
    assert r.stdout.count("written-out ok") == 1 and r.stdout.count("validate ok") == 1

"""Host check of the rules of amdr_vocab_match (csrc/vocab_match_rule.hpp: the bounded UTF-8 decoder, the wildcard matcher,
the banded optimal-string-alignment distance, the length pre-test, the bitmap, the fixed-stride write and the validation)
through csrc/check_vocab_match.cpp: a program of its own, compiled for the host alone with the address and
undefined-behaviour sanitizers (host flags only: no device code is built) and run as a child process (no GPU, nothing loaded
into Python).  It walks cells, bitmaps and rows as the kernels do, on arrays of exactly the promised sizes, and compares every
output byte with a naive full-matrix evaluation."""
import subprocess

import pytest

from bm25_update_cases import build_check_program

FAMILIES = ("fuzzy-ascii", "fuzzy-unicode", "wildcard-ascii", "wildcard-unicode", "mixed", "sizes", "cap")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_vocab_match")


def test_vocab_match_rule_families_written_out_cases_garbage_and_validation(program):
    from legal_rag_amd import _native
    from legal_rag_amd.retrieval.terms import Fuzzy, Wildcard  # noqa: F401 (the rule these classes restate)
    assert {"amdr_vocab_create", "amdr_vocab_match_device", "amdr_vocab_match", "amdr_vocab_match_plan"} <= set(_native.EXPORTS)
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("vocab match rule ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert "FAIL" not in r.stdout
    assert r.stdout.count("family ok") == len(FAMILIES)
    for name in FAMILIES:
        assert r.stdout.count(f"vocab_match {name}:") == 1, name
    assert r.stdout.count("written-out ok") == 1 and r.stdout.count("garbage ok") == 1 and r.stdout.count("validate ok") == 1

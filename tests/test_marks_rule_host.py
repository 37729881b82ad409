"""Host check of the rules of amdr_bm25_marks (csrc/marks_rule.hpp: the slot mask of a token, one lane's share of a sequence
in a round over staged masks, the cover and its carry, the mark of a position, the window scan, the score and the arg-max
order, the validation) through csrc/check_marks.cpp: a program of its own, compiled for the host alone with the address and
undefined-behaviour sanitizers (host flags only: no device code is built) and run as a child process (no GPU, nothing loaded
into Python).  It walks generated documents round by round and lane by lane as the kernel does, on arrays of exactly the
promised sizes — the 79-mask staged run, the 79-word cover and the 1 024-mark list among them — and compares every output
with a naive scan of whole documents."""
import subprocess

import pytest

from bm25_update_cases import build_check_program

TERMS = (2, 4, 9)  # vocabulary sizes: nearly every token marked (documents past the cap) .. sparse marks


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_marks")


def test_marks_rule_families_written_out_cases_and_validation(program):
    from legal_rag_amd import _native
    assert "amdr_bm25_marks_device" in _native.EXPORTS
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("marks rule ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert "FAIL" not in r.stdout
    assert r.stdout.count("family ok") == len(TERMS)
    for n in TERMS:
        assert r.stdout.count(f"marks terms={n}:") == 1, n
    assert "longest staged run 79" in r.stdout
    assert r.stdout.count("written-out ok") == 1 and r.stdout.count("validate ok") == 1

"""Host check of the rules of amdr_term_scope (csrc/term_scope_rule.hpp: posting_has, group and constraint evaluation,
the driver choice and its length, the validation of the host twin; csrc/compact.hpp: the host forms of the scans) through
csrc/check_term_scope.cpp: a program of its own, compiled for the host alone with the address and undefined-behaviour
sanitizers (host flags only: no device code is built) and run as a child process (no GPU, nothing loaded into Python).
It resolves generated constraints tile by tile as the kernels do, on arrays of exactly the promised sizes, and compares
with a plain filter over a dense term x document matrix."""
import subprocess

import pytest

from bm25_update_cases import build_check_program

FAMILIES = ("must only", "any only (iota)", "not only (iota)", "all three", "multi-token groups", "a repeated term",
            "unknown terms", "base scopes", "driver ties")
SIZES = (1023, 1024, 1025, 2049, 4100)  # around one tile of 1 024 candidates, two tiles and one more, four and a part


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_term_scope")


def test_term_scope_rule_and_validation(program):
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("term scope rule ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert "FAIL" not in r.stdout
    assert r.stdout.count("family ok") == len(FAMILIES) * len(SIZES)
    for name in FAMILIES:
        for n in SIZES:
            assert r.stdout.count(f"{name} n={n}:") == 1, (name, n)
    assert r.stdout.count("tiny n=") == 2  # one and two documents: the iota form and both ends
    assert r.stdout.count("validate ok") == 1

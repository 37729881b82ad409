"""Host check of the rules of amdr_bm25_add (csrc/bm25_add_rule.hpp: the validation of an add's arrays, the term table of
the concatenation, the tile's terms and the source of every output posting) through csrc/check_bm25_add.cpp: a program of
its own, compiled for the host alone with the address and undefined-behaviour sanitizers (host flags only: no device code
is built) and run as a child process (no GPU, nothing loaded into Python).  It merges generated indexes tile by tile as
the kernel does, on arrays of exactly the promised sizes, and compares with a plain per-term concatenation."""
import subprocess

import pytest

from bm25_update_cases import build_check_program


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_bm25_add")


def test_merge_rule_and_validation(program):
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and "bm25 add rule ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count("merge ok") == 7
    assert "FAIL" not in r.stdout

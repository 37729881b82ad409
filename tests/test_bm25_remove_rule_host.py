"""Host check of the rules of amdr_bm25_remove (csrc/bm25_remove_rule.hpp: the validation of the call's arrays, the
document map, a posting's rank, the new term table, a surviving posting's place; csrc/compact.hpp: the host forms of the
scans) through csrc/check_bm25_remove.cpp: a program of its own, compiled for the host alone with the address and
undefined-behaviour sanitizers (host flags only: no device code is built) and run as a child process (no GPU, nothing
loaded into Python).  It compacts generated indexes tile by tile as the kernels do, on arrays of exactly the promised
sizes, and compares with a plain per-term filter plus a stable reorder by new term id."""
import subprocess

import pytest

from bm25_update_cases import build_check_program


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_bm25_remove")


def test_compaction_rule_and_validation(program):
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("bm25 remove rule ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count("compact ok") == 12
    assert "FAIL" not in r.stdout

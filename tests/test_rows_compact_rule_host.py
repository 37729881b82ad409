"""Host check of the rules of amdr_dense_remove and amdr_maxsim_remove (csrc/rows_compact.hpp: the validation of the
removal list, the old row of a new row by one search and by the walk along a range, the segmented map of token rows;
csrc/compact.hpp: the host form of the scan) through csrc/check_rows_compact.cpp: a program of its own, compiled for the
host alone with the address and undefined-behaviour sanitizers (host flags only: no device code is built) and run as a
child process (no GPU, nothing loaded into Python).  It compacts generated matrices slab by slab as the kernels do, on
arrays of exactly the promised sizes, and compares with a plain filter."""
import subprocess

import pytest

from bm25_update_cases import build_check_program


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_rows_compact")


def test_row_compaction_rule_and_validation(program):
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("rows compact rule ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert "FAIL" not in r.stdout
    # 8 shapes x 7 patterns and the one-row matrix (first, last, everything, a single id); 2 stores x 6 patterns + 2
    assert r.stdout.count("uniform ok") == 8 * 7 + 4
    assert r.stdout.count("segments ok") == 2 * 6 + 2
    assert r.stdout.count("validate ok") == 1
    for pattern in ("first", "last", "one adjacent run", "alternating", "all but one", "everything", "a single id"):
        assert f" {pattern}:" in r.stdout, pattern

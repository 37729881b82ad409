"""Host check of the replace rules of amdr_dense_replace and amdr_maxsim_replace (csrc/rows_compact.hpp rs_*: a document's
place in the replace list, its length and signed source row afterwards, the source of every new token row) through
csrc/check_rows_replace.cpp: a program of its own, compiled for the host alone with the address and undefined-behaviour
sanitizers (host flags only: no device code is built) and run as a child process (no GPU, nothing loaded into Python).
It edits generated stores unit by unit and slab by slab as the kernels do, on arrays of exactly the promised sizes, and
compares with a brute-force edit, byte for byte."""
import subprocess

import pytest

from bm25_update_cases import build_check_program


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_rows_replace")


def test_row_replace_rules(program):
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("rows replace rule ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert "FAIL" not in r.stdout
    # rows 1 and 2: 4 and 6 patterns; 31, 32, 33, 65, 1 025: all 7; 3 row widths each
    assert r.stdout.count("uniform ok") == (4 + 6 + 5 * 7) * 3
    # stores of 1, 7, 40 and 300 documents: 4, 6, 7 and 7 patterns; 4 kinds of new lengths each
    assert r.stdout.count("segments ok") == (4 + 6 + 7 + 7) * 4
    for pattern in ("first", "last", "one adjacent run", "alternating", "all but one", "every row", "a single id"):
        assert f" {pattern}" in r.stdout, pattern

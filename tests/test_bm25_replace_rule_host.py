"""Host check of the rules of amdr_bm25_replace (csrc/bm25_replace_rule.hpp: the validation of the call's arrays and the
inverse term map, the document map, a new term's document frequency, where a surviving old posting and where an add
posting goes; with the tile ranks of csrc/bm25_remove_rule.hpp and the scans of csrc/compact.hpp) through
csrc/check_bm25_replace.cpp: a program of its own, compiled for the host alone with the address and undefined-behaviour
sanitizers (host flags only: no device code is built) and run as a child process (no GPU, nothing loaded into Python).
It merges generated indexes tile by tile as the kernels do, on arrays of exactly the promised sizes, and compares with a
brute-force edit, byte for byte."""
import re
import subprocess

import pytest

from bm25_update_cases import build_check_program


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_bm25_replace")


def test_replace_rule_and_validation(program):
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("bm25 replace rule ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert "FAIL" not in r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("merge ok: ")]
    assert len(lines) == 19
    for case in ("smallest index", "one document", "the first and the last document", "every document",
                 "one-token replacements", "the tile edges of a head list of 3 tiles", "a tile less one", "a tile exactly",
                 "a tile and one more", "3 tiles and five more", "an add of more than a tile", "a wide run of empty terms"):
        assert any(case in ln for ln in lines), case
    # the generated cases do hold what they are named for: emptied terms, new terms, lists that come from the add alone,
    # term-table windows too wide for the kernels' LDS window
    got = [tuple(int(x) for x in re.search(r"\((\d+) emptied, (\d+) new, (\d+) from the add alone\)", ln).groups())
           for ln in lines]
    assert sum(g[0] > 0 for g in got) >= 3 and sum(g[1] > 0 for g in got) >= 10 and sum(g[2] > 0 for g in got) >= 2, got
    assert any(int(re.search(r"(\d+) window\(s\)", ln).group(1)) > 0 for ln in lines)

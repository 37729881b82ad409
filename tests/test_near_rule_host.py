"""Host check of the rules of amdr_span_lists (csrc/near_rule.hpp: what an item is, one lane's share of a round on the staged
token run, the validation of a mixed batch; over csrc/phrase_rule.hpp's driver and conjunction) through
csrc/check_near_scope.cpp: a program of its own, compiled for the host alone with the address and undefined-behaviour
sanitizers (host flags only: no device code is built) and run as a child process (no GPU, nothing loaded into Python).
It resolves generated Nears and phrases tile by tile, round by round and lane by lane as the kernels do, on arrays of
exactly the promised sizes — the staged run of at most 64 + n tokens among them — and compares the lists with a naive
scan of every window of every document."""
import subprocess

import pytest

from bm25_update_cases import build_check_program

SIZES = (40, 300, 900)    # below one tile of 256 candidates, one tile and a part, three tiles and a part
COUNTS = (1, 2, 65)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_near_scope")


def test_near_rule_written_out_cases_and_validation(program):
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("near rule ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert "FAIL" not in r.stdout
    assert r.stdout.count("family ok") == len(SIZES) * len(COUNTS)
    for n in SIZES:
        for k in COUNTS:
            assert r.stdout.count(f"nears n={n} count={k}:") == 1, (n, k)
    assert "longest staged run 319" in r.stdout  # a whole run of 64 + 255 tokens was staged and scanned
    assert r.stdout.count("written-out ok") == 1 and r.stdout.count("validate ok") == 1

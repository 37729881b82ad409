"""Host check of the rules of amdr_phrase_lists (csrc/phrase_rule.hpp: the driver, the conjunction, one lane's share of a
document's scan, the validation of the phrases and of a token stream) and of the term step over virtual posting lists
(csrc/term_scope_rule.hpp: posting_has, ts_driver and ts_candidate on the lists, ts_validate_lists) through
csrc/check_phrase_scope.cpp: a program of its own, compiled for the host alone with the address and undefined-behaviour
sanitizers (host flags only: no device code is built) and run as a child process (no GPU, nothing loaded into Python).
It resolves generated phrases tile by tile and lane by lane as the kernels do, on arrays of exactly the promised sizes,
hands the lists to the term step, and compares both with a naive scan of every document."""
import subprocess

import pytest

from bm25_update_cases import build_check_program

SIZES = (40, 300, 900)    # below one tile of 256 candidates, one tile and a part, three tiles and a part
COUNTS = (1, 2, 65)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_phrase_scope")


def test_phrase_rule_term_step_and_validation(program):
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("phrase rule ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert "FAIL" not in r.stdout
    assert r.stdout.count("family ok") == len(SIZES) * len(COUNTS)
    for n in SIZES:
        for k in COUNTS:
            assert r.stdout.count(f"phrases n={n} count={k}:") == 1, (n, k)
    assert r.stdout.count("validate ok") == 1

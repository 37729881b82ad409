"""Host check of the rules of the carrying updates (csrc/tok_carry_rule.hpp: the validation of the add's token arrays, where
a document of the new stream takes its text from, a token through the term map, the conditions of the device's flag)
through csrc/check_tok_carry.cpp: a program of its own, compiled for the host alone with the address and
undefined-behaviour sanitizers (host flags only: no device code is built) and run as a child process (no GPU, nothing
loaded into Python).  It carries generated streams tile by tile as the kernel does, on arrays of exactly the promised
sizes, and compares with a plain per-document rebuild."""
import subprocess

import pytest

from bm25_update_cases import build_check_program

FAMILIES = ("one tile", "two tiles", "four tiles", "exactly 2047 tokens", "exactly 2048 tokens", "exactly 2049 tokens",
            "exactly 4097 tokens", "a document of 5000 tokens", "a run of 2051 empty documents")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_tok_carry")


def test_carry_rule_and_validation(program):
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("tok carry rule ok"), (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    for name in FAMILIES:
        assert sum(1 for x in lines if x.startswith(f"carry ok: {name}:")) == 1, name
    assert r.stdout.count("carry ok") == len(FAMILIES) and r.stdout.count("validate ok") == 1
    assert "FAIL" not in r.stdout
    # the families that are there for one thing each say that it happened
    long_doc = next(x for x in lines if x.startswith("carry ok: a document of 5000 tokens:"))
    assert " 3 document(s) across three tiles" in long_doc
    empties = next(x for x in lines if x.startswith("carry ok: a run of 2051 empty documents:"))
    assert " 3 window(s) searched in the table itself" in empties
    for total in (2047, 2048, 2049, 4097):
        line = next(x for x in lines if x.startswith(f"carry ok: exactly {total} tokens:"))
        assert f"new streams of {total} / {total} / {total} tokens" in line

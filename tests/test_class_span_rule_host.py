"""Host check of the rules of amdr_class_spans (csrc/class_span_rule.hpp: a slot resolved, the mask of the slots a token
fills, one lane's share of a round over staged masks, the driver among posting lists and class lists, the conjunction, the
validation with the overlap rule) through csrc/check_class_span.cpp: a program of its own, compiled for the host alone with
the address and undefined-behaviour sanitizers (host flags only: no device code is built) and run as a child process (no
GPU, nothing loaded into Python).  It resolves generated items tile by tile, round by round and lane by lane as the kernels
do, on arrays of exactly the promised sizes — the staged masks of one round among them — behind lists that stand before, and
compares the lists with a naive scan that decides the unordered form by a bipartite matching."""
import subprocess

import pytest

from bm25_update_cases import build_check_program

SIZES = (40, 300, 900)   # documents: one tile, two tiles, four tiles of the longest driver
COUNTS = (1, 2, 65)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_class_span")


def test_class_span_rule_families_written_out_cases_and_validation(program):
    from legal_rag_amd import _native
    assert "amdr_class_spans_device" in _native.EXPORTS
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("class span rule ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert "FAIL" not in r.stdout
    assert r.stdout.count("family ok") == len(SIZES) * len(COUNTS)
    for n in SIZES:
        for k in COUNTS:
            assert r.stdout.count(f"class spans n={n} count={k}:") == 1, (n, k)
    assert r.stdout.count("written-out ok") == 1 and r.stdout.count("validate ok") == 1

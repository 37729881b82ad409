"""Host check of the rules of amdr_union_lists (csrc/union_rule.hpp: a tile's part of a posting list, a document's word and
bit, the expansion of a word, the clamp, the validation) through csrc/check_union_lists.cpp: a program of its own, compiled
for the host alone with the address and undefined-behaviour sanitizers (host flags only: no device code is built) and run as
a child process (no GPU, nothing loaded into Python).  It resolves generated union items cell by cell and word by word as
the kernels do, on arrays of exactly the promised sizes — the bitmap of one tile among them — and compares the lists with a
naive set union."""
import subprocess

import pytest

from bm25_update_cases import build_check_program

TILE = 32768
SIZES = (33, TILE - 1, TILE + 1, 3 * TILE + 1)    # one word and a bit, one tile less a document, two tiles, four tiles
COUNTS = (1, 2, 65)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_check_program(tmp_path_factory, "check_union_lists")


def test_union_rule_families_written_out_cases_and_validation(program):
    from legal_rag_amd import _native
    assert _native.UNION_TILE == TILE
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("union rule ok"), (r.stdout[-3000:], r.stderr[-3000:])
    assert "FAIL" not in r.stdout
    assert r.stdout.count("family ok") == len(SIZES) * len(COUNTS)
    for n in SIZES:
        for k in COUNTS:
            assert r.stdout.count(f"unions n={n} count={k}:") == 1, (n, k)
    assert r.stdout.count("written-out ok") == 1 and r.stdout.count("validate ok") == 1

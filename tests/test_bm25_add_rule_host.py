"""Host check of the rules of amdr_bm25_add (csrc/bm25_add_rule.hpp: the validation of an add's arrays, the term table of
the concatenation, the tile's terms and the source of every output posting) through csrc/check_bm25_add.cpp: a program of
its own, compiled for the host alone with the address and undefined-behaviour sanitizers (host flags only: no device code
is built) and run as a child process (no GPU, nothing loaded into Python).  It merges generated indexes tile by tile as
the kernel does, on arrays of exactly the promised sizes, and compares with a plain per-term concatenation."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "legal-rag_amd" / "csrc"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (Path(hipcc).exists() or shutil.which(hipcc)):
        pytest.fail(f"{hipcc} not found: the host check is compiled with the compiler that builds the library")
    exe = tmp_path_factory.mktemp("bm25_add_rule") / "check_bm25_add"
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                    "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", str(CSRC / "check_bm25_add.cpp"), "-o", str(exe)],
                   check=True, cwd=str(CSRC))
    return exe


def test_merge_rule_and_validation(program):
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and "bm25 add rule ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count("merge ok") == 7
    assert "FAIL" not in r.stdout

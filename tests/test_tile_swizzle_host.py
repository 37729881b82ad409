"""Host check of csrc/tile_swizzle.hpp — the one statement of the LDS tile swizzles, the LDS-DMA piece offsets, the
accumulator row map and the power-of-two scale rule that the matrix kernels share — through csrc/check_tile_swizzle.cpp:
a program of its own, compiled for the host alone with the address and undefined-behaviour sanitizers (host flags only:
no device code is built) and run as a child process (no GPU, nothing loaded into Python)."""
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
    exe = tmp_path_factory.mktemp("tile_swizzle") / "check_tile_swizzle"
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address",
                    "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    str(CSRC / "check_tile_swizzle.cpp"), "-o", str(exe)], check=True, cwd=str(CSRC))
    return exe


def test_ring_swizzles_row_map_and_scale_rule(program):
    """Every ring shape in use lands each source unit where tile_off reads it, both swizzles are bijections, mfma32_row
    is a permutation of the 32 rows, pow2_exp scales 0 / subnormals / FLT_MIN / 1 / FLT_MAX / infinity / NaN as stated."""
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and "tile swizzle ok" in r.stdout, (r.stdout, r.stderr)

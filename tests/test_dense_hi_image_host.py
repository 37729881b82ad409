"""Host checks of csrc/dense_hi_image.hpp — the one statement of the fp16 image's addressing and conversion that the
builder kernel, the scan and the host share — through csrc/check_dense_hi_image.cpp: a program of its own, compiled for
the host alone with the address and undefined-behaviour sanitizers (host flags only: no device code is built) and run as a child process (no GPU, nothing loaded into
Python)."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "legal-rag_amd" / "csrc"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (Path(hipcc).exists() or shutil.which(hipcc)):
        pytest.fail(f"{hipcc} not found: the host check is compiled with the compiler that builds the library")
    exe = tmp_path_factory.mktemp("hi_image") / "check_dense_hi_image"
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address",
                    "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=all", str(CSRC / "check_dense_hi_image.cpp"), "-o", str(exe)],
                   check=True, cwd=str(CSRC))
    return exe


def test_image_addressing_is_a_bijection(program):
    r = subprocess.run([str(program)], capture_output=True, text=True)
    assert r.returncode == 0 and "addressing ok" in r.stdout, (r.stdout, r.stderr)


@pytest.mark.parametrize("scale_exp", [0, -10, 20, 99])
def test_conversion_is_numpy_float16_rounding(program, tmp_path, scale_exp):
    """hi_half(x, s) == float16(x * s) for a power-of-two s: normals, ties, fp16's subnormal range, what rounds to zero,
    what overflows to infinity, signed zeros, infinities."""
    rng = np.random.default_rng(100 + scale_exp)
    scale = np.float32(2.0) ** np.float32(scale_exp)
    inv = np.float32(1) / scale
    x = np.concatenate([
        rng.standard_normal(3000).astype(np.float32),                                   # normals
        (rng.standard_normal(1500) * 2.0 ** -16).astype(np.float32),                    # fp16 subnormals after rounding
        (rng.standard_normal(500) * 2.0 ** -24).astype(np.float32),                     # around the smallest subnormal
        (np.arange(-600, 600, dtype=np.float32) * np.float32(2.0 ** -12) + np.float32(1)),  # exact ties at 1 + j 2^-11
        np.array([0.0, -0.0, 1.0, -1.0, 65504.0, 65519.9, 65520.0, 7e4, np.inf, -np.inf, 2.0 ** -25, 2.0 ** -24 * 1.5,
                  -2.0 ** -25 * 1.0000001], dtype=np.float32),
    ]).astype(np.float32) * inv
    x = x[np.isfinite(x) | np.isinf(x)]
    src, dst = tmp_path / "x.f32", tmp_path / "y.f16"
    x.tofile(src)
    r = subprocess.run([str(program), str(src), str(dst), repr(float(scale))], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.fromfile(dst, dtype=np.uint16)
    with np.errstate(over="ignore"):
        want = (x * scale).astype(np.float16).view(np.uint16)
    assert got.shape == want.shape and len(got) > 6000
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(x[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    assert np.count_nonzero((want & 0x7c00) == 0) > 500  # zeros and subnormals were among them

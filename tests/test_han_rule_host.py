"""Host checks of the Han modes of the BM25 query tokeniser (csrc/tokenize_rule.hpp, reached through csrc/tokenize.cpp's
C ABI) through csrc/check_tokenize_han.cpp: a program of its own, compiled for the host alone with the address and
undefined-behaviour sanitizers (host flags only: no device code is built) and run as a child process (no GPU, nothing
loaded into Python).  It cuts the adversary list, the fuzz and byte splices of both — text that is not UTF-8 included —
in both modes and checks that the spans tile each text inside its bounds with tokens <= bytes; the sanitizers make any
access outside the route scratch, the dictionary table or the text a failure."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import han_adversary as H

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "legal-rag_amd" / "csrc"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (Path(hipcc).exists() or shutil.which(hipcc)):
        pytest.fail(f"{hipcc} not found: the host check is compiled with the compiler that builds the library")
    exe = tmp_path_factory.mktemp("han_rule") / "check_tokenize_han"
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                    "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", str(CSRC / "check_tokenize_han.cpp"),
                    str(CSRC / "tokenize.cpp"), "-lpthread", "-o", str(exe)], check=True, cwd=str(CSRC))
    return exe


def write_blob(path, items):
    enc = [x.encode("utf-8") for x in items]
    offs = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum([len(e) for e in enc], out=offs[1:])
    with open(path, "wb") as f:
        f.write(np.int64(len(enc)).tobytes() + offs.tobytes() + b"".join(enc))


@pytest.mark.parametrize("which", ["known", "fuzz"])
def test_spans_tile_every_text_in_both_modes(program, tmp_path, which):
    from legal_rag_amd import text
    d = text.load_han_dict(H.KNOWN_DICT_LINES if which == "known" else H.fuzz_dict_lines())
    keys, logw, word, unknown = d.native_tables()
    texts = H.adversary_texts() + [s for s, _ in H.KNOWN_DICT_ANSWERS] + H.fuzz_texts()
    write_blob(tmp_path / "keys", keys)
    write_blob(tmp_path / "texts", texts)
    logw.tofile(tmp_path / "logw")
    word.tofile(tmp_path / "word")
    r = subprocess.run([str(program), str(tmp_path / "keys"), str(tmp_path / "logw"), str(tmp_path / "word"),
                        repr(float(unknown)), str(tmp_path / "texts")], capture_output=True, text=True)
    assert r.returncode == 0 and "han rule ok" in r.stdout, (r.stdout, r.stderr[-3000:])
    assert f"({len(texts)} given)" in r.stdout

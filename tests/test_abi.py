"""The C-ABI shared library loads and exports every symbol include/amdretrieval.h
declares (no compute calls: this runs without a GPU)."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def header_symbols():
    src = (ROOT / "include" / "amdretrieval.h").read_text()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(amdr_[a-z0-9_]+)\s*\(", src)))


def test_library_is_built_in_tree():
    from legal_rag_amd import _native
    p = _native.lib_path()
    assert p.exists(), f"{p} missing: run __graft_entry__.build()"
    assert ROOT in p.parents


def test_every_declared_symbol_is_exported():
    from legal_rag_amd import _native
    lib = ctypes.CDLL(str(_native.lib_path()))
    syms = header_symbols()
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in amdretrieval.h but not exported"


def test_binding_table_matches_header():
    from legal_rag_amd import _native
    assert sorted(_native.EXPORTS) == header_symbols()


def header_prototypes():
    """name -> argument kinds ('P' pointer, 'i' int32_t, 'l' int64_t, 'd' double) parsed from the header."""
    src = (ROOT / "include" / "amdretrieval.h").read_text()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(amdr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        kinds = ""
        for a in [x.strip() for x in args.split(",") if x.strip() and x.strip() != "void"]:
            if "*" in a:
                kinds += "P"
            elif re.search(r"\bint64_t\b", a):
                kinds += "l"
            elif re.search(r"\bint32_t\b|\bint\b", a):
                kinds += "i"
            elif re.search(r"\bdouble\b", a):
                kinds += "d"
            else:
                raise AssertionError(f"{name}: unrecognised parameter '{a}'")
        out[name] = kinds
    return out


def test_argtypes_table_matches_header_prototypes():
    """Every export has ctypes argtypes, and they are the header's parameter kinds (no call depends
    on a wrapper remembering to wrap a Python int in the right width)."""
    from legal_rag_amd import _native
    protos = header_prototypes()
    assert sorted(protos) == sorted(_native.EXPORTS)
    for name, kinds in protos.items():
        assert _native.SIGNATURES[name] == kinds, (name, _native.SIGNATURES[name], kinds)
    lib = _native.load()
    for name in _native.EXPORTS:
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == len(protos[name])


def test_version_and_error_string_without_gpu():
    from legal_rag_amd import _native
    lib = _native.load()
    assert lib.amdr_version() >= 100
    # a bad-argument call fails loudly with a message and never touches a device
    rc = lib.amdr_dense_create(None, ctypes.c_int64(4), ctypes.c_int32(770), ctypes.c_int32(0), None)
    assert rc == -1
    assert b"out is null" in lib.amdr_last_error()


def test_no_cpu_fallback_in_product():
    """The product package must not import the oracle."""
    pkg = ROOT / "legal-rag_amd"
    for py in pkg.rglob("*.py"):
        txt = py.read_text(encoding="utf-8")
        assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f"{py} imports the oracle"


def test_dense_workspace_covers_every_pass(monkeypatch):
    """A batched dense search reserves its workspace once and then runs passes of the full chunk and a remainder:
    the slab-list space slabs(m) * m * k * 8 is NOT monotone in the pass size m (10 M rows through the full score
    matrix, k = 10: 96 queries take 22 slabs = 168 960 B, the 89-query remainder 24 slabs = 170 880 B), so the
    reservation must be the maximum over the passes.  Host-only arithmetic (amdr_dense_workspace_plan): no device."""
    from legal_rag_amd import _native
    checked = two_level = 0
    for n in (13_000_000, 12_345_678, 20_000_000, 40_000_000, 3_000_000, 600_000):
        for k in (1, 10, 80, 256):
            for nq in (5, 37, 95, 96, 97, 100, 131, 185, 191, 192, 193, 250, 1000):
                res, used = _native.dense_workspace_plan(n, 768, nq, k, nq, k)
                assert all(u <= r for u, r in zip(used, res)), (n, k, nq, res, used)
                checked += 1
                two_level += int(res[2] > 0)
    assert checked > 300 and two_level > 50
    # the advisor's worked example, pinned, on the form that has slab lists (the full score matrix, chunks of 96 on
    # 10 M rows): remainder 89 needs more list space than the chunk of 96
    monkeypatch.setenv("AMDR_DENSE_TWO_LEVEL", "0")
    res, used = _native.dense_workspace_plan(10_000_000, 768, 185, 10, 185, 10)
    assert used[1] == 170880 and res[1] >= used[1]
    assert _native.dense_workspace_plan(10_000_000, 768, 96, 10, 96, 10)[1][1] == 168960
    assert _native.dense_workspace_plan(10_000_000, 768, 89, 10, 89, 10)[1][1] == 170880
    # the exact two-level form (32-query tiles, chunks of 96): M [m][ldM] | S2 [m][32 k] in smat, list [m][k] | count [m]
    # in aux, each rounded up to 256 B, and in part the slab lists of the top-k over the n / 32 tile maxima alone.  Never
    # more than the form it replaced needed, which re-scored the UNION of the pass's m * k candidate tiles for every
    # query (S2 [m][32 m k], and its slab lists; aux: tile ids + maxima m * k * 12 B, the union (m * k + 64) * 4 B, 512 B
    # of padding)
    monkeypatch.setenv("AMDR_DENSE_TWO_LEVEL", "1")
    monkeypatch.setenv("AMDR_DENSE_HI", "0")
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    chunk = lambda nq, k: min(nq, min(96, max(32, 8192 // k // 32 * 32)))  # noqa: E731
    ld_m = lambda n: ((n + 31) // 32 + 31) // 32 * 32  # noqa: E731

    def now(n, m, k):
        return up(m * ld_m(n) * 4) + up(m * 32 * k * 4), up(m * k * 4) + up(m * 4)

    def lists(cols, m, k):  # slab lists of a top-k pass over m rows of `cols` scores
        if m == 0:
            return 0
        sl = max(1, min(-(-2048 // m), -(-cols // 16384)))
        per = (-(-cols // sl) + 63) // 64 * 64
        return -(-cols // per) * m * k * 8

    def before(n, m, k):
        return up(m * ld_m(n) * 4) + up(m * 32 * m * k * 4), m * k * 12 + (m * k + 64) * 4 + 512

    for n in (13_000_000, 12_345_678, 20_000_000, 40_000_000, 3_000_000, 600_000):
        for k in (1, 10, 80, 256):
            for nq in (5, 37, 95, 96, 97, 100, 131, 185, 191, 192, 193, 250, 1000):
                res, used = _native.dense_workspace_plan(n, 768, nq, k, nq, k)
                assert (used[0], used[2]) == now(n, chunk(nq, k), k), (n, k, nq, used)
                assert used[1] == max(lists((n + 31) // 32, m, k) for m in {chunk(nq, k), nq % chunk(nq, k)}), (n, k, nq, used)
                old_used = before(n, chunk(nq, k), k)
                old_res = [max(before(n, chunk(nq, kk), kk)[c] for kk in range(1, k + 1)) for c in (0, 1)]
                assert used[0] <= old_used[0] and used[2] <= old_used[1], (n, k, nq, used, old_used)
                assert res[0] <= old_res[0] and res[2] <= old_res[1], (n, k, nq, res, old_res)
    # the fp16 first pass (chunks of 64, k + 23 candidate tiles per query) and the exact chain behind its flag
    for hi in ("0", "1"):
        monkeypatch.setenv("AMDR_DENSE_HI", hi)
        for n in (13_000_000, 600_000, 40_000):
            for d in (128, 384, 768, 896, 1024):
                for k in (1, 10, 80, 127, 128):
                    for nq in (5, 37, 64, 65, 100, 129):
                        res, used = _native.dense_workspace_plan(n, d, nq, k, nq, k)
                        assert all(u <= r for u, r in zip(used, res)), (hi, n, d, k, nq, res, used)


# nq_max / nq of the reserve sweeps: 1-9 (the 1-4 query forms and the first batches), around a 64-query pass, and the
# largest serving batch
SWEEP_NQ = (1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 37_376)
SWEEP_K = tuple(range(1, 257))


def _reserve_sweep(plan):
    """plan(nq_max, k_max, nq, k) -> (reserved, used).  Asserts that reserve(nq_max, k_max) covers every call with
    nq <= nq_max and k <= k_max over SWEEP_NQ x SWEEP_K; returns the number of (reserve, call) pairs covered."""
    import numpy as np
    R = np.zeros((len(SWEEP_NQ), len(SWEEP_K)), dtype=np.int64)
    U = np.zeros_like(R)
    for a, nq in enumerate(SWEEP_NQ):
        for b, k in enumerate(SWEEP_K):
            R[a, b], U[a, b] = plan(nq, k, nq, k)
    # the largest use of any call within (SWEEP_NQ[a], SWEEP_K[b]): a running maximum over both axes
    need = np.maximum.accumulate(np.maximum.accumulate(U, axis=0), axis=1)
    bad = np.argwhere(need > R)
    assert bad.size == 0, [(SWEEP_NQ[a], SWEEP_K[b], int(R[a, b]), int(need[a, b])) for a, b in bad[:8]]
    return int(sum((a + 1) * (b + 1) for a in range(R.shape[0]) for b in range(R.shape[1])))


def test_bm25_reserve_covers_every_call():
    """amdr_bm25_reserve(nq_max, k_max) sizes the slab lists of every "_device" call with nq <= nq_max, k <= k_max:
    the slab size depends on k (arg-max slabs of 2 048 documents for a shallow k, 4 096 beyond), so a smaller k can
    need more list space than k_max.  Host-only arithmetic (amdr_bm25_workspace_plan): no device."""
    from legal_rag_amd import _native
    for n in (1, 591, 1260, 2048, 2049, 4097, 5000, 100_000, 10_000_000):
        assert _reserve_sweep(lambda a, b, c, d: _native.bm25_workspace_plan(n, a, b, c, d)) > 10_000, n


# the dense sweep is thinner than SWEEP_NQ x SWEEP_K (a reserve of a batch on a large matrix evaluates tens of thousands of
# plans: ~1.5 ms): the batch sizes at which the form or the pass size changes, the depths at which topk_cap (64 | 65,
# 192 | 193), the fp16 pass's limit (127 | 128) and its candidate widths step
DENSE_NQ = (1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 95, 96, 97, 191, 192, 193, 255, 256, 257)
DENSE_NQ_LONG = (4095, 4096, 37_376)  # the short matrices: around the fp16 two-pass form, the largest serving batch
DENSE_K = tuple(range(1, 21)) + (63, 64, 65, 127, 128, 191, 192, 193, 255, 256)
DENSE_PINS = ({}, {"AMDR_DENSE_TWO_LEVEL": "1", "AMDR_DENSE_HI": "0"}, {"AMDR_DENSE_TWO_LEVEL": "1", "AMDR_DENSE_HI": "1"})


def test_dense_reserve_covers_every_call(monkeypatch):
    """amdr_dense_reserve(nq_max, k_max) sizes smat, part and aux for every "_device" call with nq <= nq_max, k <= k_max,
    whichever form the call takes.  The scan's slab lists grid_x(nq, k) * nq * k * 8 are monotone in neither argument:
    20 000 rows, (4, 192) takes 625 row slabs = 3 840 000 B where (4, 256) takes 313 = 2 564 096 B; 200 000 x 100 (a
    dimension outside the MFMA forms: every batch scans), (8, 10) 1 231 360 B where (9, 10) takes 720 000 B.
    Host-only arithmetic (amdr_dense_workspace_plan): no device."""
    import numpy as np
    from legal_rag_amd import _native

    def sweep(n, d, nqs, ks):
        R = np.zeros((len(nqs), len(ks), 3), dtype=np.int64)
        U = np.zeros_like(R)
        for a, nq in enumerate(nqs):
            for b, k in enumerate(ks):
                R[a, b], U[a, b] = _native.dense_workspace_plan(n, d, nq, k, nq, k)
        need = np.maximum.accumulate(np.maximum.accumulate(U, axis=0), axis=1)
        bad = np.argwhere(need > R)  # separately for smat, part and aux
        assert bad.size == 0, (n, d, [(nqs[a], ks[b], ("smat", "part", "aux")[c], int(R[a, b, c]), int(need[a, b, c]))
                                      for a, b, c in bad[:8]])
        return bool(np.any(need > U))  # some smaller call uses more than the call at (nq_max, k_max) itself

    non_monotone = 0
    for n, d in ((20_000, 128), (20_000, 768), (200_000, 100)):
        non_monotone += sweep(n, d, DENSE_NQ, DENSE_K)
    for n, d in ((600, 768), (1024, 768)):
        non_monotone += sweep(n, d, DENSE_NQ + DENSE_NQ_LONG, DENSE_K)
    for pins in DENSE_PINS:
        for key, v in pins.items():
            monkeypatch.setenv(key, v)
        non_monotone += sweep(600_000, 768, DENSE_NQ, DENSE_K)
        for d in (768, 1024):
            non_monotone += sweep(13_000_000, d, DENSE_NQ, DENSE_K)
    assert non_monotone >= 3
    # the two worked examples: the smaller call needs more than the call at the bounds, and the reserve covers it
    for n, d, nq_max, k_max, nq, k, part in ((20_000, 128, 4, 256, 4, 192, 3_840_000), (20_000, 768, 4, 256, 4, 192, 3_840_000),
                                             (200_000, 100, 9, 10, 8, 10, 1_231_360)):
        res, used = _native.dense_workspace_plan(n, d, nq_max, k_max, nq, k)
        assert used[1] == part and res[1] >= part, (n, d, res, used)
        assert _native.dense_workspace_plan(n, d, nq_max, k_max, nq_max, k_max)[1][1] < part


@pytest.mark.parametrize("n, k_max, ks", [(100_000, 17, range(9, 17)), (5000, 18, range(13, 18)),
                                          (2049, 29, range(15, 29))], ids=["100k-docs", "5000-docs", "2049-docs"])
def test_bm25_reserve_worked_examples(n, k_max, ks):
    """Depths below k_max that take more slabs than k_max itself (2 048-document arg-max slabs against 4 096)."""
    from legal_rag_amd import _native
    for nq_max in (1, 64, 37_376):
        for k in ks:
            res, used = _native.bm25_workspace_plan(n, nq_max, k_max, nq_max, k)
            assert used > _native.bm25_workspace_plan(n, nq_max, k_max, nq_max, k_max)[1], (n, k_max, k)
            assert used <= res, (n, nq_max, k_max, k, res, used)


def test_maxsim_reserve_covers_every_call(monkeypatch):
    """amdr_maxsim_reserve(nq_max, k_max) sizes the workspace of every "_device" call within it: a call with
    4 k <= n_docs takes the two-pass form (three row blocks, the item table, 16 KB of query image per query) even when
    4 k_max > n_docs keeps the reserve's own shape one-pass.  With and without the split-fp16 image, and with the
    two-pass form pinned off.  Host-only arithmetic (amdr_maxsim_workspace_plan): no device."""
    from legal_rag_amd import _native
    for split in (True, False):
        for n in (1, 7, 8, 9, 40, 74, 158, 200, 591, 1260):
            assert _reserve_sweep(lambda a, b, c, d: _native.maxsim_workspace_plan(n, split, a, b, c, d)) > 10_000
    # the two-pass figure is the end of the layout the call runs in: aligned like its row blocks, three of them and more;
    # at a fixed depth no region shrinks with the batch
    two_pass = 0
    for n in (8, 40, 74, 591, 1260):
        for k in (1, 2, 10, 18, 147, 256):
            last = 0
            for nq in SWEEP_NQ:
                used = _native.maxsim_workspace_plan(n, True, nq, k, nq, k)[1]
                rows = (nq * n * 4 + 255) // 256 * 256
                assert used >= last, (n, k, nq, used, last)
                last = used
                if nq >= 8 and 4 * k <= n:
                    assert used % 256 == 0 and used > 3 * rows, (n, k, nq, used, rows)
                    two_pass += 1
                else:
                    assert used == rows, (n, k, nq, used, rows)
    assert two_pass >= 100
    # without the image (a store with a NaN / infinity) or with the two-pass form pinned off: one-pass rows only
    rows = (64 * 74 * 4 + 255) // 256 * 256
    assert _native.maxsim_workspace_plan(74, False, 64, 80, 64, 10) == (rows, rows)
    monkeypatch.setenv("AMDR_MAXSIM_TWOPASS", "0")
    assert _native.maxsim_workspace_plan(74, True, 64, 80, 64, 10) == (rows, rows)
    assert _reserve_sweep(lambda a, b, c, d: _native.maxsim_workspace_plan(74, True, a, b, c, d)) > 10_000


@pytest.mark.parametrize("n, k_max, ks", [(74, 80, range(10, 19)), (40, 20, (1, 5, 10)), (158, 80, (1, 10, 39)),
                                          (200, 80, (1, 10, 50)), (200, 256, (1, 10, 50)),
                                          (591, 256, (1, 10, 147))],
                         ids=["74-docs-civil-code-rank", "40-docs", "158-docs", "200-docs-k80",
                              "200-docs-k256", "591-docs"])
def test_maxsim_reserve_worked_examples(n, k_max, ks):
    """4 k_max > n_docs keeps the reserve's own shape one-pass, but these depths (4 k <= n_docs) take the two-pass
    layout.  74 documents (one rank of an 8-way Civil-Code shard), reserve(64, 80): ~19 KB of one-pass rows against
    ~1.16 MB for a call at k = 10-18."""
    from legal_rag_amd import _native
    for k in ks:
        res, used = _native.maxsim_workspace_plan(n, True, 64, k_max, 64, k)
        assert used > _native.maxsim_workspace_plan(n, True, 64, k_max, 64, k_max)[1], (n, k_max, k)
        assert used <= res, (n, k_max, k, res, used)
    if n == 74:
        assert _native.maxsim_workspace_plan(74, True, 64, 80, 64, 10)[1] > 1_000_000

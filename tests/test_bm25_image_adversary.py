"""The data of tests/bm25_image_adversary.py is what it claims (CPU only), so that the GPU tests built on it cannot pass
vacuously: the scores are exact by construction, the image runs collide in fp32 and differ in fp64 with at least k equal
members before the differing one, and a restatement of bm25_select_f32 whose check stops at the pairs below k — the
check before it was widened to the whole run that reaches the cut — decides every F1 / F3(b) case wrongly."""
import numpy as np
import pytest

import bm25_image_adversary as IA


@pytest.fixture(scope="module")
def cases():
    return IA.hand_made()


def _row(c):
    return IA.ref_scores(c.csr, c.queries[:1])[0]


def test_scores_are_the_idf_values_bit_for_bit(cases):
    for c in cases[::7] + IA.fuzz(nq=2)[::5]:
        assert np.all(IA.posting_factor(c.csr) == 1.0)
        idf = c.csr["idf"]
        row = IA.ref_scores(c.csr, [c.queries[0]])[0]
        exp = np.zeros(c.n)
        for t in c.queries[0]:
            exp[c.csr["post_doc"][c.csr["term_ptr"][t]]] = 0.0 + idf[t] * 1.0
        assert np.array_equal(row.view(np.uint64), exp.view(np.uint64)), c.name
    # query order, duplicates counted, unknown ids skipped
    csr = IA.csr_per_document(np.array([0.1, 0.2, 0.3]))
    got = IA.ref_scores(csr, [[2, -1, 0, 2, 3, 7]])[0]
    assert got.tolist() == [0.0 + 0.1, 0.0, (0.0 + 0.3) + 0.3]


def test_the_restated_plan():
    want = {200: (208, 4), 448: (448, 8), 591: (592, 10), 1000: (1008, 16), 1260: (1264, 20), 2048: (2048, 32)}
    for n, (slab, nvt) in want.items():
        assert IA.bm_plan(n, 10)[:2] == (slab, 1) and IA.nvt_bucket(slab) == nvt
    assert IA.bm_plan(5000, 16) == (1680, 3, True) and IA.bm_plan(9000, 16) == (1808, 5, True)
    assert IA.bm_plan(5000, 17)[2] and IA.bm_plan(5000, 18) == (2512, 2, False) and IA.bm_plan(2048, 17) == (2048, 1, False)
    assert IA.bm_plan(1260, 17)[2] and IA.bm_plan(591, 40)[2] and not IA.bm_plan(1000, 40)[2]
    assert IA.bm_plan(448, 65)[2] and not IA.selector_runs(448, 65) and not IA.bm_plan(448, 100)[2]
    assert IA.plan_text(9000, 10) == ("slabs=5 of <= 1808 documents", IA.ARGMAX)


def test_every_shape_depth_and_family_is_there(cases):
    seen = {(c.family, c.n, c.k) for c in cases}
    for n in IA.SHAPES:
        for k in IA.selector_depths(n):
            assert ("F4", n, k) in seen, (n, k)
            if k <= 59:  # k equal scores and a larger one have to fit into 64 survivors; k = 64 is among the controls
                assert ("F1", n, k) in seen and ("F2", n, k) in seen, (n, k)
                assert sum(c.reach for c in cases if (c.family, c.n, c.k) == ("F1", n, k)) >= 5, (n, k)
        assert {k for f, m, k in seen if f == "control" and m == n} == set(IA.control_depths(n))
        assert any(f == "F3a" and m == n for f, m, k in seen)
        assert any(f == "F3b" and m == n for f, m, k in seen)
    assert {IA.nvt_bucket(IA.bm_plan(n, 10)[0]) for n in IA.SHAPES} == {4, 8, 10, 16, 20, 32}
    for n in IA.MULTI:
        nslabs = IA.bm_plan(n, 10)[1]
        assert {c.slab_ix for c in cases if c.family == "F1" and c.n == n} == {0, nslabs // 2, nslabs - 1}
    reach = [c for c in cases if c.reach]
    assert any("lane-63" in c.name for c in reach) and any("register>0" in c.name for c in reach)
    assert any("slab-end" in c.name for c in reach) and any(" neg" in c.name for c in reach)
    print(f"{len(cases)} hand-made cases, {len(reach)} built to be decided wrongly by the narrow check")


def test_runs_collide_in_fp32_and_differ_in_fp64(cases):
    for c in cases:
        if c.family not in ("F1", "F3a", "F3b", "F4") or not c.high:
            continue
        row = _row(c)
        x = row + 0.0
        run = np.array(c.run)
        assert np.all(np.diff(run) > 0)
        assert len(set(IA.images(row[run]).tolist())) == 1, c.name               # one image
        first = int(np.nonzero(x[run] != x[run[0]])[0][0])
        if "zero-images" in c.name:  # the larger score is not kept behind k equal ones here (more than 64 share the image)
            assert len(set(x[run].tolist())) > 1
            continue
        assert first >= c.k if c.family != "F3a" else first >= 64, c.name      # at least k members before it ...
        assert len(set(x[run[:first]].tolist())) == 1, c.name                    # ... exactly equal
        assert np.all(x[np.array(c.high)] > x[run[0]]), c.name                   # and it scores more
        ids, _ = IA.ref_topk(row, c.k)
        assert set(ids.tolist()) & set(c.high), c.name                            # the exact top k holds a high document
        assert min(c.run) >= IA.bm_plan(c.n, c.k)[0] * c.slab_ix


def test_f4_images_collide_as_stated(cases):
    f32 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32)
    kinds = {"+inf": 0, "-inf": 0, "zero": 0, "subnormal": 0}
    tiny = float(np.finfo(np.float32).tiny)
    with np.errstate(over="ignore", under="ignore"):
        for c in cases:
            if c.family != "F4":
                continue
            row = _row(c)
            r = row[np.array(c.run)]
            f = f32(r)
            assert len(set((r + 0.0).tolist())) > 1, c.name
            if "+inf" in c.name:
                assert np.all(f == np.inf) and np.all(np.isfinite(r)) and np.all(r > np.finfo(np.float32).max)
                kinds["+inf"] += 1
            elif "-inf" in c.name:
                assert np.all(f == -np.inf) and np.all(np.isfinite(r))
                kinds["-inf"] += 1
            elif "zero" in c.name:
                assert np.all(f == 0.0) and np.all(np.abs(r) < IA.SUB / 2)
                assert np.any(np.signbit(f)) or "untouched above" not in c.name       # -0.0 images fold onto +0.0
                kinds["zero"] += 1
            else:
                assert "subnormal" in c.name and np.all(f != 0) and np.all(np.abs(f) < tiny) and len(set(f.tolist())) == 1
                kinds["subnormal"] += 1
    assert all(v >= 10 for v in kinds.values()), kinds
    assert any(" neg" in c.name or "neg " in c.name for c in cases if c.family == "F4")


def _wrong(c, rows, whole_run):
    """Queries of the case that the restated selector DECIDES, and decides wrongly."""
    bad = 0
    for row in rows:
        sc, lo, nv = c.slab_scores(row)
        got = IA.select_model(sc, c.k, nv, whole_run)
        want = [int(i) - lo for i in IA.ref_topk(sc, min(c.k, len(sc)))[0]]
        bad += got is not None and got != want
    return bad


def test_the_narrow_check_decides_every_reaching_case_wrongly(cases):
    reach = [c for c in cases if c.reach]
    assert {c.family for c in reach} >= {"F1", "F3b", "F4"}
    assert all(c.reach for c in cases if c.family in ("F1", "F3b") and " at-k " not in c.name) and all(IA.selector_runs(c.n, c.k) for c in reach)
    for c in reach:
        rows = [_row(c)]
        assert _wrong(c, rows, False) == 1, c.name
        assert _wrong(c, rows, True) == 0, c.name
    for c in cases[::3]:
        if not c.reach and IA.selector_runs(c.n, c.k):
            assert _wrong(c, [_row(c)], True) == 0, c.name


def test_the_fuzz_reaches_the_gap_too():
    narrow = wide = total = 0
    for c in IA.fuzz():
        if not IA.selector_runs(c.n, c.k):
            continue
        rows = IA.ref_scores(c.csr, c.queries)
        total += len(rows)
        narrow += _wrong(c, rows, False)
        wide += _wrong(c, rows, True)
    print(f"fuzz: {total} queries, the narrow check decides {narrow} wrongly, the whole-run check {wide}")
    assert total >= 300 and narrow >= 20 and wide == 0

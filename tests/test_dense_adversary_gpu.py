"""The exact dense forms against inputs with one right answer (tests/dense_adversary.py).

Integer data (max|Q| * sum|x| < 2^24: order-free, exact in fp32): every form — the GEMV scan, one wave per (query, row),
the fp32-MFMA tiles, the panel kernel, the exact two-level top-k, and the two fp16 first passes in front of their exact
tails — returns the fp64 oracle's ids and score BITS, ties to the lower id, no tolerance and no near-tie exemption; so do
the other callers of dense_row_dot (score_rows: the full matrix; the scoped search; the serving step, asked for as one
launch) and a handle grown by amdr_dense_add.  Real-valued edge data: every score inside gamma_(d+8) sum|q x| of the
fp64 value, the full list in the kernel's own order, planted top-k ids exact with no position left out.  Every search
case first asserts, through amdr_dense_plan_info, that the form it names is the form that runs."""
import numpy as np
import pytest

import dense_adversary as DA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    return _native


def _search(idx, monkeypatch, form, Q, k, finite=True, image=False):
    """One search of `form`'s pins; asserts that plan_info names the form form_of expects.  -> (scores, ids, form run)."""
    n, nq = idx.ntotal, Q.shape[0]
    pins = DA.pins_of(form, nq)
    for name in DA.PIN_NAMES:
        monkeypatch.delenv(name, raising=False)
    for name, v in pins.items():
        monkeypatch.setenv(name, v)
    try:
        want = DA.form_of(n, idx.d, nq, k, pins, finite)
        plan = idx.plan_info(nq, k)
        assert DA.form_from_plan(plan) == want, (form, n, idx.d, nq, k, plan)
        if want == DA.HI:
            assert ("dense_hi_image_tilemax_kernel" in plan) == image, plan
        s, i = idx.search(Q, k)
    finally:
        for name in pins:
            monkeypatch.delenv(name, raising=False)
    return s, i, want


def _by_matrix(form, family):
    """The cases of a form by matrix shape; the position family has its own batches, which cover every K position."""
    shapes = {}
    for n, d, nq, k in (DA.position_cases(form) if family == "position" else DA.cases(form)):
        shapes.setdefault((n, d), []).append((nq, k))
    return shapes


def _assert_bits(s, i, es, ei, what):
    assert np.array_equal(i, ei), (what, "ids", np.argwhere(i != ei)[:4].tolist())
    assert DA.bits_equal(s, es), (what, "score bits", np.argwhere(s.view(np.uint32) != es.view(np.uint32))[:4].tolist())


@pytest.mark.parametrize("form", DA.FORMS)
@pytest.mark.parametrize("family", DA.INT_FAMILIES)
def test_integer_data_bit_for_bit(nat, monkeypatch, family, form):
    ran = 0
    for (n, d), lst in _by_matrix(form, family).items():
        X, a, _ = DA.integer_X(family, n, d)
        finite = DA.stats_finite(X)
        idx = nat.DenseIndex(X)
        for image in ((False, True) if form == DA.HI else (False,)):
            if image:
                idx.build_image()
            for nq, k in lst:
                Q, b = DA.integer_Q(family, n, d, nq, k)
                _, es, ei = DA.integer_expect(X, a, Q, b, k)
                if family == "position":  # every K position that has a row is in some query's list (asserted there)
                    assert np.array_equal(DA.position_case(n, d, nq, k)["ids"], ei)
                s, i, took = _search(idx, monkeypatch, form, Q, k, finite, image)
                # unscaled statistics never refuse a form; scaled ones may (then the exact form answers: the same bits)
                assert took == form or family.startswith("scale"), (family, form, took)
                _assert_bits(s, i, es, ei, (family, form, took, n, d, nq, k, "image" if image else ""))
                ran += 1
        idx.close()
    assert ran >= len(DA.position_cases(form) if family == "position" else DA.cases(form))


# the other callers of dense_row_dot, on the matrices of the RowWaves cases (every listed d) up to 1 025 rows
_ROW_DOT_SHAPES = sorted({(n, d) for n, d, _, _ in DA.cases(DA.ROWWAVES) if n <= 1025} | {(1025, 1024), (257, 260)})


@pytest.mark.parametrize("family", DA.INT_FAMILIES)
def test_integer_data_through_the_other_callers_of_the_row_dot(nat, monkeypatch, family):
    ws = nat.ScopeWorkspace()
    for n, d in _ROW_DOT_SHAPES:
        X, a, _ = DA.integer_X(family, n, d)
        idx = nat.DenseIndex(X)
        nq, k = 9, min(10, n)
        Q, b = DA.integer_Q(family, n, d, nq, k)
        S, es, ei = DA.integer_expect(X, a, Q, b, k)
        # score_rows: every (query, row) score — and -FLT_MAX for a row outside the matrix
        rows = np.tile(np.concatenate([np.arange(n), [-1, n]]), (nq, 1))
        got = idx.score_rows(Q, rows)
        assert DA.bits_equal(got[:, :n], S.astype(np.float32)), (family, n, d, "score_rows")
        assert np.all(got[:, n:] == -DA.FLT_MAX)
        # the scoped search: one scope of every row equals the search; one of every second row, the oracle on those rows
        s, i = ws.dense_search(idx, Q, [0, n], np.arange(n), np.zeros(nq, np.int32), k)
        _assert_bits(s, i, es, ei, (family, n, d, "scope: all rows"))
        half = np.arange(0, n, 2)
        kh = min(k, half.size)
        hs, hi = DA.oracle_topk(S[:, half], kh)
        s, i = ws.dense_search(idx, Q, [0, half.size], half, np.zeros(nq, np.int32), kh)
        _assert_bits(s, i, hs, half[hi], (family, n, d, "scope: every second row"))
        idx.close()
    ws.close()


@pytest.mark.parametrize("family", DA.INT_FAMILIES)
def test_integer_data_through_the_one_launch_serving_step(nat, monkeypatch, family):
    import torch
    from legal_rag_amd.retrieval.engine import HybridEngine
    from oracle import bm25 as OB
    # The library reports no plan for this step: amdr_hybrid_small_device decides natively (1-4 queries, <= 2 048 rows,
    # kd + kb <= 32, a BM25 index of one slab: at most 2 048 documents, as here) and otherwise runs the separate launches, the RowWaves
    # form again, without saying so.  What can be pinned is pinned; that the one launch ran is not proven here.
    monkeypatch.setenv("AMDR_HYBRID_SMALL", "1")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    for n, d in ((33, 4), (257, 260), (1023, 768), (1025, 1024), (591, 64)):
        X, a, _ = DA.integer_X(family, n, d)
        docs = [[f"w{j}" for j in rng.integers(0, 40, size=5)] for _ in range(n)]
        ob = OB.BM25Okapi(docs)
        csr = OB.to_csr(ob)
        eng = HybridEngine(nat.DenseIndex(X), nat.BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"],
                                                            csr["doc_len"], ob.avgdl, ob.k1, ob.b), None)
        for nq, k in ((1, 10), (4, 16), (3, 1)):
            k = min(k, n)
            Q, b = DA.integer_Q(family, n, d, nq, k)
            _, es, ei = DA.integer_expect(X, a, Q, b, k)
            qt_h, qp_h = nat.BM25Index.pack_queries([[int(t) for t in rng.integers(0, 40, size=4)] for _ in range(nq)])
            assert nq <= 4 and n <= 2048 and 2 * k <= 32
            r = eng.search_batch(nat.make_fuse_params(), k, q_emb=torch.from_numpy(Q).to(dev),
                                 q_terms=torch.from_numpy(qt_h).to(dev), q_ptr=torch.from_numpy(qp_h).to(dev))
            torch.cuda.synchronize()
            _assert_bits(r.dense_scores.cpu().numpy(), r.dense_ids.cpu().numpy(), es, ei, (family, n, d, nq, k, "one launch"))
        eng.dense.close()
        eng.bm25.close()


@pytest.mark.parametrize("form,n,d,nq,k", [(DA.ROWWAVES, 1025, 260, 4, 10), (DA.ROWWAVES, 257, 768, 1, 256),
                                           (DA.TILES, 1025, 768, 33, 10), (DA.TILES, 4099, 64, 9, 256),
                                           (DA.TWOLEVEL, 4099, 320, 33, 10), (DA.TWOLEVEL, 1025, 1024, 129, 1)])
@pytest.mark.parametrize("family", ["wide", "cancel", "scale-80-69"])
def test_add_path_gives_the_bits_of_one_create(nat, monkeypatch, family, form, n, d, nq, k):
    X, a, _ = DA.integer_X(family, n, d)
    Q, b = DA.integer_Q(family, n, d, nq, k)
    _, es, ei = DA.integer_expect(X, a, Q, b, k)
    third = n // 3
    idx = nat.DenseIndex(X[:third])
    idx.add(X[third:2 * third + 1])
    idx.add(X[2 * third + 1:])
    assert idx.ntotal == n
    s, i, took = _search(idx, monkeypatch, form, Q, k, DA.stats_finite(X))
    assert took == form
    _assert_bits(s, i, es, ei, (family, form, n, d, nq, k, "grown by two adds"))
    idx.close()
    one = nat.DenseIndex(X)
    s1, i1, _ = _search(one, monkeypatch, form, Q, k, DA.stats_finite(X))
    one.close()
    assert np.array_equal(i, i1) and DA.bits_equal(s, s1)


# ---- real-valued edges: the proven bound ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(DA.FULL_SHAPES))
@pytest.mark.parametrize("kind", DA.REAL_KINDS)
def test_real_data_full_matrix_inside_the_bound(nat, monkeypatch, kind, form):
    worst = 0.0
    for n, d, nq in DA.FULL_SHAPES[form]:
        X, Q = DA.real_case(kind, n, d, nq)
        S, B = DA.exact_scores(X, Q), DA.bound_matrix(X, Q)
        idx = nat.DenseIndex(X)
        s, i, took = _search(idx, monkeypatch, form, Q, n, DA.stats_finite(X))
        assert took == form
        ratio = DA.check_full_view(s, i, S, B)
        print(f"OBS dense {form} full {kind} n={n} d={d} nq={nq}: max |err| / bound {ratio:.4f}")
        assert ratio <= 1.0, (kind, form, n, d, nq, ratio)
        if form == DA.ROWWAVES:  # the full-matrix probe of the row dot itself
            got = idx.score_rows(Q, np.tile(np.arange(n), (nq, 1)))
            r2 = DA.check_bound(got, np.tile(np.arange(n), (nq, 1)), S, B)
            print(f"OBS dense score_rows {kind} n={n} d={d} nq={nq}: max |err| / bound {r2:.4f}")
            assert r2 <= 1.0, (kind, n, d, nq, r2)
        idx.close()
        worst = max(worst, ratio)
    print(f"OBS dense {form} full {kind}: largest |err| / bound {worst:.4f}")


@pytest.mark.parametrize("form", list(DA.PLANTED_SHAPES))
@pytest.mark.parametrize("kind", DA.REAL_KINDS)
def test_real_data_planted_topk_exact_ids_inside_the_bound(nat, monkeypatch, kind, form):
    worst = 0.0
    for n, d, nq, k in DA.PLANTED_SHAPES[form]:
        c = DA.planted_case(kind, n, d, nq, k)
        finite = DA.stats_finite(c["X"])
        idx = nat.DenseIndex(c["X"])
        for image in ((False, True) if form == DA.HI and finite else (False,)):
            if image:
                idx.build_image()
            s, i, took = _search(idx, monkeypatch, form, c["Q"], k, finite, image)
            assert took == form or not finite, (kind, form, took)
            assert np.array_equal(i, c["ids"]), (kind, form, n, d, nq, k, np.argwhere(i != c["ids"])[:4].tolist())  # no position exempt
            ratio = DA.check_bound(s, i, c["S"], c["bound"])
            print(f"OBS dense {took} planted {kind} n={n} d={d} nq={nq} k={k}{' image' if image else ''}: max |err| / bound {ratio:.4f}")
            assert ratio <= 1.0, (kind, form, n, d, nq, k, ratio)
            worst = max(worst, ratio)
        idx.close()
    print(f"OBS dense {form} planted {kind}: largest |err| / bound {worst:.4f}")

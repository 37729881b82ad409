"""One live handle through a long seeded script of adds, removes, replaces and refused updates (update_sequence_cases.py).
After EVERY step the handle is compared with the model's bytes, with the exact reference computed from the model alone
(ids and score bits, every query, every checked (nq, k)), with the derived state the model predicts, and with a fresh
handle of the model's bytes."""
import numpy as np
import pytest
import torch

import dense_adversary as DA
import update_sequence_cases as C
from test_dense_remove_gpu import assert_same, bits
from test_dense_replace_gpu import assert_same_device

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


class Pins:
    """Environment pins for the calls inside (the library reads them per call); every other pin of the route is unset."""

    def __init__(self, monkeypatch, pins):
        self.mp, self.pins = monkeypatch, pins

    def __enter__(self):
        for name in DA.PIN_NAMES:
            self.mp.delenv(name, raising=False)
        for name, v in self.pins.items():
            self.mp.setenv(name, v)

    def __exit__(self, *exc):
        for name in self.pins:
            self.mp.delenv(name, raising=False)


def same_or_nan(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    both_nan = np.isnan(got) & np.isnan(want)
    return bool(np.all(both_nan | (bits(got) == bits(want)) | ((got == 0) & (want == 0))))


def search_both(nat, h, Qd, Q, nq, k):
    """search, and search_device inside the reserve the caller made (no workspace may grow): two (scores, ids)."""
    host = h.search(Q[:nq], k)
    s = torch.empty((nq, k), dtype=torch.float32, device=DEV)
    i = torch.empty((nq, k), dtype=torch.int64, device=DEV)
    g0 = nat.workspace_growths()
    h.search_device(Qd.data_ptr(), nq, k, s.data_ptr(), i.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert nat.workspace_growths() == g0, ("search_device grew a workspace", nq, k)
    torch.cuda.synchronize()
    return host, (s.cpu().numpy(), i.cpu().numpy())


def assert_list(got, want, what):
    (gs, gi), (es, ei) = got, want
    assert np.array_equal(gi, ei), (what, "ids", np.argwhere(gi != ei)[:4].tolist())
    assert DA.bits_equal(gs, es), (what, "score bits")


def apply(nat, g, st):
    op = st.op
    if op[0] == "build":
        g.build_image()
    elif op[0] == "add":
        g.add(op[1])
    elif op[0] == "remove":
        g.remove(op[1])
    elif op[0] == "replace":
        g.replace(op[1], op[2])
    elif op[0] == "refused":
        with pytest.raises(nat.NativeError, match="status -1"):
            getattr(g, op[1])(*op[2:])
    else:
        raise AssertionError(op[0])


def check_dense_state(nat, monkeypatch, profile, g, st, Q, Qd):
    p = C.PROFILES[profile]
    at = (profile, st.step, st.note)
    n, d = st.n, st.d
    # the primary bytes and the visible derived state: the model's, and a fresh handle's
    assert g.ntotal == n, at
    if n:
        assert np.array_equal(bits(g.read_rows(0, n)), bits(st.X)), at
    info = g.image_info()
    assert (info[0], info[2], info[3]) == st.image, (at, info)
    f = nat.DenseIndex(st.X) if n else nat.DenseIndex(dim=d)
    if st.image[0]:
        f.build_image()
        fi = f.image_info()
        assert (fi[0], fi[2], fi[3]) == st.image, (at, fi)
    finite = st.finite_rows
    if n:
        DA.assert_integer_budget(st.X[finite], Q)
    assert n == 0 or finite.size >= max(C.DENSE_KS), at  # (no list reaches a NaN row)
    # live against fresh through the per-operation modules' own comparisons (resident bytes, searches, score_rows)
    assert_same(g, f, Q, st.X)
    assert_same_device(g, f, Q)
    # and both against the exact reference
    for h, who in ((g, "live"), (f, "fresh")):
        h.reserve(C.NQ_ALL, max(C.DENSE_KS))
        for nq in C.DENSE_NQS:
            for k in C.DENSE_KS:
                want = C.expected_topk(profile, st.step, nq, k)
                for got, entry in zip(search_both(nat, h, Qd, Q, nq, k), ("search", "search_device")):
                    assert_list(got, want, (at, who, entry, nq, k))
        if n:
            rows = np.tile(np.asarray(st.seam + [n, -1], dtype=np.int64), (5, 1))
            with np.errstate(invalid="ignore"):
                want = DA.exact_scores(st.X[st.seam], Q[:5]).astype(np.float32)
            got = h.score_rows(Q[:5], rows)
            assert same_or_nan(got[:, :len(st.seam)], want), (at, who, "score_rows")
            assert np.all(got[:, len(st.seam):] == np.float32(-DA.FLT_MAX)), (at, who, "score_rows outside [0, n)")
            scope = np.asarray([r for r in st.seam if r in set(finite.tolist())], dtype=np.int64)
            ks = min(4, scope.size)
            ws = nat.ScopeWorkspace()
            got = ws.dense_search(h, Q[:4], np.asarray([0, scope.size], np.int64), scope, [0] * 4, ks)
            ws.close()
            assert_list(got, C.scoped_expected(st.X, Q[:4], scope, ks), (at, who, "scoped search"))
        if profile == "dense-short":
            # the long-batch form of a short corpus below 1 025 rows, the exact form above — on both sides of a crossing
            with Pins(monkeypatch, C.SHORT_PINS):
                h.reserve(C.NQ_ALL, max(C.DENSE_KS))  # (a reserve sizes the workspaces for the route under the pins)
                form = DA.form_from_plan(h.plan_info(64, 10))
                assert form == C.form_at(st, 64, 10, C.SHORT_PINS) and (form == DA.SMALL) == (n <= C.SHORT_MAX), (at, who, form)
                want = C.expected_topk(profile, st.step, 64, 10)
                for got, entry in zip(search_both(nat, h, Qd, Q, 64, 10), ("search", "search_device")):
                    assert_list(got, want, (at, who, "short-corpus pins", entry))
        if profile == "dense-rowwaves":
            form = DA.form_from_plan(h.plan_info(3, 10))
            assert form == (DA.ROWWAVES if n <= C.ROW_WAVES_MAX else DA.SCAN), (at, who, form)
            want = C.expected_topk(profile, st.step, 3, 10)
            for got, entry in zip(search_both(nat, h, Qd, Q, 3, 10), ("search", "search_device")):
                assert_list(got, want, (at, who, "3 queries", entry))
        if p["hi"]:
            check_hi(nat, monkeypatch, profile, h, who, st, Q, Qd)
    f.close()


def check_hi(nat, monkeypatch, profile, h, who, st, Q, Qd):
    """k = 10 under AMDR_DENSE_HI=1 + AMDR_DENSE_TWO_LEVEL=1, over the resident image and without it: the fp16 first pass
    took every query, resolved every one (no query fell back to the exact chain, which would hide a stale image), at width
    level 0, and is still in use."""
    at = (profile, st.step, st.note, who)
    for image in (True, False):
        pins = dict(C.HI_PINS, **({} if image else {"AMDR_DENSE_HI_IMAGE": "0"}))
        with Pins(monkeypatch, pins):
            want_form = C.form_at(st, 64, C.HI_K, C.HI_PINS)
            assert (want_form == DA.HI) == (st.n >= C.HI_MIN_ROWS), at
            h.reserve(C.NQ_ALL, max(C.DENSE_KS))  # (a reserve sizes the workspaces for the route under the pins)
            c0 = h.hi_counters()
            searched = 0
            for nq in C.HI_NQS:
                plan = h.plan_info(nq, C.HI_K)
                assert DA.form_from_plan(plan) == want_form, (at, plan)
                if want_form == DA.HI:
                    assert ("dense_hi_image_tilemax_kernel" in plan) == (image and st.image[0]), (at, plan)
                want = C.expected_topk(profile, st.step, nq, C.HI_K)
                for got, entry in zip(search_both(nat, h, Qd, Q, nq, C.HI_K), ("search", "search_device")):
                    assert_list(got, want, (at, "fp16 first pass", image, entry, nq))
                searched += 2 * nq
            c1 = h.hi_counters()
            took, unresolved = c1[0] - c0[0], c1[1] - c0[1]
            assert took == (searched if want_form == DA.HI else 0), (at, took, searched)
            assert unresolved == 0 and c1[5] == c0[5], (at, c0, c1)
            assert c1[2] == 0 and c1[3], (at, c1)


@pytest.mark.parametrize("profile", C.DENSE_PROFILES)
def test_dense_sequence(nat, monkeypatch, profile):
    for name in DA.PIN_NAMES:
        monkeypatch.delenv(name, raising=False)
    states = C.dense_states(profile)
    Q = C.dense_queries(profile)
    Qd = torch.from_numpy(Q).to(DEV)
    g = nat.DenseIndex(states[0].X)
    check_dense_state(nat, monkeypatch, profile, g, states[0], Q, Qd)
    for st in states[1:]:
        apply(nat, g, st)
        check_dense_state(nat, monkeypatch, profile, g, st, Q, Qd)
    g.close()


# ---- BM25 ---------------------------------------------------------------------------------------------------------------
def bm25_refused(nat, m, g, st):
    """The refusal through the product's path (ValueError before the native call) and the same arguments given to the
    native call itself, which refuses them on the host: amdr_bm25_remove / _replace validate before they enqueue."""
    from legal_rag_amd.bm25_model import docs_csr
    n = m.corpus_size
    idf = np.fromiter(m.idf.values(), dtype=np.float64, count=len(m.idf))
    which = st.op[1]
    if which == "remove id == n":
        with pytest.raises(ValueError):
            m.remove_documents([0, n])
        with pytest.raises(nat.NativeError, match="status -1"):
            g.remove(np.asarray([0, n], np.int64), idf, float(m.avgdl))
    elif which == "remove every document":
        with pytest.raises(ValueError):
            m.remove_documents(range(n))
        with pytest.raises(nat.NativeError, match="status -1"):
            g.remove(np.arange(n, dtype=np.int64), idf, float(m.avgdl))
    elif which == "replace an id twice":
        two = [["all", "z0"], ["all"]]
        with pytest.raises(ValueError):
            m.replace_documents([3, 3], two)
        tp, pd, pt = docs_csr([{"all": 1, "z0": 1}, {"all": 1}], m.vocab())
        with pytest.raises(nat.NativeError, match="status -1"):
            g.replace(np.asarray([3, 3], np.int64), tp, pd, pt, np.asarray([2, 1], np.int32), idf, float(m.avgdl))
    else:
        raise AssertionError(which)
    assert m.gpu(0) is g


def check_bm25_state(nat, g, st, tokens_before):
    from bm25_update_cases import SEARCHES, assert_same_results, same_arrays
    import class_span_cases as CC
    import near_cases as NC
    import phrase_cases as PC
    import union_cases as UC
    at = ("bm25", st.step, st.note)
    ob, csr = C.bm25_oracle(st.step)
    # the visible state, the primary bytes against the oracle's CSR, all six arrays against a fresh handle
    assert g.info()[:4] + g.info()[5:] + (g.replaces(),) == st.info(), (at, g.info(), g.replaces(), st.info())
    assert g.info()[4] == C.BM25_TILE, at
    assert g.tokens_info() == tokens_before, (at, g.tokens_info())
    got = g.read()
    for name, j in (("term_ptr", 0), ("post_doc", 1), ("post_tf", 2), ("idf", 4), ("doc_len", 5)):
        assert got[j].dtype == csr[name].dtype and got[j].tobytes() == csr[name].tobytes(), (at, name)
    f = nat.BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"], csr["doc_len"], float(ob.avgdl),
                      float(ob.k1), float(ob.b))
    same_arrays(got, f.read())
    # scores and every ranking against the oracle, bit for bit
    qs, words = C.bm25_queries(st.step)
    scores = g.get_scores(qs)
    exp = [np.asarray(ob.get_scores(w), dtype=np.float64) for w in words]
    for j in range(len(qs)):
        assert scores[j].tobytes() == exp[j].tobytes(), (at, "get_scores", j)
    for nq, k in SEARCHES:
        s, i = g.search(qs[:nq], k)
        for j in range(nq):
            order = sorted(range(st.n), key=lambda d: exp[j][d], reverse=True)[:k]  # (oracle.bm25.search's stable sort)
            assert i[j].tolist() == order and s[j].tobytes() == exp[j][order].tobytes(), (at, "search", nq, k, j)
    assert_same_results(nat, g, f, qs, st.at)
    # the token stream of the model, then one phrase, Near, union and class span with tokens of both sides of the seam
    corpus = PC.SeqCorpus(f"step{st.step}", len(st.vocab), [[st.vocab[w] for w in d] for d in st.docs])
    phrases, nears, unions, classes = C.bm25_span_items(st)
    stream = corpus.stream()
    for h, who in ((g, "live"), (f, "fresh")):
        h.set_tokens(*stream)
        assert h.tokens_info() == (True, int(stream[0][-1])), (at, who)
        lens = [PC.driver_len(corpus, p) for p in phrases]
        for got, want, what in (
                (h.phrase_lists(*PC.operands(phrases), max(lens), sum(lens)), PC.expected_lists(corpus, phrases), "phrase"),
                (h.span_lists(*NC.operands(nears), *NC.bounds(corpus, nears)), NC.expected_lists(corpus, nears), "near"),
                (h.union_lists(*UC.operands(unions), UC.rows_cap(corpus, unions)), UC.expected_lists(corpus, unions), "union"),
                (h.class_spans(*[x for part in CC.operands(classes, corpus.n_terms) for x in part], *CC.bounds(corpus, classes)),
                 CC.expected_lists(corpus, classes), "class span")):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and not got[2].any(), (at, who, what)
    f.close()
    return (True, int(stream[0][-1]))


def test_bm25_sequence(nat):
    from bm25_update_cases import fit
    states = C.bm25_states()
    m = fit(states[0].docs)
    g = m.gpu(0)
    tokens = check_bm25_state(nat, g, states[0], (False, 0))
    for st in states[1:]:
        if st.kind == "X":
            bm25_refused(nat, m, g, st)
            tokens = check_bm25_state(nat, g, st, tokens)  # the stream is still the one set before the refusal
            continue
        if st.kind == "A":
            m.add_documents(st.op[1])
        elif st.kind == "Rm":
            m.remove_documents(st.op[1])
        else:
            m.replace_documents(st.op[1], st.op[2])
        assert m.gpu(0) is g, st.note  # the product's path took the update in place
        tokens = check_bm25_state(nat, g, st, (False, 0))  # every successful update drops the stream
    g.close()


# ---- ColBERT ------------------------------------------------------------------------------------------------------------
def ms_apply(nat, g, st):
    op = st.op
    if op[0] == "add":
        g.add(*C.ms_store(op[1]))
    elif op[0] == "remove":
        g.remove(op[1])
    elif op[0] == "replace":
        g.replace(op[1], *C.ms_store(op[2]))
    else:
        n = st.n
        one = np.ones((1, C.MS_DIM), np.float32)
        with pytest.raises(nat.NativeError, match="status -1"):
            if op[1] == "remove id == n":
                g.remove([0, n])
            elif op[1] == "replace an id twice":
                g.replace([3, 3], np.concatenate([one, one]), np.asarray([0, 1, 2], np.int64))
            elif op[1] == "add an empty document":
                g.add(one, np.asarray([0, 1, 1], np.int64))
            elif op[1] == "remove every document":
                g.remove(np.arange(n))
            else:
                raise AssertionError(op[1])


def check_ms_state(nat, monkeypatch, g, st):
    import maxsim_adversary as MS
    at = ("colbert", st.step, st.note)
    Q = C.ms_queries()
    D, ptr = C.ms_store(st.docs)
    n = st.n
    # the primary bytes and the visible derived state: the model's, and a fresh handle's
    gD, gp = g.read()
    assert np.array_equal(gp, ptr) and gD.tobytes() == D.tobytes(), at
    assert g.info() == st.info(), (at, g.info(), st.info())
    f = nat.MaxSimIndex(D, ptr)
    fi = f.info()
    assert fi[:2] + fi[3:5] == st.info()[:2] + st.info()[3:5] and fi[5] == int(st.images), (at, fi)
    want = np.asarray(st.stats(), np.float32)
    for h, who in ((g, "live"), (f, "fresh")):
        assert np.asarray(h.stats(), np.float32).tobytes() == want.tobytes(), (at, who, h.stats(), want)
    finite = st.finite
    assert finite == bool(st.images), at
    if finite:
        exp_split, exp_f32 = MS.split_expected(D, ptr, Q), MS.f32_expected(D, ptr, Q)  # (the exactness budgets are asserted inside)
    else:
        exp_split = exp_f32 = MS.nonfinite_expected(D, ptr, Q)
    seam = sorted({min(max(r, 0), n - 1) for r in (st.at - 2, st.at - 1, st.at, st.at + 1, st.at + 2)})
    for h, who in ((g, "live"), (f, "fresh")):
        for pins in (MS.P_DEF, MS.P_F32, MS.P_ONE):
            for name in MS.PIN_NAMES:
                monkeypatch.delenv(name, raising=False)
            for name, v in pins.items():
                monkeypatch.setenv(name, v)
            for nq in C.MS_NQS:
                want_form = MS.form_of(n, nq, 1, True, pins, finite)
                assert MS.form_from_plan(h.plan_info(nq)) == want_form, (at, who, pins, nq, h.plan_info(nq))
                if not finite:
                    assert want_form in (MS.PAIRF32, MS.BLOCKED), (at, want_form)
                form = MS.form_of(n, nq, 1, False, pins, finite)
                exp = exp_split if form in MS.SPLIT_FORMS else exp_f32
                assert MS.same_scores(h.scores(Q[:nq]), exp[:nq]), (at, who, pins, "scores", nq, form)
                form = MS.form_of(n, nq, C.MS_K, True, pins, finite)
                exp = exp_split if form in MS.SPLIT_FORMS else exp_f32
                es, ei = MS.topk_expected(exp[:nq], C.MS_K)
                s, i = h.search(Q[:nq], C.MS_K)
                assert np.array_equal(i, ei) and MS.same_scores(s, es), (at, who, pins, "search", nq, form)
        for name in MS.PIN_NAMES:
            monkeypatch.delenv(name, raising=False)
        ws = nat.ScopeWorkspace()
        table = (np.asarray([0, len(seam)], np.int64), np.asarray(seam, np.int64), [0] * 7)
        if finite:
            s, i = ws.maxsim_search(h, Q[:7], *table, 4)
            es, ei = MS.topk_expected(exp_split[:7], 4, rows=[seam] * 7)
            assert np.array_equal(i, ei) and MS.same_scores(s, es), (at, who, "scoped search")
        else:
            with pytest.raises(nat.NativeError, match="split-fp16"):
                ws.maxsim_search(h, Q[:7], *table, 4)
        ws.close()
    f.close()


def test_colbert_sequence(nat, monkeypatch):
    states = C.ms_states()
    g = nat.MaxSimIndex(*C.ms_store(states[0].docs))
    check_ms_state(nat, monkeypatch, g, states[0])
    for st in states[1:]:
        ms_apply(nat, g, st)
        check_ms_state(nat, monkeypatch, g, st)
    g.close()


# ---- the serving step ---------------------------------------------------------------------------------------------------
def test_serving_sequence(nat):
    """Dense + BM25 edited in lockstep across 2 048 rows; the ENGINE object is kept, the fresh one is made per step.
    bm25_update_cases.assert_same_serving_step makes both engines itself, from the BM25 handles and a dense matrix of its
    own, on every call — it cannot keep an engine across the steps or take the edited dense handle —, so its comparison
    (test_hybrid_small_gpu's _run and _same, then the lists against the channels' own searches) is applied here to the
    kept engine; the helper itself runs once per step on the two BM25 handles as well."""
    from bm25_update_cases import assert_same_serving_step, fit, queries_for, same_pair
    from legal_rag_amd.retrieval.engine import HybridEngine
    from test_hybrid_small_gpu import _run, _same
    states = C.serving_states()
    m = fit(states[0].docs)
    gd, gb = nat.DenseIndex(states[0].X), m.gpu(0)
    eng = HybridEngine(gd, gb, None)
    params = nat.make_fuse_params(method="weighted_sum", min_final_score=0.0)
    seen = set()
    for st in states:
        if st.kind == "A":
            gd.add(st.op[1])
            m.add_documents(st.op[2])
        elif st.kind == "Rm":
            gd.remove(st.op[1])
            m.remove_documents(st.op[1].tolist())
        elif st.kind == "Rp":
            gd.replace(st.op[1], st.op[2])
            m.replace_documents(st.op[1].tolist(), st.op[3])
        elif st.kind == "X":
            with pytest.raises(nat.NativeError, match="status -1"):
                gd.remove([st.n])
            with pytest.raises(ValueError):
                m.remove_documents([st.n])
        assert m.gpu(0) is gb and gd.ntotal == gb.n_docs == st.n, st.note
        assert np.array_equal(bits(gd.read_rows(0, st.n)), bits(st.X)), st.note
        seen.add(st.n <= C.SERVING_MAX)
        mf = fit(st.docs)
        fd, fb = nat.DenseIndex(st.X), mf.gpu(0)
        fresh = HybridEngine(fd, fb, None)
        qs = queries_for(np.random.default_rng(7600 + st.step), gb.n_terms)
        rng = np.random.default_rng(7700 + st.step)
        for nq, k in ((1, 10), (2, 16), (3, 5), (4, 1)):
            q = rng.standard_normal((nq, C.SERVING_D)).astype(np.float32)
            q[0] = st.X[min(st.at, st.n - 1)]  # the row at the seam is query 0's best
            qt_h, qp_h = nat.BM25Index.pack_queries(qs[:nq])
            Q = torch.from_numpy(q).to(DEV)
            qt = torch.from_numpy(np.concatenate([qt_h, np.zeros(1, np.int32)])).to(DEV)
            qp = torch.from_numpy(qp_h).to(DEV)
            a, b = _run(eng, params, k, Q, qt, qp, True), _run(fresh, params, k, Q, qt, qp, True)
            _same(a, b, ("serving step", st.step, st.note, nq, k))
            assert a["dense_ids"][0, 0] == min(st.at, st.n - 1), (st.note, nq, k)
            same_pair((a["bm25_scores"], a["bm25_ids"]), gb.search(qs[:nq], k), ("serving step against search", st.note, nq, k))
            same_pair((a["dense_scores"], a["dense_ids"]), gd.search(q, k), ("serving step against dense search", st.note, nq, k))
        assert_same_serving_step(nat, gb, fb, qs)
        fd.close()
        fb.close()
    assert seen == {True, False}
    gd.close()
    gb.close()


@pytest.mark.parametrize("how", ["remove", "replace"])
def test_the_two_pass_bound_follows_a_scale_lowering_rebuild(nat, monkeypatch, how):
    """update_sequence_cases.ms_bound_case: the one large token goes, the scale exponent falls by three steps and the
    largest scaled token norm rises 4.6 times.  A handle that kept d_norm_max would search with a margin that loses a
    true top-10 document of every query (test_update_sequence certifies it on the fp64 model); the live handle returns the
    fp64 oracle's ids in the two-pass form, and the score bits of the one-pass form and of a fresh handle."""
    import maxsim_adversary as MS
    import rounding_adversary as RA
    for name in MS.PIN_NAMES:
        monkeypatch.delenv(name, raising=False)
    c = C.ms_bound_case()
    Q, (Da, pa), (Db, pb) = c["Q"], c["before"], c["after"]
    g = nat.MaxSimIndex(Da, pa)
    e0 = g.info()[3]
    assert MS.form_of(len(pa) - 1, len(Q), C.BOUND_K, True, MS.P_DEF) == MS.TWOPASS
    assert np.array_equal(g.search(Q, C.BOUND_K)[1], RA.topk_exact(RA.exact_maxsim(Q, Da, pa), C.BOUND_K)[1])
    if how == "remove":
        g.remove([0])
        D, ptr, top = Db, pb, c["top"]
    else:
        g.replace([0], c["small"], np.asarray([0, 1], np.int64))
        D, ptr, top = np.concatenate([c["small"], Db]), pa, c["top"] + 1
    assert np.array_equal(RA.topk_exact(RA.exact_maxsim(Q, D, ptr), C.BOUND_K)[1], top)
    gD, gp = g.read()
    assert np.array_equal(gp, ptr) and gD.tobytes() == D.tobytes()
    f = nat.MaxSimIndex(D, ptr)
    assert g.info()[3] == f.info()[3] == e0 + 3 and g.info()[4] == 1 and g.info()[5] == 2
    assert np.asarray(g.stats(), np.float32).tobytes() == np.asarray(f.stats(), np.float32).tobytes()
    # the bound against the fp64 value: a 128-term fp32 sum of squares and a square root, |rel. error| <= 131 * 2^-24
    want = C.ms_scaled_norm_max(D)
    assert g.stats()[0] == RA.maxsim_scales(Q, D)[0] and abs(g.stats()[1] - want) <= 131 * 2.0 ** -24 * want, (g.stats(), want)
    assert MS.form_from_plan(g.plan_info(len(Q))) == MS.TWOPASS
    s2, i2 = g.search(Q, C.BOUND_K)
    assert np.array_equal(i2, top)
    monkeypatch.setenv("AMDR_MAXSIM_TWOPASS", "0")
    s1, i1 = g.search(Q, C.BOUND_K)
    monkeypatch.delenv("AMDR_MAXSIM_TWOPASS")
    sf, i_f = f.search(Q, C.BOUND_K)
    assert np.array_equal(i1, top) and np.array_equal(i_f, top)
    assert s2.tobytes() == s1.tobytes() == sf.tobytes()
    g.close()
    f.close()

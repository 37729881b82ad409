"""Every MaxSim form, asserted to be the form that ran, against the one right answer of tests/maxsim_adversary.py: all
scores as uint32 bits (a zero by value), all ids, no tolerance, no skipped position.  A case runs scores(), search() at
every depth kind of its store and search_device() after reserve(), under each of its pins (default; AMDR_MAXSIM_F16X3=0
the fp32-input forms; AMDR_MAXSIM_TWOPASS=0 one pass), with and without AMDR_MAXSIM_DOCS=7; the route is checked against
MaxSimIndex.plan_info (which has no k: the route at depth 1) and, per depth, against the workspace a call takes (only the
two-pass layout exceeds the score rows).  Then the scoped form (host and device twins, default and 4-document slabs) and
the non-finite rule of include/amdretrieval.h on the fp32-input forms."""
import numpy as np
import pytest
import torch

import maxsim_adversary as MA

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CASES = {c["name"]: c for c in MA.cases()}


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    return _native


def _pin(mp, *envs):
    for name in MA.PIN_NAMES:
        mp.delenv(name, raising=False)
    env = {}
    for e in envs:
        env.update(e)
    for name, v in env.items():
        mp.setenv(name, v)
    return env


def _same(got_s, got_i, want_s, want_i, what):
    assert np.array_equal(got_i, want_i), (what, got_i.tolist(), want_i.tolist())
    assert MA.same_scores(got_s, want_s), (what, got_s.tolist(), want_s.tolist())
    assert not np.any(np.signbit(got_s) & (got_s == 0)), what  # top-k outputs: -0.0 as +0.0


def _device(idx, Q, k):
    nq, q_len = Q.shape[:2]
    q = torch.from_numpy(Q).to(DEV)
    s = torch.full((nq, k), 123.0, dtype=torch.float32, device=DEV)
    i = torch.full((nq, k), 77, dtype=torch.int64, device=DEV)
    idx.search_device(q.data_ptr(), nq, q_len, k, s.data_ptr(), i.data_ptr(), 0)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def _run(nat, mp, c, ks, pin_sets, finite=True, want=None):
    """Every entry point on the store of c under each pin set x DOCS7; want: the expected matrix whatever the form
    (default: by the form's arithmetic).  Returns {(pins, docs7): scores() matrix}."""
    D, ptr, Q = c["D"], c["doc_ptr"], c["Q"]
    n, nq = len(ptr) - 1, len(Q)
    out = {}
    for pi, pins in enumerate(pin_sets):
        for di, docs in enumerate(MA.DOCS7):
            env = _pin(mp, pins, docs)
            idx = nat.MaxSimIndex(D, ptr)
            assert idx.info()[4] == int(finite)
            assert MA.form_from_plan(idx.plan_info(nq)) == MA.form_of(n, nq, 1, True, env, finite), (env, idx.plan_info(nq))
            form = MA.form_of(n, nq, 1, False, env, finite)
            assert form != MA.TWOPASS
            exp = want if want is not None else MA.expected_of(c, form)
            got = idx.scores(Q)
            assert MA.same_scores(got, exp), (form, env, np.argwhere(got.view(np.uint32) != exp.view(np.uint32))[:5].tolist())
            out[(pi, di)] = got
            idx.reserve(nq, max(ks.values()))
            for kind, k in ks.items():
                form = MA.form_of(n, nq, k, True, env, finite)
                two = nat.maxsim_workspace_plan(n, finite, nq, k, nq, k)[1] > MA.rows_bytes(n, nq)
                assert two == (form == MA.TWOPASS), (kind, k, env)
                exp = want if want is not None else MA.expected_of(c, form)
                es, ei = MA.topk_expected(exp, k)
                _same(*idx.search(Q, k), es, ei, (form, "search", kind, k, env))
                _same(*_device(idx, Q, k), es, ei, (form, "search_device", kind, k, env))
            idx.close()
    _pin(mp)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_every_form_returns_the_one_right_answer(nat, monkeypatch, name):
    case = CASES[name]
    c = MA.case_view(case)
    _run(nat, monkeypatch, c, MA.case_depths(case, c), case["pins"])


# ---- the scoped form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slab", [None, "4"], ids=["default-slabs", "slab-4"])
@pytest.mark.parametrize("family,arg,n_docs,nq,q_len", MA.SCOPE_CASES)
def test_scoped_form(nat, monkeypatch, family, arg, n_docs, nq, q_len, slab):
    """ScopeWorkspace.maxsim_search and maxsim_search_device over scopes of every document, one document (first, inside,
    last) and a run: the ids and bits of the expected matrix ranked inside each query's scope."""
    c = MA.view(family, arg, n_docs, nq, q_len)
    _pin(monkeypatch, {"AMDR_SCOPE_SLAB": slab} if slab else {})
    n = len(c["doc_ptr"]) - 1
    scopes = MA.scopes_of(n)
    sp = np.concatenate([[0], np.cumsum([len(r) for r in scopes])]).astype(np.int64)
    rw = np.concatenate(scopes).astype(np.int64)
    rows_max = max(len(r) for r in scopes)
    idx, ws = nat.MaxSimIndex(c["D"], c["doc_ptr"]), nat.ScopeWorkspace()
    ks = sorted({1, MA.tie_k(c["exp_split"], n) or 2, n, min(n + 3, MA.MAX_K)})
    ws.reserve(nq, max(ks), rows_max)
    assert "scope_maxsim_kernel" in ws.plan_info(nq, max(ks), rows_max)
    q_d = torch.from_numpy(c["Q"]).to(DEV)
    sp_d, rw_d = torch.from_numpy(sp).to(DEV), torch.from_numpy(rw).to(DEV)
    for qs in (np.zeros(nq, np.int32), (np.arange(nq) % len(scopes)).astype(np.int32), ((np.arange(nq) + 3) % len(scopes)).astype(np.int32)):
        qs_d = torch.from_numpy(qs).to(DEV)
        for k in ks:
            es, ei = MA.topk_expected(c["exp_split"], k, rows=[scopes[s] for s in qs])
            _same(*ws.maxsim_search(idx, c["Q"], sp, rw, qs, k), es, ei, ("scoped", k, qs.tolist()))
            s = torch.full((nq, k), 123.0, dtype=torch.float32, device=DEV)
            i = torch.full((nq, k), 77, dtype=torch.int64, device=DEV)
            ws.maxsim_search_device(idx, q_d.data_ptr(), q_len, (sp_d.data_ptr(), rw_d.data_ptr(), qs_d.data_ptr(), len(scopes), rows_max),
                                    nq, k, s.data_ptr(), i.data_ptr(), 0)
            torch.cuda.synchronize()
            _same(s.cpu().numpy(), i.cpu().numpy(), es, ei, ("scoped device", k, qs.tolist()))
    ws.close()
    idx.close()
    _pin(monkeypatch)


# ---- non-finite stores --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MA.NONFINITE_KINDS)
def test_non_finite_store(nat, monkeypatch, kind):
    """A store holding a NaN or an infinity takes the fp32-input forms, PairF32 (7 queries) and Blocked (9): both return
    the bits of the written rule (MA.nonfinite_expected; never a NaN) from scores, search and search_device, the same
    for the seven queries they share; every other document keeps the bits it has in the store with the bad token zeroed."""
    got = {}
    for nq, form in ((7, MA.PAIRF32), (9, MA.BLOCKED)):
        c, bad, clean = MA.nonfinite_case(kind, nq)
        n = len(c["doc_ptr"]) - 1
        assert MA.form_of(n, nq, 1, False, {}, finite=False) == form == MA.form_of(n, nq, 2, True, {}, finite=False)
        want = MA.nonfinite_expected(c["D"], c["doc_ptr"], c["Q"])
        runs = _run(nat, monkeypatch, c, {"one": 1, "two": 2, "all": n, "over": n + 3}, ({},), finite=False, want=want)
        got[nq] = runs[(0, 0)]
        assert not np.isnan(got[nq]).any()
        others = np.arange(n) != bad
        ref = _run(nat, monkeypatch, dict(c, D=clean, exp_f32=MA.f32_expected(clean, c["doc_ptr"], c["Q"])), {"one": 1}, (MA.P_F32,))
        for r in runs.values():
            assert np.array_equal(r[:, others].view(np.uint32), ref[(0, 0)][:, others].view(np.uint32))
    assert np.array_equal(got[7].view(np.uint32), got[9][:7].view(np.uint32))

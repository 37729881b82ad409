"""Unions of posting lists resolved on the GPU (amdr_union_lists: csrc/union_lists.hip, csrc/union_rule.hpp) and read by the
term step as virtual posting lists: the device lists and the host twin's equal the reference of tests/union_cases.py exactly
— a Python set union over the documents' tokens — at the smallest shapes where the kernels can go wrong (a word, a tile and
four tiles of documents; 1, 2 and 65 items; an item of more terms than a block has threads); an array continued behind a
span step's lists; a union wherever a term id may stand in a constraint; the status word at the capacity; argument errors; a
handle without a token stream; the lists across updates; capture of the span, union and term steps in one chain."""
import numpy as np
import pytest
import torch

import phrase_cases as PC
import term_scope_cases as TC
import union_cases as UC
from legal_rag_amd._native import UNION_TILE as T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = -77
T_OPS = (torch.int64, torch.int32, torch.int64, torch.int32, torch.int64, torch.int64, torch.int32)


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


def make_index(nat, corpus, stream=False):
    tp, pd, pt, idf, dl, avgdl = corpus.postings()
    gi = nat.BM25Index(tp, pd, pt, idf, dl, avgdl)
    if stream:
        gi.set_tokens(*corpus.stream())
    return gi


@pytest.fixture(scope="module")
def rand(nat):
    """The "rand" corpus of phrase_cases (token sequences) and its index with the token stream resident."""
    corpus = PC.rand_corpus()
    return corpus, make_index(nat, corpus, stream=True)


def dev_arr(a, dtype):
    t = torch.zeros(max(int(np.size(a)), 1), dtype=dtype, device=DEV)
    if np.size(a):
        t[:np.size(a)].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def run_device(nat, gi, items, rows_cap, before=None):
    """amdr_union_lists_device on fresh tensors: (list_ptr, docs [rows_cap], status) as numpy arrays; what the call does not
    write keeps SENTINEL.  before = (list_ptr, docs): the array the call continues."""
    n, k = len(items), 0 if before is None else before[0].size - 1
    ip, it = (dev_arr(a, dt) for a, dt in zip(UC.operands(items), (torch.int64, torch.int32)))
    lp = torch.full((k + n + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    dc = torch.full((max(rows_cap, 1),), SENTINEL, dtype=torch.int32, device=DEV)
    if before is not None:
        lp[:k + 1].copy_(torch.from_numpy(before[0]))
        dc[:before[1].size].copy_(torch.from_numpy(before[1]))
    st = torch.full((max(n, 1),), SENTINEL, dtype=torch.int32, device=DEV)
    wb = nat.union_lists_plan(n, gi.n_docs)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=DEV)
    gi.union_lists_device(ip.data_ptr(), it.data_ptr(), n, k, rows_cap, lp.data_ptr(), dc.data_ptr(), st.data_ptr(),
                          work.data_ptr(), wb, stream_ptr())
    torch.cuda.synchronize()
    return lp.cpu().numpy(), dc.cpu().numpy()[:rows_cap], st.cpu().numpy()[:n]


def run_twin(gi, items, rows_cap):
    return gi.union_lists(*UC.operands(items), rows_cap)


def assert_lists(got, want_ptr, want_docs, device_cap=None):
    lp, docs, status = got
    assert lp.dtype == np.int64 and np.array_equal(lp, want_ptr), (lp, want_ptr)
    assert docs.dtype == np.int32 and np.array_equal(docs[:want_ptr[-1]].view(np.uint8), want_docs.view(np.uint8))
    assert status.dtype == np.int32 and not status.any(), status
    if device_cap is not None:  # nothing is written past the lists
        assert np.all(docs[want_ptr[-1]:] == SENTINEL)


def check_both(nat, corpus, gi, items):
    want_ptr, want_docs = UC.expected_lists(corpus, items)
    cap = UC.rows_cap(corpus, items)
    assert cap >= want_ptr[-1]
    assert_lists(run_device(nat, gi, items, cap), want_ptr, want_docs, cap)
    assert_lists(run_twin(gi, items, cap), want_ptr, want_docs)
    assert_lists(run_device(nat, gi, items, int(want_ptr[-1])), want_ptr, want_docs)  # a capacity of exactly the lists
    return want_ptr, want_docs


# ---- the lists ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", UC.edge_sizes(T))
def test_edge_sizes_items_and_1_2_65_items_per_call(nat, n):
    corpus = UC.edge_corpus(n, T)
    gi = make_index(nat, corpus)
    assert gi.tokens_info() == (False, 0)  # the postings alone
    items = UC.batch(corpus, 65)
    want_ptr, want_docs = check_both(nat, corpus, gi, items)
    named = UC.edge_items(corpus)
    at = {name: i for i, name in enumerate(named)}
    every = want_docs[want_ptr[at["every document"]]:want_ptr[at["every document"] + 1]]
    assert every.size == n and every[0] == 0 and every[-1] == n - 1
    assert np.all(np.diff(want_ptr)[[at[x] for x in ("no term", "unknown -1", "unknown n_terms", "unknown ids")]] == 0)
    for name in ("300 terms", "overlapping", "marks and straddle"):  # alone: another grid, the same list
        check_both(nat, corpus, gi, [named[name]])
    check_both(nat, corpus, gi, [named["overlapping"], named["300 terms"]])
    lp0, docs0, st0 = gi.union_lists(np.zeros(1, np.int64), np.zeros(0, np.int32), 0)  # no item: an empty array
    assert lp0.tolist() == [0] and docs0.size == 0 and st0.size == 0


# ---- one list array ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 3])
def test_the_union_step_continues_the_array_a_span_step_began(nat, rand, k):
    import near_cases as NC
    corpus, gi = rand
    spans = NC.scope_items(corpus)[:k]
    unions = UC.chain_unions(corpus) + [[]]
    n = len(unions)
    s_max, s_cap = NC.bounds(corpus, spans) if k else (0, 0)
    cap = s_cap + UC.rows_cap(corpus, unions)
    ops = [dev_arr(a, dt) for a, dt in zip(NC.operands(spans), (torch.int64, torch.int32, torch.int32, torch.int32))]
    ip, it = (dev_arr(a, dt) for a, dt in zip(UC.operands(unions), (torch.int64, torch.int32)))
    lp = torch.full((k + n + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    dc = torch.full((cap,), SENTINEL, dtype=torch.int32, device=DEV)
    st = torch.full((k + n,), SENTINEL, dtype=torch.int32, device=DEV)
    swb, uwb = nat.span_lists_plan(k, s_max), nat.union_lists_plan(n, gi.n_docs)
    swork = torch.empty(max(swb, 1), dtype=torch.uint8, device=DEV)
    uwork = torch.empty(uwb, dtype=torch.uint8, device=DEV)
    s = stream_ptr()
    if k:  # (k = 0: the union step starts the array itself)
        gi.span_lists_device(*[x.data_ptr() for x in ops], k, s_max, s_cap, lp.data_ptr(), dc.data_ptr(), st.data_ptr(),
                             swork.data_ptr(), swb, s)
        torch.cuda.synchronize()
        span_ptr, span_docs = lp.cpu().numpy()[:k + 1].copy(), dc.cpu().numpy().copy()
        assert np.array_equal(span_ptr, NC.expected_lists(corpus, spans)[0])
        gi.span_lists_device(*[x.data_ptr() for x in ops], k, s_max, s_cap, lp.data_ptr(), dc.data_ptr(), st.data_ptr(),
                             swork.data_ptr(), swb, s)  # again, with the union step behind it and no synchronise between
    gi.union_lists_device(ip.data_ptr(), it.data_ptr(), n, k, cap, lp.data_ptr(), dc.data_ptr(), st.data_ptr() + 4 * k,
                          uwork.data_ptr(), uwb, s)
    torch.cuda.synchronize()
    before = NC.expected_lists(corpus, spans) if k else (np.zeros(1, np.int64), np.zeros(0, np.int32))
    want_ptr, want_docs = UC.expected_lists(corpus, unions, before=before)
    got_ptr, got_docs = lp.cpu().numpy(), dc.cpu().numpy()
    assert np.array_equal(got_ptr, want_ptr) and np.array_equal(got_docs[:want_ptr[-1]], want_docs)
    assert np.all(got_docs[want_ptr[-1]:] == SENTINEL) and not st.cpu().numpy().any()
    if k:  # the span part's bytes are untouched
        used = int(span_ptr[-1])
        assert np.array_equal(got_ptr[:k + 1], span_ptr) and np.array_equal(got_docs[:used].view(np.uint8), span_docs[:used].view(np.uint8))
    # ... and the same from given arrays: the call reads list_ptr[n_before] on the device
    given = (before[0], before[1])
    assert_lists(run_device(nat, gi, unions, cap, before=given), want_ptr, want_docs, cap)


# ---- through the term step ---------------------------------------------------------------------------------------------------
def test_a_union_stands_wherever_a_term_id_may_and_upper_bounds_never_overflow(nat, rand):
    """MUST and driver, MUST beside a rarer plain term, ANY, NOT, inside a tuple group next to a phrase, two unions as MUST,
    an id past the lists, and inside a base scope — against set algebra over the documents' tokens."""
    from legal_rag_amd.retrieval.engine import HybridEngine
    from legal_rag_amd.retrieval.terms import OneOf, Phrase, TermTable, driver_length
    corpus, gi = rand
    phrases, unions = UC.scope_lists(corpus)
    fam = UC.scope_family(corpus)
    UC.scope_certificates(corpus, fam, phrases, unions)
    ops = TC.operands(fam)
    want_ptr, want_rows = UC.expected_table(corpus, fam, phrases, unions)
    ub = UC.list_bounds(corpus, phrases, unions)
    lens = [driver_length(g, ub, None if b < 0 else int(fam.bases[b].size), corpus.n_docs) for g, b in fam.cons]
    cand_max, rows_cap = max(lens), sum(lens)
    p_lens = [PC.driver_len(corpus, p) for p in phrases]
    # the host twins, the arrays joined in numpy
    plp, pdocs, p_status = gi.phrase_lists(*PC.operands(phrases), max(p_lens), sum(p_lens))
    ulp, udocs, u_status = run_twin(gi, unions, UC.rows_cap(corpus, unions))
    assert not p_status.any() and not u_status.any()
    assert all(ulp[i + 1] - ulp[i] <= UC.upper_bound(corpus, u) for i, u in enumerate(unions))
    lists = (np.concatenate([plp, plp[-1] + ulp[1:]]), np.concatenate([pdocs, udocs]))
    sp, rows, status = gi.term_scope(ops, cand_max, rows_cap, lists=lists)
    assert not status.any() and np.array_equal(sp, want_ptr) and np.array_equal(rows, want_rows)
    # the same through the engine: the phrase step, the union step behind it and the term step on one stream
    qscope = np.arange(len(fam.cons), dtype=np.int32)
    tt = TermTable(ops, qscope, len(fam.cons), int(ops[1].size), len(fam.bases), np.asarray(lens, np.int64), cand_max, rows_cap,
                   PC.operands(phrases), tuple(Phrase(*[f"t{t}" for t in p]) for p in phrases), max(p_lens), sum(p_lens))
    tt.union_ops, tt.union_rows_cap = UC.operands(unions), UC.rows_cap(corpus, unions)
    tt.unions = tuple(OneOf(*[f"t{t}" for t in u]) for u in unions)
    eng = HybridEngine(None, gi, None)
    table, st = eng.term_scopes(tt)
    torch.cuda.synchronize()
    assert st.dtype == torch.int32 and st.numel() == len(fam.cons) + len(phrases) + len(unions) and not st.cpu().numpy().any()
    assert np.array_equal(table[0].cpu().numpy(), want_ptr) and np.array_equal(table[1].cpu().numpy()[:want_ptr[-1]], want_rows)
    # unions alone (n_before = 0): the union step starts the list array
    alone = TC.Family("unions alone", "rand", [TC.c([(TC.MUST, [corpus.n_terms + j])]) for j in range(len(unions))])
    ops1 = TC.operands(alone)
    lens1 = [UC.upper_bound(corpus, u) for u in unions]
    t1 = TermTable(ops1, np.arange(len(unions), dtype=np.int32), len(unions), int(ops1[1].size), 0, np.asarray(lens1, np.int64),
                   max(lens1), sum(lens1))
    t1.union_ops, t1.union_rows_cap, t1.unions = tt.union_ops, tt.union_rows_cap, tt.unions
    table1, st1 = eng.term_scopes(t1)
    torch.cuda.synchronize()
    u_ptr, u_docs = UC.expected_lists(corpus, unions)
    assert st1.numel() == 2 * len(unions) and not st1.cpu().numpy().any()
    assert np.array_equal(table1[0].cpu().numpy(), u_ptr) and np.array_equal(table1[1].cpu().numpy()[:u_ptr[-1]], u_docs)
    # an overflow of the union step's bound lands behind the constraints' and the phrases' words, at the union's place
    tt.phr_rows_cap, tt.union_rows_cap = int(plp[-1]), int(ulp[-1]) - 1  # (the array's capacity: both parts exact, less one)
    _, st2 = eng.term_scopes(tt)
    torch.cuda.synchronize()
    assert st2.cpu().numpy()[len(fam.cons) + len(phrases):].tolist() == [0, 0, 0, 2]


# ---- the status word -----------------------------------------------------------------------------------------------------------
def test_rows_cap_one_below_the_total_sets_status_2_from_the_first_item_that_does_not_fit(nat):
    corpus = UC.edge_corpus(T + 1, T)
    gi = make_index(nat, corpus)
    named = UC.edge_items(corpus)
    items = [named[x] for x in ("one term", "overlapping", "no term", "300 terms", "straddle", "empty list", "marks and straddle")]
    want_ptr, want_docs = UC.expected_lists(corpus, items)
    total = int(want_ptr[-1])
    for cap in (total - 1, int(want_ptr[4]) - 1, 0):  # the last item loses a document; cut inside the fourth; no room at all
        first = int(np.searchsorted(want_ptr[1:], cap, side="right"))
        for lp, docs, status in (run_device(nat, gi, items, cap), run_twin(gi, items, cap)):
            assert status.tolist() == [2 if p >= first and want_ptr[p + 1] > want_ptr[p] else 0 for p in range(len(items))]
            assert np.array_equal(lp, np.minimum(want_ptr, cap)) and np.array_equal(docs[:cap], want_docs[:cap])
    # behind earlier lists the capacity is the whole array's
    before = (np.asarray([0, 2, 5], np.int64), np.asarray([4, 9, 1, 2, 3], np.int32))
    lp, docs, status = run_device(nat, gi, items, 5 + total - 1, before=before)
    assert lp.tolist() == np.concatenate([before[0], np.minimum(5 + want_ptr[1:], 5 + total - 1)]).tolist()
    assert status.tolist() == [0] * (len(items) - 1) + [2] and docs[:5].tolist() == before[1].tolist()
    assert np.array_equal(docs[5:], want_docs[:total - 1])


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing_and_leave_the_outputs_untouched(nat):
    corpus = UC.edge_corpus(T + 1, T)
    gi = make_index(nat, corpus)
    items = UC.batch(corpus, 20)
    n, cap = len(items), UC.rows_cap(corpus, items)
    ip, it = (dev_arr(a, dt) for a, dt in zip(UC.operands(items), (torch.int64, torch.int32)))
    lp = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    dc = torch.full((cap,), SENTINEL, dtype=torch.int32, device=DEV)
    st = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    wb = nat.union_lists_plan(n, gi.n_docs)
    assert wb == nat.union_lists_plan(n, T + 1) > 2 * n * T // 8  # two tiles per item
    work = torch.empty(wb, dtype=torch.uint8, device=DEV)
    good = dict(ip=ip.data_ptr(), it=it.data_ptr(), n=n, before=0, cap=cap, lp=lp.data_ptr(), dc=dc.data_ptr(), st=st.data_ptr(),
                work=work.data_ptr(), wb=wb)

    def call(**over):
        a = dict(good, **over)
        gi.union_lists_device(a["ip"], a["it"], a["n"], a["before"], a["cap"], a["lp"], a["dc"], a["st"], a["work"], a["wb"],
                              stream_ptr())
    for over in (dict(n=-1), dict(before=-1), dict(cap=-1), dict(wb=-1), dict(wb=wb - 1), dict(work=0), dict(lp=0), dict(dc=0),
                 dict(st=0), dict(ip=0), dict(it=0), dict(n=2**30), dict(n=2**31)):  # (2^30 items x 2 tiles = 2^31 cells)
        with pytest.raises(nat.NativeError):
            call(**over)
    torch.cuda.synchronize()
    assert (lp == SENTINEL).all() and (dc == SENTINEL).all() and (st == SENTINEL).all()
    call()  # the same buffers with the arguments as they should be
    torch.cuda.synchronize()
    want_ptr, want_docs = UC.expected_lists(corpus, items)
    assert np.array_equal(lp.cpu().numpy(), want_ptr) and np.array_equal(dc.cpu().numpy()[:want_ptr[-1]], want_docs)
    z = np.zeros(19, np.int32)
    for bad_ptr in ([1, 2, 4], [0, 4, 2]):  # the twin validates the pointer array
        with pytest.raises(nat.NativeError, match="item_ptr"):
            gi.union_lists(np.asarray(bad_ptr, np.int64), z, cap)
    with pytest.raises(nat.NativeError):
        gi.union_lists(np.asarray([0, 2], np.int64), z, -1)


# ---- updates -----------------------------------------------------------------------------------------------------------------
def test_after_add_remove_and_replace_the_lists_are_those_of_the_edited_corpus(nat):
    corpus = PC.SeqCorpus("small", 4, [[0, 1, 2], [1, 3, 0], [], [2, 2, 0, 3, 1], [3, 0, 1], [1]])
    V = corpus.n_terms
    idf = np.linspace(0.5, 3.0, V)
    one = PC.SeqCorpus("one", V, [[2, 2, 3]])
    a_ptr, a_doc, a_tf, _, a_len, _ = one.postings()
    items = [[2, 3], [0], [3, -1, 2, 2], [], [0, 1, 2, 3]]

    def same(gi, after):
        assert gi.tokens_info() == (False, 0)  # no stream was ever set, and none is needed
        want_ptr, want_docs = UC.expected_lists(after, items)
        cap = UC.rows_cap(after, items)
        assert_lists(run_twin(gi, items, cap), want_ptr, want_docs)
        assert_lists(run_device(nat, gi, items, cap), want_ptr, want_docs, cap)
    gi = make_index(nat, corpus)
    same(gi, corpus)
    assert UC.item_list(corpus, items[0]).tolist() == [0, 1, 3, 4]
    gi.add(a_ptr, a_doc, a_tf, idf, a_len, 2.0)
    added = PC.SeqCorpus("added", V, corpus.docs + one.docs)
    assert UC.item_list(added, items[0]).tolist() == [0, 1, 3, 4, 6]
    same(gi, added)
    gi = make_index(nat, corpus)
    gi.remove(np.asarray([3], np.int64), idf, 2.0)
    same(gi, PC.SeqCorpus("removed", V, corpus.docs[:3] + corpus.docs[4:]))
    gi = make_index(nat, corpus)
    gi.replace(np.asarray([5], np.int64), a_ptr, a_doc, a_tf, a_len, idf, 2.0)
    after = PC.SeqCorpus("replaced", V, corpus.docs[:5] + one.docs)
    assert UC.item_list(after, items[0]).tolist() == [0, 1, 3, 4, 5]
    same(gi, after)


# ---- capture -----------------------------------------------------------------------------------------------------------------
def test_captured_span_union_and_term_steps_replay_with_the_items_rewritten_in_place(nat, rand):
    """One linear chain on one stream: the span step's three launches, the union step's three, then the term step's."""
    import near_cases as NC
    corpus, gi = rand
    V, k, n, M = corpus.n_terms, 2, 4, 3  # two phrases of two tokens in front, four unions of three ids behind
    n_x = k + n
    cand_max, rows_cap = corpus.n_docs, n_x * corpus.n_docs  # hold for every item over this corpus
    fam = TC.Family("each list alone", "rand", [TC.c([(TC.MUST, [V + p])]) for p in range(n_x)])
    t = [dev_arr(a, dt) for a, dt in zip(TC.operands(fam), T_OPS)]
    sp_ptr = dev_arr(np.arange(0, 2 * k + 1, 2), torch.int64)
    sp_terms = torch.zeros(2 * k, dtype=torch.int32, device=DEV)
    sp_kind, sp_dist = torch.zeros(k, dtype=torch.int32, device=DEV), torch.zeros(k, dtype=torch.int32, device=DEV)
    ip = dev_arr(np.arange(0, n * M + 1, M), torch.int64)
    it_ = torch.zeros(n * M, dtype=torch.int32, device=DEV)
    lp = torch.zeros(n_x + 1, dtype=torch.int64, device=DEV)
    dc = torch.zeros(rows_cap, dtype=torch.int32, device=DEV)
    pst = torch.zeros(n_x, dtype=torch.int32, device=DEV)
    sp = torch.zeros(n_x + 1, dtype=torch.int64, device=DEV)
    rw = torch.zeros(rows_cap, dtype=torch.int64, device=DEV)
    st = torch.zeros(n_x, dtype=torch.int32, device=DEV)
    swb, uwb, wb = nat.span_lists_plan(k, cand_max), nat.union_lists_plan(n, gi.n_docs), nat.term_scope_plan(n_x, cand_max)
    swork, uwork, work = (torch.empty(b, dtype=torch.uint8, device=DEV) for b in (swb, uwb, wb))

    def variant(seed):
        r = np.random.default_rng(seed)
        phrases = []
        while len(phrases) < k:
            seq = corpus.docs[int(r.integers(0, corpus.n_docs))]
            if len(seq) >= 2:
                s = int(r.integers(0, len(seq) - 1))
                phrases.append([int(seq[s]), int(seq[s + 1])])
        unions = [[int(x) for x in r.integers(-1, V + 1, size=M)] for _ in range(n)]
        return phrases, unions

    def step():
        s = stream_ptr()
        gi.span_lists_device(sp_ptr.data_ptr(), sp_terms.data_ptr(), sp_kind.data_ptr(), sp_dist.data_ptr(), k, cand_max,
                             rows_cap, lp.data_ptr(), dc.data_ptr(), pst.data_ptr(), swork.data_ptr(), swb, s)
        gi.union_lists_device(ip.data_ptr(), it_.data_ptr(), n, k, rows_cap, lp.data_ptr(), dc.data_ptr(),
                              pst.data_ptr() + 4 * k, uwork.data_ptr(), uwb, s)
        gi.term_scope_device([x.data_ptr() for x in t], 0, n_x, n_x, cand_max, rows_cap, sp.data_ptr(), rw.data_ptr(),
                             st.data_ptr(), work.data_ptr(), wb, s, lists=(lp.data_ptr(), dc.data_ptr(), n_x))

    def write(phrases, unions):
        sp_terms.copy_(torch.from_numpy(PC.operands(phrases)[1]))
        it_.copy_(torch.from_numpy(UC.operands(unions)[1]))

    def snapshot():
        torch.cuda.synchronize()
        return [x.cpu().numpy().copy() for x in (lp, dc, pst, sp, rw, st)]
    write(*variant(1))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):  # an eager run first, outside the capture
        step()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    g0 = nat.workspace_growths()
    for seed in (2, 3):
        phrases, unions = variant(seed)
        write(phrases, unions)
        graph.replay()
        got = snapshot()
        assert nat.workspace_growths() == g0
        want_ptr, want_docs = UC.expected_lists(corpus, unions, before=PC.expected_lists(corpus, phrases))
        assert want_ptr[k] > 0 and want_ptr[-1] > want_ptr[k]
        assert np.array_equal(got[0], want_ptr) and np.array_equal(got[1][:want_ptr[-1]], want_docs) and not got[2].any()
        assert np.array_equal(got[3], want_ptr) and np.array_equal(got[4][:want_ptr[-1]], want_docs) and not got[5].any()

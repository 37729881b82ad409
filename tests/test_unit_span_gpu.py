"""Unit spans resolved on the GPU (amdr_unit_spans: csrc/unit_span.hip, csrc/unit_span_rule.hpp) and the break flags they
read (amdr_bm25_set_breaks): the device lists and the host twin's equal the brute-force evaluator of
tests/unit_span_cases.py — lists, list_ptr and status words — on the generated corpus (documents of 1 .. 200 tokens, units
at lane 0, 63 and 64, over a round boundary and over three rounds, 64 units in one round, classes of 2 and 300 ids, drivers
of 255, 256 and 257 candidates); behind earlier lists and the empty call; both status words; the refusals of set_breaks;
the flags dropped by set_tokens and by a plain and a carrying add; read-back; one capture replayed twice."""
import numpy as np
import pytest
import torch

import unit_span_cases as UC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = -77
I_OPS = (torch.int64, torch.int32, torch.int32)
EMPTY = (np.zeros(1, np.int64), np.zeros(0, np.int32))


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


def make_index(nat, corpus, stream=True, breaks=True):
    tp, pd, pt, idf, dl, avgdl = corpus.postings()
    gi = nat.BM25Index(tp, pd, pt, idf, dl, avgdl)
    if stream:
        gi.set_tokens(*corpus.stream())
        if breaks:
            gi.set_breaks(corpus.flags())
    return gi


@pytest.fixture(scope="module")
def cases(nat):
    corpus, at = UC.make_corpus()
    assert corpus.n_docs <= 4000
    return corpus, make_index(nat, corpus), UC.batch(corpus, UC.N_ITEMS)


def dev_arr(a, dtype):
    t = torch.zeros(max(int(np.size(a)), 1), dtype=dtype, device=DEV)
    if np.size(a):
        t[:np.size(a)].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def run_device(nat, gi, corpus, items, cand_max, rows_cap, before=EMPTY):
    """The union step for the items' classes and amdr_unit_spans_device behind it, on fresh tensors, continuing the array
    `before` = (list_ptr, docs): (list_ptr, docs [capacity], the items' status) as numpy arrays; what no call writes keeps
    SENTINEL.  rows_cap: the room of the ITEMS' documents; the classes' lists get exactly theirs."""
    k, n = before[0].size - 1, len(items)
    ops, (c_ptr, c_terms) = UC.operands(items, corpus.n_terms, cls_first=k)
    n_cls = c_ptr.size - 1
    cls_want = UC.class_lists(corpus, items, before=before)
    cap = int(cls_want[0][-1]) + rows_cap
    o = [dev_arr(a, dt) for a, dt in zip(ops, I_OPS)]
    cp, ct = dev_arr(c_ptr, torch.int64), dev_arr(c_terms, torch.int32)
    lp = torch.full((k + n_cls + n + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    dc = torch.full((max(cap, 1),), SENTINEL, dtype=torch.int32, device=DEV)
    lp[:k + 1].copy_(torch.from_numpy(before[0]))
    if before[1].size:
        dc[:before[1].size].copy_(torch.from_numpy(before[1]))
    st = torch.full((max(n_cls + n, 1),), SENTINEL, dtype=torch.int32, device=DEV)
    uwb, wwb = nat.union_lists_plan(n_cls, gi.n_docs), nat.unit_spans_plan(n, cand_max)
    uwork = torch.empty(max(uwb, 1), dtype=torch.uint8, device=DEV)
    wwork = torch.empty(max(wwb, 1), dtype=torch.uint8, device=DEV)
    s = stream_ptr()
    gi.union_lists_device(cp.data_ptr(), ct.data_ptr(), n_cls, k, cap, lp.data_ptr(), dc.data_ptr(), st.data_ptr(),
                          uwork.data_ptr(), uwb, s)
    gi.unit_spans_device(*[x.data_ptr() for x in o], n, cp.data_ptr(), ct.data_ptr(), n_cls, k, k + n_cls, cand_max, cap,
                         lp.data_ptr(), dc.data_ptr(), st.data_ptr() + 4 * n_cls, wwork.data_ptr(), wwb, s)
    torch.cuda.synchronize()
    got_lp, got_dc, got_st = lp.cpu().numpy(), dc.cpu().numpy()[:cap], st.cpu().numpy()
    assert np.array_equal(got_lp[:k + n_cls + 1], cls_want[0]) and not got_st[:n_cls].any()       # the classes' lists, as the
    assert np.array_equal(got_dc[:cls_want[0][-1]].view(np.uint8), cls_want[1].view(np.uint8))    # union step left them
    return got_lp, got_dc, got_st[n_cls:n_cls + n]


def run_twin(gi, corpus, items, cand_max, rows_cap):
    ops, classes = UC.operands(items, corpus.n_terms)
    return gi.unit_spans(*ops, *classes, cand_max, rows_cap)


def check_both(nat, corpus, gi, items, before=EMPTY):
    cand_max, rows_cap = UC.bounds(corpus, items)
    cls_ptr, cls_docs = UC.class_lists(corpus, items, before=before)
    want_ptr, want_docs = UC.expected_lists(corpus, items, before=(cls_ptr, cls_docs))
    total = int(want_ptr[-1] - cls_ptr[-1])
    assert rows_cap >= total
    for cap in (rows_cap, total):  # the bound a caller knows; a capacity of exactly the lists
        lp, docs, status = run_device(nat, gi, corpus, items, cand_max, cap, before=before)
        assert lp.dtype == np.int64 and np.array_equal(lp, want_ptr), (lp, want_ptr)
        assert docs.dtype == np.int32 and np.array_equal(docs[:want_ptr[-1]].view(np.uint8), want_docs.view(np.uint8))
        assert status.dtype == np.int32 and not status.any(), status
        assert np.all(docs[want_ptr[-1]:] == SENTINEL)  # nothing is written past the lists
    t_ptr, t_docs = UC.expected_lists(corpus, items)
    lp, docs, status = run_twin(gi, corpus, items, cand_max, rows_cap)
    assert lp.dtype == np.int64 and np.array_equal(lp, t_ptr) and not status.any()
    assert docs.dtype == np.int32 and np.array_equal(docs.view(np.uint8), t_docs.view(np.uint8))
    return want_ptr, want_docs


# ---- the lists ---------------------------------------------------------------------------------------------------------------
def test_device_and_twin_equal_the_evaluator_on_the_generated_corpus(nat, cases):
    corpus, gi, items = cases
    want_ptr, _ = check_both(nat, corpus, gi, items)
    named = UC.named_items()
    idx = {name: i for i, name in enumerate(named)}
    sizes = np.diff(want_ptr)[len(UC.classes_of(items)):]
    assert all(sizes[idx[x]] > 0 for x in ("a b /s", "a b +p", "g g /s", "pair b /s", "all k b /s", "r255 /s", "r256 /s", "r257 +s"))
    assert not sizes[[idx[x] for x in ("unknown -1", "unknown past the classes", "nowhere")]].any()
    assert UC.bounds(corpus, items)[0] > UC.TILE  # more than one tile of candidates
    for name in ("a b /s", "g g /p", "all k b +p", "unknown -1", "r257 +s"):  # alone: another grid, the same list
        check_both(nat, corpus, gi, [named[name]])
    check_both(nat, corpus, gi, [named["r256 /s"], named["b a +s"]])


def test_behind_earlier_lists_and_the_empty_call(nat, cases):
    corpus, gi, items = cases
    first = [np.arange(0, corpus.n_docs, 3, dtype=np.int32), np.zeros(0, np.int32), np.arange(5, 40, dtype=np.int32)]
    before = UC._array(first)
    assert before[0].size - 1 == 3 and before[0][-1] > 0
    want_ptr, want_docs = check_both(nat, corpus, gi, items[:9] + items[-3:], before=before)
    assert np.array_equal(want_ptr[:4], before[0]) and np.array_equal(want_docs[:before[1].size], before[1])
    # no item: behind n_before lists the array stays as it is; alone, an empty array begins
    lp, docs, status = run_device(nat, gi, corpus, [], 0, 0, before=before)
    assert np.array_equal(lp, before[0]) and np.array_equal(docs, before[1]) and status.size == 0
    lp, docs, status = run_device(nat, gi, corpus, [], 0, 0)
    assert lp.tolist() == [0]
    lp0, docs0, st0 = gi.unit_spans(*UC.operands([], corpus.n_terms)[0], *EMPTY, 0, 0)
    assert lp0.tolist() == [0] and docs0.size == 0 and st0.size == 0


def test_cand_max_below_a_driver_gives_1_and_rows_cap_below_the_total_gives_2(nat, cases):
    corpus, gi, _ = cases
    named = UC.named_items()
    items = [named[x] for x in ("r255 /s", "r256 /s", "r257 +s", "a b /s", "pair b /s")]
    cand_max, rows_cap = UC.bounds(corpus, items)
    assert cand_max == 257
    t_ptr, t_docs = UC.expected_lists(corpus, items)
    n_cls = len(UC.classes_of(items))
    for cut in (256, 255):
        over = [UC.driver_len(corpus, it) > cut for it in items]
        assert any(over) and not all(over)
        kept = [UC.item_list(corpus, it) if not o else np.zeros(0, np.int32) for it, o in zip(items, over)]
        for lp, docs, status in (run_device(nat, gi, corpus, items, cut, rows_cap), run_twin(gi, corpus, items, cut, rows_cap)):
            assert status.tolist() == [1 if o else 0 for o in over]
            assert np.diff(lp)[-len(items):].tolist() == [x.size for x in kept]
            assert np.array_equal(docs[lp[-len(items) - 1]:lp[-1]], np.concatenate(kept))
    total = int(t_ptr[-1])
    for cap in (total - 1, int(t_ptr[2]) - 1, 0):
        first = int(np.searchsorted(t_ptr[1:], cap, side="right"))
        flags = [2 if p >= first and t_ptr[p + 1] > t_ptr[p] else 0 for p in range(len(items))]
        lp, docs, status = run_device(nat, gi, corpus, items, cand_max, cap)
        base = int(lp[n_cls])
        assert status.tolist() == flags and np.array_equal(lp[n_cls:], base + np.minimum(t_ptr, cap))
        assert np.array_equal(docs[base:base + cap], t_docs[:cap])
        lp, docs, status = run_twin(gi, corpus, items, cand_max, cap)
        assert status.tolist() == flags and np.array_equal(lp, np.minimum(t_ptr, cap)) and np.array_equal(docs, t_docs[:cap])


# ---- the flags ---------------------------------------------------------------------------------------------------------------
def small():
    docs = [[0, 1, 2], [1, 3, 0], [], [2, 2, 0, 3, 1], [3, 0, 1], [1]]
    brk = [[0, 0, 1], [3, 1, 0], [], [0, 1, 0, 3, 0], [0, 0, 0], [1]]
    return UC.UnitCorpus("small", 4, docs, brk)


def device_call(nat, gi, corpus, items):
    cand_max, rows_cap = UC.bounds(corpus, items)
    return run_device(nat, gi, corpus, items, cand_max, rows_cap)


def test_set_breaks_refusals_read_back_and_info(nat):
    corpus = small()
    gi = make_index(nat, corpus, breaks=False)
    n = int(corpus.stream()[0][-1])
    assert gi.breaks_info() == (False, 0)
    with pytest.raises(nat.NativeError, match="no break flags"):
        gi.read_breaks()
    for bad in (np.zeros(n - 1, np.uint8), np.zeros(n + 1, np.uint8), np.zeros(0, np.uint8)):  # a wrong count
        with pytest.raises(nat.NativeError, match=f"stream of {n} tokens"):
            gi.set_breaks(bad)
    two = corpus.flags().copy()
    two[4] = 2                                                                            # a paragraph start that is no sentence start
    for bad in (two, np.where(np.arange(n) == n - 1, 4, 0).astype(np.uint8), np.full(n, 255, np.uint8)):
        with pytest.raises(nat.NativeError, match="flag"):
            gi.set_breaks(bad)
    assert gi.breaks_info() == (False, 0)                                                  # a refusal leaves the handle as it was
    gi.set_breaks(corpus.flags())
    assert gi.breaks_info() == (True, n) and np.array_equal(gi.read_breaks(), corpus.flags()) and gi.read_breaks().dtype == np.uint8
    with pytest.raises(nat.NativeError, match="flag"):
        gi.set_breaks(two)
    assert np.array_equal(gi.read_breaks(), corpus.flags())                                # ... also the flags it had
    other = np.where(corpus.flags() == 1, 3, corpus.flags()).astype(np.uint8)
    gi.set_breaks(other)
    assert np.array_equal(gi.read_breaks(), other)
    bare = make_index(nat, corpus, stream=False)                                           # no resident stream
    with pytest.raises(nat.NativeError, match="no token stream"):
        bare.set_breaks(corpus.flags())
    assert bare.breaks_info() == (False, 0)


def test_the_flags_go_with_set_tokens_and_with_a_plain_and_a_carrying_add_and_the_device_call_refuses(nat):
    corpus = small()
    V = corpus.n_terms
    idf = np.linspace(0.5, 3.0, V)
    one = UC.UnitCorpus("one", V, [[2, 0, 3]], [[0, 1, 0]])
    a_ptr, a_doc, a_tf, _, a_len, _ = one.postings()
    items = [(0, [0, 1]), (2, [(0, 1), 3]), (1, [2, (0, 1)]), (3, [3, 0])]

    def gone(gi, after, stream_kept):
        assert gi.breaks_info() == (False, 0) and gi.tokens_info()[0] == stream_kept
        with pytest.raises(nat.NativeError, match="no break flags" if stream_kept else "no token stream"):
            device_call(nat, gi, after, items)
        with pytest.raises(nat.NativeError):
            run_twin(gi, after, items, *UC.bounds(after, items))
        with pytest.raises(nat.NativeError):
            gi.read_breaks()
        if not stream_kept:
            gi.set_tokens(*after.stream())
        gi.set_breaks(after.flags())
        check_both(nat, after, gi, items)
    gi = make_index(nat, corpus)
    check_both(nat, corpus, gi, items)
    assert UC.item_list(corpus, items[0]).tolist() == [0, 4] and UC.item_list(corpus, (2, [0, 1])).tolist() == [0, 1, 4]
    gi.set_tokens(*corpus.stream())                       # the same stream again: the flags described the one before
    gone(gi, corpus, True)
    added = UC.UnitCorpus("added", V, corpus.docs + one.docs, corpus.breaks + one.breaks)
    gi.add(a_ptr, a_doc, a_tf, idf, a_len, 2.0)            # a plain add drops the stream, and the flags with it
    gone(gi, added, False)
    gi = make_index(nat, corpus)
    gi.add(a_ptr, a_doc, a_tf, idf, a_len, 2.0, tokens=one.stream())  # a carrying add keeps the stream, not the flags
    assert np.array_equal(gi.read_tokens()[1], added.stream()[1])
    gone(gi, added, True)
    gi = make_index(nat, corpus)
    gi.remove(np.asarray([3], np.int64), idf, 2.0)
    gone(gi, UC.UnitCorpus("removed", V, corpus.docs[:3] + corpus.docs[4:], corpus.breaks[:3] + corpus.breaks[4:]), False)


# ---- capture -----------------------------------------------------------------------------------------------------------------
def test_the_device_call_is_captured_once_and_replayed_twice_with_equal_results(nat, cases):
    """Twice: a step that relied on a buffer cleared before the capture would pass one replay and fail the next."""
    corpus, gi, items = cases
    items = items[:24]
    n = len(items)
    cand_max, rows_cap = UC.bounds(corpus, items)
    ops, (c_ptr, c_terms) = UC.operands(items, corpus.n_terms)
    n_cls = c_ptr.size - 1
    cls_want = UC.class_lists(corpus, items)
    cap = int(cls_want[0][-1]) + rows_cap
    want_ptr, want_docs = UC.expected_lists(corpus, items, before=cls_want)
    o = [dev_arr(a, dt) for a, dt in zip(ops, I_OPS)]
    cp, ct = dev_arr(c_ptr, torch.int64), dev_arr(c_terms, torch.int32)
    lp = torch.zeros(n_cls + n + 1, dtype=torch.int64, device=DEV)
    dc = torch.zeros(cap, dtype=torch.int32, device=DEV)
    st = torch.zeros(n_cls + n, dtype=torch.int32, device=DEV)
    uwb, wwb = nat.union_lists_plan(n_cls, gi.n_docs), nat.unit_spans_plan(n, cand_max)
    uwork, wwork = (torch.empty(b, dtype=torch.uint8, device=DEV) for b in (uwb, wwb))

    def step():
        s = stream_ptr()
        gi.union_lists_device(cp.data_ptr(), ct.data_ptr(), n_cls, 0, cap, lp.data_ptr(), dc.data_ptr(), st.data_ptr(),
                              uwork.data_ptr(), uwb, s)
        gi.unit_spans_device(*[x.data_ptr() for x in o], n, cp.data_ptr(), ct.data_ptr(), n_cls, 0, n_cls, cand_max, cap,
                             lp.data_ptr(), dc.data_ptr(), st.data_ptr() + 4 * n_cls, wwork.data_ptr(), wwb, s)

    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):  # an eager run first, outside the capture
        step()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    g0 = nat.workspace_growths()
    for _ in range(2):
        for x in (lp, dc, st, wwork):  # whatever the last run left is gone
            x.fill_(SENTINEL if x.dtype != torch.uint8 else 0xA5)
        graph.replay()
        torch.cuda.synchronize()
        assert nat.workspace_growths() == g0
        assert np.array_equal(lp.cpu().numpy(), want_ptr) and np.array_equal(dc.cpu().numpy()[:want_ptr[-1]], want_docs)
        assert not st.cpu().numpy().any() and want_ptr[-1] > cls_want[0][-1]


# ---- through pack() and the engine ---------------------------------------------------------------------------------------------
def test_a_within_stands_wherever_a_term_may_through_pack_and_term_scopes(nat, cases):
    from legal_rag_amd.retrieval.engine import HybridEngine
    from legal_rag_amd.retrieval.terms import Near, NearOf, OneOf, Phrase, Prefix, Terms, Within, pack
    corpus, gi, _ = cases
    w = UC.word
    vocab = {w(t): t for t in range(corpus.n_terms)}
    df = {w(t): int(x) for t, x in enumerate(corpus.df())}
    ab = Within(w(UC.A), w(UC.B))
    pk = Within(OneOf(w(UC.K0), w(UC.K0 + 1)), w(UC.B), unit="paragraph")
    kb = Within(w(UC.B), Prefix("k"), unit="paragraph", ordered=True)
    w23 = Within(w(2), w(3), w(2))
    terms = [Terms(all_of=[ab]), Terms(all_of=[w(UC.A)], none_of=[ab]), Terms(any_of=[pk, kb, w(UC.G)]),
             Terms(all_of=[(w23, Phrase(w(2), w(3)), Prefix("k"))]), Terms(all_of=[w23, NearOf(OneOf(w(4), w(5)), w(2), distance=3)]),
             Terms(all_of=[Within(w(2), "nowhere")]), Terms(none_of=[(Within(w(3), w(4), ordered=True), w(2))], all_of=[Near(w(2), w(3), distance=2)])]
    tt = pack([(None, t) for t in terms], vocab, df, corpus.n_docs)
    assert tt.n_unit == 6 and tt.n_cspan == 1 and tt.n_union >= 3 and tt.n_phr == 1 and tt.n_near == 1
    words = [[w(t) for t in seq] for seq in corpus.docs]
    want = [np.asarray([d for d in range(corpus.n_docs) if t.matches(words[d], corpus.breaks[d])], np.int64) for t in terms]
    assert want[5].size == 0 and all(x.size for i, x in enumerate(want) if i != 5)
    want_ptr = np.zeros(len(want) + 1, np.int64)
    np.cumsum([x.size for x in want], out=want_ptr[1:])
    eng = HybridEngine(None, gi, None)
    table, st = eng.term_scopes(tt)
    torch.cuda.synchronize()
    n_x = tt.n_phr + tt.n_near + tt.n_union + tt.n_cspan + tt.n_unit
    assert st.dtype == torch.int32 and st.numel() == len(terms) + n_x and not st.cpu().numpy().any()
    assert np.array_equal(table[0].cpu().numpy(), want_ptr)
    assert np.array_equal(table[1].cpu().numpy()[:want_ptr[-1]], np.concatenate(want))
    # a Within alone in a table: the unit step starts the array
    t1 = pack([(None, Terms(all_of=[ab]))], vocab, df, corpus.n_docs)
    assert (t1.n_phr, t1.n_near, t1.n_union, t1.n_cspan, t1.n_unit) == (0, 0, 0, 0, 1)
    table1, st1 = eng.term_scopes(t1)
    torch.cuda.synchronize()
    assert st1.numel() == 2 and not st1.cpu().numpy().any() and table1[0].cpu().numpy().tolist() == [0, want[0].size]
    assert np.array_equal(table1[1].cpu().numpy()[:want[0].size], want[0])
    # an overflow of the unit step's bound lands at the Within's place
    t1.unit_rows_cap = want[0].size - 1
    _, st2 = eng.term_scopes(t1)
    torch.cuda.synchronize()
    assert st2.cpu().numpy()[1:].tolist() == [2]

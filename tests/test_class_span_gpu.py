"""Class spans resolved on the GPU (amdr_class_spans: csrc/class_span.hip, csrc/class_span_rule.hpp) and read by the term step
as virtual posting lists: the device lists and the host twin's equal the reference of tests/class_span_cases.py byte for
byte — `PhraseOf.within` / `NearOf.within` over the documents' words — at the smallest shapes where the kernels can go
wrong (documents of 1 .. 320 tokens, classes of 1 .. 4 096 ids, drivers around the tile, 1, 2 and 65 items); three
equivalences against code that exists; the list array continued behind earlier lists; the status words; argument errors; a
handle without a token stream; the lists across updates; capture of the span, union, class and term steps in one chain;
a class span wherever a term id may stand, through pack() and HybridEngine.term_scopes."""
import numpy as np
import pytest
import torch

import class_span_cases as CC
import near_cases as NC
import phrase_cases as PC
import term_scope_cases as TC
import union_cases as UC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = -77
T_OPS = (torch.int64, torch.int32, torch.int64, torch.int32, torch.int64, torch.int64, torch.int32)
I_OPS = (torch.int64, torch.int32, torch.int32, torch.int32)
EMPTY = (np.zeros(1, np.int64), np.zeros(0, np.int32))


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


def make_index(nat, corpus, stream=True):
    tp, pd, pt, idf, dl, avgdl = corpus.postings()
    gi = nat.BM25Index(tp, pd, pt, idf, dl, avgdl)
    if stream:
        gi.set_tokens(*corpus.stream())
    return gi


@pytest.fixture(scope="module")
def rand(nat):
    corpus = PC.rand_corpus()
    return corpus, make_index(nat, corpus)


def dev_arr(a, dtype):
    t = torch.zeros(max(int(np.size(a)), 1), dtype=dtype, device=DEV)
    if np.size(a):
        t[:np.size(a)].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def run_device(nat, gi, corpus, items, cand_max, rows_cap, before=EMPTY):
    """The union step for the items' classes and amdr_class_spans_device behind it, on fresh tensors, continuing the array
    `before` = (list_ptr, docs): (list_ptr, docs [capacity], the items' status) as numpy arrays; what no call writes keeps
    SENTINEL.  rows_cap: the room of the ITEMS' documents; the classes' lists get exactly theirs."""
    k, n = before[0].size - 1, len(items)
    ops, (c_ptr, c_terms) = CC.operands(items, corpus.n_terms, cls_first=k)
    n_cls = c_ptr.size - 1
    cls_want = CC.class_lists(corpus, items, before=before)
    cap = int(cls_want[0][-1]) + rows_cap
    o = [dev_arr(a, dt) for a, dt in zip(ops, I_OPS)]
    cp, ct = dev_arr(c_ptr, torch.int64), dev_arr(c_terms, torch.int32)
    lp = torch.full((k + n_cls + n + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    dc = torch.full((max(cap, 1),), SENTINEL, dtype=torch.int32, device=DEV)
    lp[:k + 1].copy_(torch.from_numpy(before[0]))
    if before[1].size:
        dc[:before[1].size].copy_(torch.from_numpy(before[1]))
    st = torch.full((max(n_cls + n, 1),), SENTINEL, dtype=torch.int32, device=DEV)
    uwb, cwb = nat.union_lists_plan(n_cls, gi.n_docs), nat.class_spans_plan(n, cand_max)
    uwork = torch.empty(max(uwb, 1), dtype=torch.uint8, device=DEV)
    cwork = torch.empty(max(cwb, 1), dtype=torch.uint8, device=DEV)
    s = stream_ptr()
    gi.union_lists_device(cp.data_ptr(), ct.data_ptr(), n_cls, k, cap, lp.data_ptr(), dc.data_ptr(), st.data_ptr(),
                          uwork.data_ptr(), uwb, s)
    gi.class_spans_device(*[x.data_ptr() for x in o], n, cp.data_ptr(), ct.data_ptr(), n_cls, k, k + n_cls, cand_max, cap,
                          lp.data_ptr(), dc.data_ptr(), st.data_ptr() + 4 * n_cls, cwork.data_ptr(), cwb, s)
    torch.cuda.synchronize()
    got_lp, got_dc, got_st = lp.cpu().numpy(), dc.cpu().numpy()[:cap], st.cpu().numpy()
    assert np.array_equal(got_lp[:k + n_cls + 1], cls_want[0]) and not got_st[:n_cls].any()       # the classes' lists, as the
    assert np.array_equal(got_dc[:cls_want[0][-1]].view(np.uint8), cls_want[1].view(np.uint8))    # union step left them
    return got_lp, got_dc, got_st[n_cls:n_cls + n]


def run_twin(gi, corpus, items, cand_max, rows_cap):
    ops, classes = CC.operands(items, corpus.n_terms)
    return gi.class_spans(*ops, *classes, cand_max, rows_cap)


def check_both(nat, corpus, gi, items, before=EMPTY):
    cand_max, rows_cap = CC.bounds(corpus, items)
    cls_ptr, cls_docs = CC.class_lists(corpus, items, before=before)
    want_ptr, want_docs = CC.expected_lists(corpus, items, before=(cls_ptr, cls_docs))
    total = int(want_ptr[-1] - cls_ptr[-1])
    assert rows_cap >= total
    for cap in (rows_cap, total):  # the bound a caller knows; a capacity of exactly the lists
        lp, docs, status = run_device(nat, gi, corpus, items, cand_max, cap, before=before)
        assert lp.dtype == np.int64 and np.array_equal(lp, want_ptr), (lp, want_ptr)
        assert docs.dtype == np.int32 and np.array_equal(docs[:want_ptr[-1]].view(np.uint8), want_docs.view(np.uint8))
        assert status.dtype == np.int32 and not status.any(), status
        assert np.all(docs[want_ptr[-1]:] == SENTINEL)  # nothing is written past the lists
    t_ptr, t_docs = CC.expected_lists(corpus, items)
    lp, docs, status = run_twin(gi, corpus, items, cand_max, rows_cap)
    assert lp.dtype == np.int64 and np.array_equal(lp, t_ptr) and not status.any()
    assert docs.dtype == np.int32 and np.array_equal(docs.view(np.uint8), t_docs.view(np.uint8))
    return want_ptr, want_docs


# ---- the lists ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", CC.SIZES)
def test_document_lengths_match_positions_class_sizes_and_1_2_65_items_per_call(nat, m):
    corpus, at = CC.edge_corpus(m)
    gi = make_index(nat, corpus)
    named = CC.edge_items(m)
    items = CC.batch(corpus, named, 65)
    want_ptr, _ = check_both(nat, corpus, gi, items)
    idx = {name: i for i, name in enumerate(named)}
    n_cls = len(CC.classes_of(items))
    sizes = np.diff(want_ptr)[n_cls:]
    assert sizes[idx["near"]] > 0 and sizes[idx["phrase"]] > 0 and sizes[idx["equal slots"]] > 0
    assert not sizes[[idx[x] for x in ("empty class", "nowhere", "unknown -1", "unknown past the classes", "phrase of two")]].any()
    for name in ("near", "ordered", "phrase", "equal slots", "every k", "unknown -1"):  # alone: another grid, the same list
        check_both(nat, corpus, gi, [named[name]])
    check_both(nat, corpus, gi, [named["three"], named["near reversed"]])
    # NearOf(A, B, distance=1, ordered=True) is PhraseOf(A, B)
    a, b = (run_device(nat, gi, corpus, [named[x]], *CC.bounds(corpus, [named[x]])) for x in ("ordered 1", "phrase"))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8)) and a[0][-1] > a[0][-2]
    lp0, docs0, st0 = gi.class_spans(*CC.operands([], corpus.n_terms)[0], *EMPTY, 0, 0)  # no item: an empty array
    assert lp0.tolist() == [0] and docs0.size == 0 and st0.size == 0


@pytest.mark.parametrize("count", CC.DRIVER_COUNTS)
def test_drivers_around_the_tile_a_class_list_or_a_plain_posting_and_the_status_words(nat, count):
    corpus = CC.driver_corpus(count)
    gi = make_index(nat, corpus)
    named = CC.driver_items()
    items = list(named.values())
    want_ptr, want_docs = check_both(nat, corpus, gi, items)
    cand_max, rows_cap = CC.bounds(corpus, items)
    assert cand_max == count + 1 and CC.driver(corpus, items[0]) == (1, count)
    n_cls = 1
    t_ptr, t_docs = CC.expected_lists(corpus, items)
    # cand_max one below the longest driver: status 1 and no rows for the items it drives, the others as they were
    over = [CC.driver(corpus, it)[1] > cand_max - 1 for it in items]
    assert any(over) and not all(over)
    kept = [CC.item_list(corpus, it) if not o else np.zeros(0, np.int32) for it, o in zip(items, over)]
    for lp, docs, status in (run_device(nat, gi, corpus, items, cand_max - 1, rows_cap), run_twin(gi, corpus, items, cand_max - 1, rows_cap)):
        assert status.tolist() == [1 if o else 0 for o in over]
        assert np.diff(lp)[-len(items):].tolist() == [x.size for x in kept]
        assert np.array_equal(docs[lp[-len(items) - 1]:lp[-1]], np.concatenate(kept))
    # a capacity one below the total: status 2 from the first item that does not fit, the documents that fit unchanged
    total = int(t_ptr[-1])
    for cap in (total - 1, int(t_ptr[2]) - 1, 0):
        first = int(np.searchsorted(t_ptr[1:], cap, side="right"))
        flags = [2 if p >= first and t_ptr[p + 1] > t_ptr[p] else 0 for p in range(len(items))]
        lp, docs, status = run_device(nat, gi, corpus, items, cand_max, cap)
        base = int(want_ptr[n_cls])
        assert status.tolist() == flags and np.array_equal(lp[n_cls:], base + np.minimum(t_ptr, cap))
        assert np.array_equal(docs[base:base + cap], t_docs[:cap])
        lp, docs, status = run_twin(gi, corpus, items, cand_max, cap)
        assert status.tolist() == flags and np.array_equal(lp, np.minimum(t_ptr, cap)) and np.array_equal(docs, t_docs[:cap])


# ---- equivalences against code that exists -------------------------------------------------------------------------------------
def test_plain_items_give_the_bytes_of_the_span_step_and_a_one_id_class_the_plain_tokens_list(nat, rand):
    corpus, gi = rand
    items = NC.scope_items(corpus) + [NC.near([0, 1], 3), NC.phrase([1, 0]), NC.near([2, 2, 0], 4), NC.near([0, -1], 3)]
    cand_max, rows_cap = NC.bounds(corpus, items)
    s_lp, s_docs, s_status = gi.span_lists(*NC.operands(items), cand_max, rows_cap)
    lp, docs, status = run_device(nat, gi, corpus, items, cand_max, rows_cap)
    assert np.array_equal(lp, s_lp) and np.array_equal(docs[:lp[-1]].view(np.uint8), s_docs.view(np.uint8))
    assert np.array_equal(status, s_status) and lp[-1] > 0
    t_lp, t_docs, _ = run_twin(gi, corpus, items, cand_max, rows_cap)
    assert np.array_equal(t_lp, s_lp) and np.array_equal(t_docs.view(np.uint8), s_docs.view(np.uint8))
    # every token a class of its own id: the same lists, behind the classes'
    classy = [(kind, [CC.cls(t) if t >= 0 else t for t in terms], n) for kind, terms, n in items]
    lp1, docs1, status1 = run_device(nat, gi, corpus, classy, cand_max, rows_cap)
    n_cls = len(CC.classes_of(classy))
    assert n_cls == len({t for _, terms, _ in items for t in terms if t >= 0}) and np.array_equal(lp1[n_cls:] - lp1[n_cls], s_lp) and not status1.any()
    assert np.array_equal(docs1[lp1[n_cls]:lp1[-1]].view(np.uint8), s_docs.view(np.uint8))


# ---- one list array ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spans,unions", [(0, 1), (3, 2)])
def test_the_class_step_continues_the_array_behind_spans_and_unions(nat, rand, spans, unions):
    corpus, gi = rand
    first = NC.expected_lists(corpus, NC.scope_items(corpus)[:spans]) if spans else EMPTY
    before = UC.expected_lists(corpus, UC.chain_unions(corpus)[:unions], before=first)
    assert before[0].size - 1 == spans + unions and before[0][-1] > 0
    order = [int(t) for t in np.argsort(-corpus.df())]
    A, B_ = CC.cls(*order[:2]), CC.cls(*order[2:5])
    items = [CC.near_of([A, B_], 2), CC.phrase_of([A, order[5]]), CC.near_of([B_, A, A], 6, True), CC.near_of([A, A], 1),
             CC.near_of([order[-1], A], 40), CC.phrase_of([A, -1])]
    want_ptr, want_docs = check_both(nat, corpus, gi, items, before=before)  # (run_device asserts the classes' part)
    k = before[0].size - 1
    assert np.array_equal(want_ptr[:k + 1], before[0]) and np.array_equal(want_docs[:before[0][-1]], before[1])
    assert np.diff(want_ptr)[k + 2:k + 5].min() > 0
    lp, docs, _ = run_device(nat, gi, corpus, items, *CC.bounds(corpus, items), before=before)
    used = int(before[0][-1])  # every earlier byte untouched
    assert np.array_equal(lp[:k + 1], before[0]) and np.array_equal(docs[:used].view(np.uint8), before[1].view(np.uint8))


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing_and_leave_the_outputs_untouched(nat, rand):
    corpus, gi = rand
    order = [int(t) for t in np.argsort(-corpus.df())]
    items = [CC.near_of([CC.cls(*order[:2]), order[2]], 3), CC.phrase_of([order[0], CC.cls(*order[1:4])])]
    n, n_cls = 2, 2
    cand_max, rows_cap = CC.bounds(corpus, items)
    cls_ptr, cls_docs = CC.class_lists(corpus, items)
    cap = int(cls_ptr[-1]) + rows_cap
    ops, (c_ptr, c_terms) = CC.operands(items, corpus.n_terms)
    o = [dev_arr(a, dt) for a, dt in zip(ops, I_OPS)]
    cp, ct = dev_arr(c_ptr, torch.int64), dev_arr(c_terms, torch.int32)
    lp = torch.full((n_cls + n + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    dc = torch.full((cap,), SENTINEL, dtype=torch.int32, device=DEV)
    st = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    wb = nat.class_spans_plan(n, cand_max)
    work = torch.empty(wb, dtype=torch.uint8, device=DEV)
    good = dict(ip=o[0].data_ptr(), sl=o[1].data_ptr(), kd=o[2].data_ptr(), ds=o[3].data_ptr(), n=n, cp=cp.data_ptr(),
                ct=ct.data_ptr(), n_cls=n_cls, first=0, before=n_cls, cand=cand_max, cap=cap, lp=lp.data_ptr(), dc=dc.data_ptr(),
                st=st.data_ptr(), work=work.data_ptr(), wb=wb)

    def call(index=gi, **over):
        a = dict(good, **over)
        index.class_spans_device(a["ip"], a["sl"], a["kd"], a["ds"], a["n"], a["cp"], a["ct"], a["n_cls"], a["first"], a["before"],
                                 a["cand"], a["cap"], a["lp"], a["dc"], a["st"], a["work"], a["wb"], stream_ptr())
    for over in (dict(n=-1), dict(n_cls=-1), dict(first=-1), dict(before=-1), dict(cand=-1), dict(cap=-1), dict(wb=-1), dict(wb=wb - 1),
                 dict(work=0), dict(lp=0), dict(dc=0), dict(st=0), dict(ip=0), dict(sl=0), dict(kd=0), dict(ds=0), dict(cp=0),
                 dict(ct=0), dict(before=1), dict(first=1), dict(n_cls=3), dict(n=2**24), dict(n=2**31),
                 dict(n=2**23, cand=257)):  # classes beyond the lists written before; cells x 256 threads >= 2^32
        with pytest.raises(nat.NativeError):
            call(**over)
    bare = make_index(nat, corpus, stream=False)  # a handle without a token stream: both forms refuse
    with pytest.raises(nat.NativeError, match="no token stream"):
        call(index=bare)
    with pytest.raises(nat.NativeError, match="no token stream"):
        run_twin(bare, corpus, items, cand_max, rows_cap)
    torch.cuda.synchronize()
    assert (lp == SENTINEL).all() and (dc == SENTINEL).all() and (st == SENTINEL).all()
    # the twin validates: pointers, kinds, lengths, distances, member order, the overlap rule
    (ip, sl, kd, ds), (c_ptr, c_terms) = ops, (c_ptr, c_terms)
    V = corpus.n_terms
    for bad, what in (((np.asarray([1, 2, 4], np.int64), sl, kd, ds, c_ptr, c_terms), "item_ptr"),
                      ((ip, sl, np.asarray([3, 0], np.int32), ds, c_ptr, c_terms), "kind"),
                      ((np.asarray([0, 1, 4], np.int64), sl, kd, ds, c_ptr, c_terms), "fewer than 2"),
                      ((ip, sl, kd, np.asarray([256, 0], np.int32), c_ptr, c_terms), "distance"),
                      ((ip, sl, kd, ds, np.asarray([0, 3, 2], np.int64), c_terms), "cls_ptr"),
                      ((ip, sl, kd, ds, c_ptr, c_terms[::-1].copy()), "strictly ascending"),
                      ((ip, np.asarray([V + 0, order[0], order[0], V + 1], np.int32), kd, ds, c_ptr, c_terms), "overlapping")):
        with pytest.raises(nat.NativeError, match=what):
            gi.class_spans(*bad, cand_max, rows_cap)
    with pytest.raises(nat.NativeError):
        gi.class_spans(ip, sl, kd, ds, c_ptr, c_terms, cand_max, -1)
    want_ptr, want_docs = CC.expected_lists(corpus, items, before=(cls_ptr, cls_docs))
    lp.copy_(torch.from_numpy(np.concatenate([cls_ptr, np.full(n, SENTINEL, np.int64)])))
    dc[:cls_docs.size].copy_(torch.from_numpy(cls_docs))
    call()  # the same buffers with the arguments as they should be
    torch.cuda.synchronize()
    assert np.array_equal(lp.cpu().numpy(), want_ptr) and np.array_equal(dc.cpu().numpy()[:want_ptr[-1]], want_docs)
    assert not st.cpu().numpy().any() and want_ptr[-1] > cls_ptr[-1]


# ---- updates -----------------------------------------------------------------------------------------------------------------
def test_after_add_remove_and_replace_set_tokens_brings_the_lists_of_the_edited_corpus(nat):
    corpus = PC.SeqCorpus("small", 4, [[0, 1, 2], [1, 3, 0], [], [2, 2, 0, 3, 1], [3, 0, 1], [1]])
    V = corpus.n_terms
    idf = np.linspace(0.5, 3.0, V)
    one = PC.SeqCorpus("one", V, [[2, 0, 3]])
    a_ptr, a_doc, a_tf, _, a_len, _ = one.postings()
    items = [CC.near_of([CC.cls(0, 1), 3], 1), CC.phrase_of([CC.cls(2, 3), CC.cls(0, 1)]), CC.near_of([CC.cls(0, 1), CC.cls(0, 1), 2], 2),
             CC.near_of([3, CC.cls(0, 2)], 2, True)]

    def same(gi, after):
        with pytest.raises(nat.NativeError, match="no token stream"):  # the update dropped it
            run_twin(gi, after, items, *CC.bounds(after, items))
        gi.set_tokens(*after.stream())
        check_both(nat, after, gi, items)
    gi = make_index(nat, corpus)
    check_both(nat, corpus, gi, items)
    assert CC.item_list(corpus, items[0]).tolist() == [1, 3, 4]
    gi.add(a_ptr, a_doc, a_tf, idf, a_len, 2.0)
    added = PC.SeqCorpus("added", V, corpus.docs + one.docs)
    assert CC.item_list(added, items[0]).tolist() == [1, 3, 4, 6]
    same(gi, added)
    gi = make_index(nat, corpus)
    gi.remove(np.asarray([3], np.int64), idf, 2.0)
    same(gi, PC.SeqCorpus("removed", V, corpus.docs[:3] + corpus.docs[4:]))
    gi = make_index(nat, corpus)
    gi.replace(np.asarray([5], np.int64), a_ptr, a_doc, a_tf, a_len, idf, 2.0)
    after = PC.SeqCorpus("replaced", V, corpus.docs[:5] + one.docs)
    assert CC.item_list(after, items[0]).tolist() == [1, 3, 4, 5]
    same(gi, after)


# ---- capture -----------------------------------------------------------------------------------------------------------------
def test_captured_span_union_class_and_term_steps_replay_with_the_items_rewritten_in_place(nat, rand):
    """One linear chain on one stream: the span step's three launches, the union step's, the class step's, the term step's."""
    corpus, gi = rand
    V, k, u, n, M = corpus.n_terms, 2, 2, 3, 3  # two phrases in front, two unions of three ids, three class spans of two slots
    n_x = k + u + n
    cand_max, rows_cap = corpus.n_docs, n_x * corpus.n_docs  # hold for every item over this corpus
    fam = TC.Family("each list alone", "rand", [TC.c([(TC.MUST, [V + p])]) for p in range(n_x)])
    t = [dev_arr(a, dt) for a, dt in zip(TC.operands(fam), T_OPS)]
    sp_ptr = dev_arr(np.arange(0, 2 * k + 1, 2), torch.int64)
    sp_terms = torch.zeros(2 * k, dtype=torch.int32, device=DEV)
    sp_kind, sp_dist = torch.zeros(k, dtype=torch.int32, device=DEV), torch.zeros(k, dtype=torch.int32, device=DEV)
    ip = dev_arr(np.arange(0, u * M + 1, M), torch.int64)
    it_ = torch.zeros(u * M, dtype=torch.int32, device=DEV)
    c_ptr = dev_arr(np.arange(0, 2 * n + 1, 2), torch.int64)
    c_slots, c_kind, c_dist = (torch.zeros(sz, dtype=torch.int32, device=DEV) for sz in (2 * n, n, n))
    lp = torch.zeros(n_x + 1, dtype=torch.int64, device=DEV)
    dc = torch.zeros(rows_cap, dtype=torch.int32, device=DEV)
    pst = torch.zeros(n_x, dtype=torch.int32, device=DEV)
    sp = torch.zeros(n_x + 1, dtype=torch.int64, device=DEV)
    rw = torch.zeros(rows_cap, dtype=torch.int64, device=DEV)
    st = torch.zeros(n_x, dtype=torch.int32, device=DEV)
    swb, uwb = nat.span_lists_plan(k, cand_max), nat.union_lists_plan(u, gi.n_docs)
    cwb, wb = nat.class_spans_plan(n, cand_max), nat.term_scope_plan(n_x, cand_max)
    swork, uwork, cwork, work = (torch.empty(b, dtype=torch.uint8, device=DEV) for b in (swb, uwb, cwb, wb))

    def variant(seed):
        r = np.random.default_rng(seed)
        phrases = []
        while len(phrases) < k:
            seq = corpus.docs[int(r.integers(0, corpus.n_docs))]
            if len(seq) >= 2:
                s = int(r.integers(0, len(seq) - 1))
                phrases.append([int(seq[s]), int(seq[s + 1])])
        unions = [sorted(set(int(x) for x in r.choice(6, size=M, replace=False))) for _ in range(u)]  # ids 0 .. 5
        kinds = [int(x) for x in r.integers(0, 3, size=n)]
        # (a plain slot from the ids 6 .. 11: disjoint from every class, as the unordered form asks)
        spans = [(kinds[j], [CC.cls(*unions[j % u]), int(r.integers(6, V))] if j % 2 else [int(r.integers(6, V)), CC.cls(*unions[j % u])],
                  0 if kinds[j] == 0 else int(r.integers(1, 6))) for j in range(n)]
        return phrases, unions, spans

    def step():
        s = stream_ptr()
        gi.span_lists_device(sp_ptr.data_ptr(), sp_terms.data_ptr(), sp_kind.data_ptr(), sp_dist.data_ptr(), k, cand_max,
                             rows_cap, lp.data_ptr(), dc.data_ptr(), pst.data_ptr(), swork.data_ptr(), swb, s)
        gi.union_lists_device(ip.data_ptr(), it_.data_ptr(), u, k, rows_cap, lp.data_ptr(), dc.data_ptr(),
                              pst.data_ptr() + 4 * k, uwork.data_ptr(), uwb, s)
        gi.class_spans_device(c_ptr.data_ptr(), c_slots.data_ptr(), c_kind.data_ptr(), c_dist.data_ptr(), n, ip.data_ptr(),
                              it_.data_ptr(), u, k, k + u, cand_max, rows_cap, lp.data_ptr(), dc.data_ptr(),
                              pst.data_ptr() + 4 * (k + u), cwork.data_ptr(), cwb, s)
        gi.term_scope_device([x.data_ptr() for x in t], 0, n_x, n_x, cand_max, rows_cap, sp.data_ptr(), rw.data_ptr(),
                             st.data_ptr(), work.data_ptr(), wb, s, lists=(lp.data_ptr(), dc.data_ptr(), n_x))

    def write(phrases, unions, spans):
        sp_terms.copy_(torch.from_numpy(PC.operands(phrases)[1]))
        it_.copy_(torch.from_numpy(UC.operands(unions)[1]))
        slots = [V + k + unions.index(list(x)) if isinstance(x, tuple) else x for _, sl, _ in spans for x in sl]
        c_slots.copy_(torch.from_numpy(np.asarray(slots, np.int32)))
        c_kind.copy_(torch.from_numpy(np.asarray([s[0] for s in spans], np.int32)))
        c_dist.copy_(torch.from_numpy(np.asarray([s[2] for s in spans], np.int32)))

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
        phrases, unions, spans = variant(seed)
        write(phrases, unions, spans)
        graph.replay()
        got = snapshot()
        assert nat.workspace_growths() == g0
        first = UC.expected_lists(corpus, unions, before=PC.expected_lists(corpus, phrases))
        want_ptr, want_docs = CC.expected_lists(corpus, spans, before=first)
        assert want_ptr[k] > 0 and want_ptr[k + u] > want_ptr[k] and want_ptr[-1] > want_ptr[k + u]
        assert np.array_equal(got[0], want_ptr) and np.array_equal(got[1][:want_ptr[-1]], want_docs) and not got[2].any()
        assert np.array_equal(got[3], want_ptr) and np.array_equal(got[4][:want_ptr[-1]], want_docs) and not got[5].any()


# ---- through pack() and the engine ---------------------------------------------------------------------------------------------
def test_a_class_span_stands_wherever_a_term_may_through_pack_and_term_scopes(nat, rand):
    """MUST and driver, MUST beside a rarer plain term, ANY, NOT, inside a tuple group next to a Phrase and a Prefix, a
    folded item beside its plain form, an item with an unknown slot — against Terms.matches over the documents' words."""
    from legal_rag_amd.retrieval.engine import HybridEngine
    from legal_rag_amd.retrieval.terms import Near, NearOf, OneOf, Phrase, PhraseOf, Prefix, Terms, pack
    corpus, gi = rand
    order = [int(t) for t in np.argsort(-corpus.df())]
    w = [CC.word(t) for t in order]
    vocab = {CC.word(t): t for t in range(corpus.n_terms)}
    df = {CC.word(t): int(x) for t, x in enumerate(corpus.df())}
    ab, cde = OneOf(w[0], w[1]), OneOf(w[2], w[3], w[4])
    n1, p1, o1 = NearOf(ab, cde, distance=2), PhraseOf(ab, w[5]), NearOf(cde, ab, ab, distance=6, ordered=True)
    terms = [Terms(all_of=[n1]), Terms(all_of=[p1, w[7]]), Terms(all_of=[w[0]], any_of=[o1, w[-2]]), Terms(all_of=[w[1]], none_of=[n1]),
             Terms(all_of=[(p1, Phrase(w[0], w[1]), Prefix("w1"))]), Terms(all_of=[n1, o1]),
             Terms(any_of=[NearOf(w[0], OneOf(w[1]), distance=3), Near(w[0], w[1], distance=3)]),
             Terms(all_of=[NearOf(ab, Prefix("nowhere"), distance=9)]), Terms(none_of=[(PhraseOf(w[6], cde), w[0])])]
    tt = pack([(None, t) for t in terms], vocab, df, corpus.n_docs)
    assert tt.n_cspan == 5 and tt.n_union >= 2 and tt.n_near == 1 and tt.n_phr == 1
    words = CC.words_of(corpus)
    want = [np.asarray([d for d, ws in enumerate(words) if t.matches(ws)], np.int64) for t in terms]
    assert want[7].size == 0 and all(x.size for i, x in enumerate(want) if i != 7)
    want_ptr = np.zeros(len(want) + 1, np.int64)
    np.cumsum([x.size for x in want], out=want_ptr[1:])
    eng = HybridEngine(None, gi, None)
    table, st = eng.term_scopes(tt)
    torch.cuda.synchronize()
    n_x = tt.n_phr + tt.n_near + tt.n_union + tt.n_cspan
    assert st.dtype == torch.int32 and st.numel() == len(terms) + n_x and not st.cpu().numpy().any()
    assert np.array_equal(table[0].cpu().numpy(), want_ptr)
    assert np.array_equal(table[1].cpu().numpy()[:want_ptr[-1]], np.concatenate(want))
    # class spans alone in a table whose only unions are theirs
    t1 = pack([(None, Terms(all_of=[p1]))], vocab, df, corpus.n_docs)
    assert (t1.n_phr, t1.n_near, t1.n_union, t1.n_cspan) == (0, 0, 1, 1)
    table1, st1 = eng.term_scopes(t1)
    torch.cuda.synchronize()
    one = np.asarray([d for d, ws in enumerate(words) if p1.within(ws)], np.int64)
    assert st1.numel() == 3 and not st1.cpu().numpy().any() and table1[0].cpu().numpy().tolist() == [0, one.size]
    assert np.array_equal(table1[1].cpu().numpy()[:one.size], one)
    # an overflow of the class step's bound lands behind the unions' words, at the class span's place
    t1.cspan_rows_cap = one.size - 1
    lists = CC.class_lists(corpus, [CC.phrase_of([CC.cls(order[0], order[1]), order[5]])])
    t1.union_rows_cap = int(lists[0][-1])  # (the array's capacity: the union's part exact, the span's one short)
    _, st2 = eng.term_scopes(t1)
    torch.cuda.synchronize()
    assert st2.cpu().numpy()[1:].tolist() == [0, 2]

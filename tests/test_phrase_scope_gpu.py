"""Phrases resolved on the GPU (csrc/phrase_scope.hip) and read by the term step as virtual posting lists
(csrc/term_scope.hip): the device lists and the host twin's equal the reference of tests/phrase_cases.py exactly — a plain
window scan of every document — at the smallest shapes where the kernels can go wrong; the status words at both bounds;
argument errors; the token stream's validation and its life across add / remove / replace; capture; a phrase wherever a
term id may stand in a constraint; the bound from upper bounds; the scoped channels on the device-built table against the
host-uploaded one."""
import ctypes as C

import numpy as np
import pytest
import torch

import phrase_cases as PC
import term_scope_cases as TC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = -77


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
def world(nat):
    """name -> (corpus, its BM25Index with the token stream resident)."""
    edge, at = PC.edge_corpus()
    out = {"edge": edge, "tiles": PC.tiles_corpus(), "rand": PC.rand_corpus()}
    return {name: (c, make_index(nat, c)) for name, c in out.items()}, at


def dev_arr(a, dtype):
    """A device tensor of the array (one element at least: an empty operand still has an address)."""
    t = torch.zeros(max(int(np.size(a)), 1), dtype=dtype, device=DEV)
    if np.size(a):
        t[:np.size(a)].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def run_device(nat, gi, phrases, cand_max, rows_cap):
    """amdr_phrase_lists_device on fresh tensors: (list_ptr, docs [rows_cap], status) as numpy arrays; what the call does
    not write keeps SENTINEL."""
    pp, pt = PC.operands(phrases)
    n_phr = len(phrases)
    tp, tt = dev_arr(pp, torch.int64), dev_arr(pt, torch.int32)
    lp = torch.full((n_phr + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    dc = torch.full((max(rows_cap, 1),), SENTINEL, dtype=torch.int32, device=DEV)
    st = torch.full((max(n_phr, 1),), SENTINEL, dtype=torch.int32, device=DEV)
    wb = nat.phrase_lists_plan(n_phr, cand_max)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=DEV)
    gi.phrase_lists_device(tp.data_ptr(), tt.data_ptr(), n_phr, cand_max, rows_cap, lp.data_ptr(), dc.data_ptr(),
                           st.data_ptr(), work.data_ptr(), wb, stream_ptr())
    torch.cuda.synchronize()
    return lp.cpu().numpy(), dc.cpu().numpy()[:rows_cap], st.cpu().numpy()[:n_phr]


def run_twin(gi, phrases, cand_max, rows_cap):
    return gi.phrase_lists(*PC.operands(phrases), cand_max, rows_cap)


def bounds(corpus, phrases):
    lens = [PC.driver_len(corpus, p) for p in phrases]
    return lens, max(lens, default=0), sum(lens)


def assert_lists(got, want_ptr, want_docs, device_cap=None):
    lp, docs, status = got
    assert np.array_equal(lp, want_ptr), (lp, want_ptr)
    assert docs.dtype == np.int32 and np.array_equal(docs[:want_ptr[-1]], want_docs)
    assert not status.any(), status
    if device_cap is not None:  # nothing is written past the lists
        assert np.all(docs[want_ptr[-1]:] == SENTINEL)


def check_both(nat, corpus, gi, phrases):
    want_ptr, want_docs = PC.expected_lists(corpus, phrases)
    lens, cand_max, rows_cap = bounds(corpus, phrases)
    assert_lists(run_device(nat, gi, phrases, cand_max, rows_cap), want_ptr, want_docs, rows_cap)
    assert_lists(run_twin(gi, phrases, cand_max, rows_cap), want_ptr, want_docs)
    # bounds larger than needed (another tile count) and a rows_cap of exactly the lists change nothing
    assert_lists(run_device(nat, gi, phrases, cand_max + 700, int(want_ptr[-1])), want_ptr, want_docs)
    assert_lists(run_twin(gi, phrases, cand_max + 700, int(want_ptr[-1])), want_ptr, want_docs)
    for p in range(len(phrases)):
        assert np.all(np.diff(want_docs[want_ptr[p]:want_ptr[p + 1]]) > 0)
    return want_ptr, want_docs


# ---- the lists ---------------------------------------------------------------------------------------------------------------
def test_edge_shapes_lengths_2_3_16_boundaries_overlaps_and_the_lane_stride(nat, world):
    (corpus, gi), at = world[0]["edge"], world[1]
    PC.edge_certificates(corpus, at)
    want_ptr, want_docs = check_both(nat, corpus, gi, PC.EDGE_PHRASES)
    lists = {tuple(p): set(want_docs[want_ptr[i]:want_ptr[i + 1]].tolist()) for i, p in enumerate(PC.EDGE_PHRASES)}
    ab = lists[tuple(PC.AB)]
    assert {0, corpus.n_docs - 1, at["match at the last L tokens"], at["overlap a b a c"]} <= ab
    assert not ab & {at[n] for n in ("empty", "shorter than the phrase", "boundary left", "boundary right", "wrong order",
                                     "not adjacent")}
    assert lists[tuple(PC.ABAC)] == {at["overlap a b a c"]} and at["a a a"] in lists[tuple(PC.AA)]
    assert lists[tuple(PC.W16)] == {at["16 at the end"], at["16 exactly"]}
    assert lists[tuple(PC.ABC)] == {at["a b c"], at["x a b c x"]}
    stride_hits = {at[n] for n in at if n.startswith("stride") and not n.endswith("none")}
    assert lists[tuple(PC.PQ)] == stride_hits and len(stride_hits) == 19
    assert lists[tuple(PC.UV)] == {at["long"]} and lists[(PC.A, PC.B, PC.C_, PC.D)] == set()
    # each phrase alone: another grid, the same list
    for p in PC.EDGE_PHRASES:
        check_both(nat, corpus, gi, [p])


def test_driver_lengths_around_the_tile_and_documents_0_and_n_minus_1(nat, world):
    corpus, gi = world[0]["tiles"]
    PC.tiles_certificates(corpus)
    phrases = PC.tiles_phrases()
    lens, cand_max, _ = bounds(corpus, phrases)
    assert lens == list(PC.DRIVER_LENGTHS) and cand_max == 2 * PC.TILE + 1
    want_ptr, want_docs = check_both(nat, corpus, gi, phrases)
    last = want_docs[want_ptr[-2]:want_ptr[-1]]
    assert last[0] == 0 and last[-1] == corpus.n_docs - 1
    for p in phrases:  # alone: cand_max is the phrase's own driver length (0 tiles of work, 1 tile, 2 tiles, 3 tiles)
        check_both(nat, corpus, gi, [p])


@pytest.mark.parametrize("count", [1, 2, 65])
def test_one_two_and_65_phrases_over_random_documents(nat, world, count):
    corpus, gi = world[0]["rand"]
    phrases = PC.rand_phrases(corpus)
    if count == 65:
        PC.rand_certificates(corpus, phrases)
    check_both(nat, corpus, gi, phrases[:count])


def test_an_id_outside_the_vocabulary_at_each_position_gives_an_empty_list(nat, world):
    corpus, gi = world[0]["edge"]
    phrases = [list(PC.ABC)]
    for j in range(3):
        for bad in (-1, corpus.n_terms, 2**31 - 1):
            ph = list(PC.ABC)
            ph[j] = bad
            phrases.append(ph)
    want_ptr, want_docs = check_both(nat, corpus, gi, phrases)
    assert want_ptr[1] > 0 and want_ptr[-1] == want_ptr[1]
    # lengths the rule does not know (1 and 17) give empty lists from the device call; the twin refuses them
    for odd in ([PC.A], [PC.A] * 17):
        lp, docs, status = run_device(nat, gi, [odd, PC.AB], 100, 100)
        assert lp[1] == 0 and lp[2] == PC.phrase_list(corpus, PC.AB).size and not status.any()
        with pytest.raises(nat.NativeError, match="fewer than 2 or more than 16"):
            run_twin(gi, [odd, PC.AB], 100, 100)


# ---- the status words --------------------------------------------------------------------------------------------------------
def test_cand_max_one_below_the_longest_driver_sets_status_1_for_that_phrase_alone(nat, world):
    corpus, gi = world[0]["tiles"]
    phrases = PC.tiles_phrases()
    lens, cand_max, rows_cap = bounds(corpus, phrases)
    longest = int(np.argmax(lens))
    assert lens.count(cand_max) == 1
    lists = [PC.phrase_list(corpus, p) for p in phrases]
    assert lists[longest].size > 0
    lists[longest] = lists[longest][:0]  # left empty
    want_ptr = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.int64)
    want_docs = np.concatenate(lists)
    for lp, docs, status in (run_device(nat, gi, phrases, cand_max - 1, rows_cap), run_twin(gi, phrases, cand_max - 1, rows_cap)):
        assert status.tolist() == [1 if p == longest else 0 for p in range(len(phrases))]
        assert np.array_equal(lp, want_ptr) and np.array_equal(docs[:want_ptr[-1]], want_docs)


def test_rows_cap_one_below_the_total_sets_status_2_from_the_first_phrase_that_does_not_fit(nat, world):
    corpus, gi = world[0]["tiles"]
    phrases = PC.tiles_phrases()
    lens, cand_max, _ = bounds(corpus, phrases)
    want_ptr, want_docs = PC.expected_lists(corpus, phrases)
    total = int(want_ptr[-1])
    for cap in (total - 1, int(want_ptr[-2]) - 1):  # the last phrase alone loses a document; the last two are cut
        first = int(np.searchsorted(want_ptr[1:], cap, side="right"))
        for lp, docs, status in (run_device(nat, gi, phrases, cand_max, cap), run_twin(gi, phrases, cand_max, cap)):
            assert status.tolist() == [2 if p >= first and want_ptr[p + 1] > want_ptr[p] else 0 for p in range(len(phrases))]
            assert np.array_equal(lp, np.minimum(want_ptr, cap)) and np.array_equal(docs[:cap], want_docs[:cap])


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing_and_leave_the_outputs_untouched(nat, world):
    corpus, gi = world[0]["tiles"]
    phrases = PC.tiles_phrases()
    lens, cand_max, rows_cap = bounds(corpus, phrases)
    n_phr = len(phrases)
    pp, pt = PC.operands(phrases)
    tp, tt = dev_arr(pp, torch.int64), dev_arr(pt, torch.int32)
    lp = torch.full((n_phr + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    dc = torch.full((rows_cap,), SENTINEL, dtype=torch.int32, device=DEV)
    st = torch.full((n_phr,), SENTINEL, dtype=torch.int32, device=DEV)
    wb = nat.phrase_lists_plan(n_phr, cand_max)
    work = torch.empty(wb, dtype=torch.uint8, device=DEV)
    good = dict(pp=tp.data_ptr(), pt=tt.data_ptr(), n_phr=n_phr, cand_max=cand_max, rows_cap=rows_cap, lp=lp.data_ptr(),
                dc=dc.data_ptr(), st=st.data_ptr(), work=work.data_ptr(), wb=wb)

    def call(index=gi, **over):
        a = dict(good, **over)
        index.phrase_lists_device(a["pp"], a["pt"], a["n_phr"], a["cand_max"], a["rows_cap"], a["lp"], a["dc"], a["st"],
                                  a["work"], a["wb"], stream_ptr())
    for over in (dict(n_phr=-1), dict(cand_max=-1), dict(rows_cap=-1), dict(wb=-1), dict(wb=wb - 1), dict(work=0), dict(lp=0),
                 dict(dc=0), dict(st=0), dict(pp=0), dict(pt=0), dict(cand_max=65_536 * PC.TILE)):
        with pytest.raises(nat.NativeError):
            call(**over)
    bare = make_index(nat, corpus, stream=False)  # no resident stream
    with pytest.raises(nat.NativeError, match="no token stream"):
        call(index=bare)
    with pytest.raises(nat.NativeError, match="no token stream"):
        run_twin(bare, phrases, cand_max, rows_cap)
    torch.cuda.synchronize()
    assert (lp == SENTINEL).all() and (dc == SENTINEL).all() and (st == SENTINEL).all()
    call()  # the same buffers with the arguments as they should be
    torch.cuda.synchronize()
    want_ptr, want_docs = PC.expected_lists(corpus, phrases)
    assert np.array_equal(lp.cpu().numpy(), want_ptr) and np.array_equal(dc.cpu().numpy()[:want_ptr[-1]], want_docs)
    # the twin validates the pointer array and the lengths
    for bad_ptr in ([1, 2, 4], [0, 4, 2], [0, 1, 4], [0, 17, 19]):
        with pytest.raises(nat.NativeError):
            gi.phrase_lists(np.asarray(bad_ptr, np.int64), np.zeros(19, np.int32), cand_max, rows_cap)
    lp0, docs0, st0 = gi.phrase_lists(np.zeros(1, np.int64), np.zeros(0, np.int32), 0, 0)  # no phrase: an empty table
    assert lp0.tolist() == [0] and docs0.size == 0 and st0.size == 0
    # the term step's twin validates the virtual lists
    fam = TC.Family("one", "tiles", [TC.c([(TC.MUST, [corpus.n_terms])])])
    ops = TC.operands(fam)
    ok = (np.asarray([0, 3], np.int64), np.asarray([1, 5, 9], np.int32))
    sp, rows, status = gi.term_scope(ops, 3, 3, lists=ok)
    assert rows.tolist() == [1, 5, 9] and not status.any()
    for x_ptr, x_doc in (([1, 3], [1, 5, 9]), ([0, 3, 2], [1, 5, 9]), ([0, 3], [1, 9, 5]), ([0, 3], [1, 5, 5]),
                         ([0, 3], [-1, 5, 9]), ([0, 3], [1, 5, corpus.n_docs])):
        with pytest.raises(nat.NativeError):
            gi.term_scope(ops, 3, 3, lists=(np.asarray(x_ptr, np.int64), np.asarray(x_doc, np.int32)))


# ---- the token stream --------------------------------------------------------------------------------------------------------
def small_corpus():
    return PC.SeqCorpus("small", 4, [[0, 1, 2], [1, 0], [], [2, 2, 0, 1], [3, 0, 1], [1]])


def test_set_tokens_validates_on_the_host_and_leaves_the_handle_unchanged(nat):
    corpus = small_corpus()
    gi = make_index(nat, corpus, stream=False)
    assert gi.tokens_info() == (False, 0)
    with pytest.raises(nat.NativeError, match="no token stream"):
        gi.read_tokens()
    ptr, tok = corpus.stream()
    gi.set_tokens(ptr, tok)
    assert gi.tokens_info() == (True, int(ptr[-1]))
    lib, h = nat.load(), gi._h
    p64 = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def refused(doc_ptr, tokens, what):
        assert lib.amdr_bm25_set_tokens(h, None if doc_ptr is None else p64(doc_ptr), None if tokens is None else p64(tokens)) == -1
        assert what in lib.amdr_last_error().decode(), (what, lib.amdr_last_error())
    refused(None, tok, "null")
    refused(ptr, None, "null")
    off = ptr.copy()
    off[0] = 1
    refused(off, tok, "doc_ptr")
    down = ptr.copy()
    down[2] = down[1] - 1
    refused(down, tok, "doc_ptr")
    for bad in (-1, corpus.n_terms):
        t2 = tok.copy()
        t2[4] = bad
        refused(ptr, t2, "outside [0, n_terms)")
    moved = ptr.copy()
    moved[1] += 1  # document 0 one token longer, document 1 one shorter: the total is unchanged
    refused(moved, tok, "doc_len")
    with pytest.raises(ValueError):
        gi.set_tokens(ptr[:-1], tok)
    # the stream is the one set before the refusals
    got_ptr, got_tok = gi.read_tokens()
    assert np.array_equal(got_ptr, ptr) and np.array_equal(got_tok, tok) and gi.tokens_info() == (True, int(ptr[-1]))
    lp, docs, status = gi.phrase_lists(*PC.operands([[0, 1]]), 6, 6)
    assert docs.tolist() == PC.phrase_list(corpus, [0, 1]).tolist() == [0, 3, 4]
    gi.set_tokens(ptr, tok)  # a second call replaces the stream
    assert gi.phrase_lists(*PC.operands([[0, 1]]), 6, 6)[1].tolist() == [0, 3, 4]


def test_every_successful_update_drops_the_stream_and_a_failed_one_leaves_it(nat):
    corpus = small_corpus()
    V = corpus.n_terms
    idf = np.linspace(0.5, 3.0, V)
    one = PC.SeqCorpus("one", V, [[1, 0, 1]])
    a_ptr, a_doc, a_tf, _, a_len, _ = one.postings()

    def fresh():
        gi = make_index(nat, corpus)
        assert gi.tokens_info()[0]
        return gi

    def gone(gi, after):
        assert gi.tokens_info() == (False, 0)
        with pytest.raises(nat.NativeError, match="no token stream"):
            gi.phrase_lists(*PC.operands([[0, 1]]), 8, 8)
        gi.set_tokens(*after.stream())  # a stream for the new state is accepted, one for the old state is not
        assert gi.phrase_lists(*PC.operands([[0, 1]]), 8, 8)[1].tolist() == PC.phrase_list(after, [0, 1]).tolist()
        if after.n_docs != corpus.n_docs:
            with pytest.raises(ValueError):
                gi.set_tokens(*corpus.stream())
    gi = fresh()
    with pytest.raises(nat.NativeError):
        gi.remove(np.asarray([99], np.int64), idf, 2.0)  # a failed update
    assert gi.tokens_info()[0] and gi.phrase_lists(*PC.operands([[0, 1]]), 8, 8)[1].tolist() == [0, 3, 4]
    gi.add(a_ptr, a_doc, a_tf, idf, a_len, 2.0)
    gone(gi, PC.SeqCorpus("added", V, corpus.docs + one.docs))
    gi = fresh()
    gi.remove(np.asarray([3], np.int64), idf, 2.0)
    gone(gi, PC.SeqCorpus("removed", V, corpus.docs[:3] + corpus.docs[4:]))
    gi = fresh()
    gi.replace(np.asarray([4], np.int64), a_ptr, a_doc, a_tf, a_len, idf, 2.0)
    after = PC.SeqCorpus("replaced", V, corpus.docs[:4] + one.docs + corpus.docs[5:])
    assert PC.phrase_list(after, [0, 1]).tolist() == [0, 3, 4] and PC.phrase_list(after, [1, 0]).tolist() == [1, 4]
    gone(gi, after)
    with pytest.raises(nat.NativeError, match="doc_len"):  # the replaced document has 3 tokens as before; shift one
        ptr, tok = after.stream()
        ptr = ptr.copy()
        ptr[1] -= 1
        gi.set_tokens(ptr, tok)


# ---- through the term step ---------------------------------------------------------------------------------------------------
T_OPS = (torch.int64, torch.int32, torch.int64, torch.int32, torch.int64, torch.int64, torch.int32)


def term_bounds(fam, corpus, ub):
    from legal_rag_amd.retrieval.terms import driver_length
    lens = [driver_length(g, ub, None if b < 0 else int(fam.bases[b].size), corpus.n_docs) for g, b in fam.cons]
    return lens, max(lens), sum(lens)


def run_both_steps_device(nat, gi, phrases, p_max, p_cap, ops, cand_max, rows_cap):
    """The phrase step, then the term step over its lists, on one stream without a synchronise between them."""
    pp, pt = PC.operands(phrases)
    n_phr = len(phrases)
    tp, tt = dev_arr(pp, torch.int64), dev_arr(pt, torch.int32)
    lp = torch.full((n_phr + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    dc = torch.full((max(p_cap, 1),), SENTINEL, dtype=torch.int32, device=DEV)
    pst = torch.full((n_phr,), SENTINEL, dtype=torch.int32, device=DEV)
    pwb = nat.phrase_lists_plan(n_phr, p_max)
    pwork = torch.empty(max(pwb, 1), dtype=torch.uint8, device=DEV)
    n_cons, n_groups, n_base = ops[6].size, ops[1].size, ops[4].size - 1
    t = [dev_arr(a, dt) for a, dt in zip(ops, T_OPS)]
    sp = torch.full((n_cons + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    rw = torch.full((max(rows_cap, 1),), SENTINEL, dtype=torch.int64, device=DEV)
    st = torch.full((n_cons,), SENTINEL, dtype=torch.int32, device=DEV)
    wb = nat.term_scope_plan(n_cons, cand_max)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=DEV)
    gi.phrase_lists_device(tp.data_ptr(), tt.data_ptr(), n_phr, p_max, p_cap, lp.data_ptr(), dc.data_ptr(), pst.data_ptr(),
                           pwork.data_ptr(), pwb, stream_ptr())
    gi.term_scope_device([x.data_ptr() for x in t], n_base, n_cons, n_groups, cand_max, rows_cap, sp.data_ptr(), rw.data_ptr(),
                         st.data_ptr(), work.data_ptr(), wb, stream_ptr(), lists=(lp.data_ptr(), dc.data_ptr(), n_phr))
    torch.cuda.synchronize()
    return (sp.cpu().numpy(), rw.cpu().numpy()[:rows_cap], st.cpu().numpy()), pst.cpu().numpy()


def test_a_phrase_stands_wherever_a_term_id_may_and_upper_bounds_never_overflow(nat, world):
    corpus, gi = world[0]["rand"]
    phrases = PC.scope_phrases(corpus)
    fam = PC.scope_family(corpus, phrases)
    PC.scope_certificates(corpus, fam, phrases)
    ops = TC.operands(fam)
    want_ptr, want_rows = PC.expected_table(corpus, fam, phrases)
    # every bound from the host's upper bounds alone: the smallest document frequency among a phrase's tokens
    ub = PC.upper_bounds(corpus, phrases)
    p_lens, p_max, p_cap = bounds(corpus, phrases)
    lens, cand_max, rows_cap = term_bounds(fam, corpus, ub)
    true_lens = [PC.phrase_list(corpus, p).size for p in phrases]
    assert all(t < u for t, u in zip(true_lens, p_lens)) and lens[0] == p_lens[0] > true_lens[0]
    (sp, rows, status), p_status = run_both_steps_device(nat, gi, phrases, p_max, p_cap, ops, cand_max, rows_cap)
    assert not status.any() and not p_status.any()
    assert np.array_equal(sp, want_ptr) and np.array_equal(rows[:want_ptr[-1]], want_rows)
    assert np.all(rows[want_ptr[-1]:] == SENTINEL)
    # the twins: the lists come back to the host and go into the term step's twin
    lp, docs, p_status = run_twin(gi, phrases, p_max, p_cap)
    sp2, rows2, status2 = gi.term_scope(ops, cand_max, rows_cap, lists=(lp, docs))
    assert not status2.any() and np.array_equal(sp2, want_ptr) and np.array_equal(rows2, want_rows)
    # bounds computed from the TRUE list lengths are tight: they suffice, and a phrase-driven constraint overflows one below
    tight = np.concatenate([corpus.df(), true_lens])
    t_lens, t_max, t_cap = term_bounds(fam, corpus, tight)
    assert t_lens[0] == true_lens[0] and t_cap < rows_cap
    sp3, rows3, status3 = gi.term_scope(ops, t_max, t_cap, lists=(lp, docs))
    assert not status3.any() and np.array_equal(rows3, want_rows)
    alone = TC.operands(TC.Family("the driver", "rand", fam.cons[:1]))
    assert gi.term_scope(alone, true_lens[0], true_lens[0], lists=(lp, docs))[2].tolist() == [0]
    sp4, rows4, status4 = gi.term_scope(alone, true_lens[0] - 1, true_lens[0], lists=(lp, docs))
    assert status4.tolist() == [1] and rows4.size == 0
    # without the lists the same ids name no document: the existing entry points are the n_x = 0 forms
    sp5, rows5, status5 = gi.term_scope(ops, cand_max, rows_cap)
    none = PC.expected_table(corpus, fam, [])
    assert np.array_equal(sp5, none[0]) and np.array_equal(rows5, none[1]) and sp5[1] == 0


# ---- the scoped channels on the device-built table -----------------------------------------------------------------------------
@pytest.fixture(params=[None, "64"], ids=["default-slabs", "slab-64"])
def slab(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("AMDR_SCOPE_SLAB", raising=False)
    else:
        monkeypatch.setenv("AMDR_SCOPE_SLAB", request.param)
    return request.param


@pytest.fixture(scope="module")
def engines(nat, world):
    """corpus name -> the three channels over that corpus's rows (values exact in every arithmetic, as test_scope_gpu's)."""
    from legal_rag_amd.retrieval.engine import HybridEngine
    out = {}
    for name in ("rand", "tiles"):
        rng = np.random.default_rng(33)
        corpus, gi = world[0][name]
        n = corpus.n_docs
        X = (rng.integers(-8, 9, size=(n, 64)) / 8.0).astype(np.float32)
        lens = rng.integers(1, 4, size=n)
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        D = (rng.integers(-8, 9, size=(int(ptr[-1]), 128)) / 8.0).astype(np.float32)
        eng = HybridEngine(nat.DenseIndex(X), gi, nat.MaxSimIndex(D, ptr))
        nq = 70
        Q = torch.from_numpy((rng.integers(-8, 9, size=(nq, 64)) / 8.0).astype(np.float32)).to(DEV)
        Qt = torch.from_numpy((rng.integers(-8, 9, size=(nq, 32, 128)) / 8.0).astype(np.float32)).to(DEV)
        q_terms, q_ptr = nat.BM25Index.pack_queries([[int(t) for t in rng.integers(0, corpus.n_terms, size=5)]
                                                     for _ in range(nq)])
        out[name] = (eng, Q, Qt, torch.from_numpy(q_terms).to(DEV), torch.from_numpy(q_ptr).to(DEV))
    return out


def phrase_table(fam, corpus, phrases, qscope):
    from legal_rag_amd.retrieval.terms import Phrase, TermTable
    lens, cand_max, rows_cap = term_bounds(fam, corpus, PC.upper_bounds(corpus, phrases))
    p_lens, p_max, p_cap = bounds(corpus, phrases)
    ops = TC.operands(fam)
    return TermTable(ops, np.asarray(qscope, np.int32), len(fam.cons), int(ops[1].size), len(fam.bases),
                     np.asarray(lens, np.int64), cand_max, rows_cap, PC.operands(phrases),
                     tuple(Phrase(*[f"t{t}" for t in p]) for p in phrases), p_max, p_cap)


def short_family(corpus):
    """Constraints of at most 256 candidates over the "tiles" corpus: the step of their table is the one launch."""
    V = corpus.n_terms
    return TC.Family("short phrase lists", "tiles", [TC.c([(TC.MUST, [V + 1])]), TC.c([(TC.MUST, [V + 2])]),
                                                      TC.c([(TC.MUST, [V + 3]), (TC.NOT, [V + 2])]),
                                                      TC.c([(TC.MUST, [PC.T_RARE[PC.TILE - 1]]), (TC.ANY, [V + 2]), (TC.ANY, [V + 3])])])


@pytest.mark.parametrize("which, one_launch", [("rand", False), ("tiles", True)], ids=["phrases-in-constraints", "short-lists"])
def test_scoped_channels_on_the_device_built_table_return_the_host_tables_bits(nat, world, engines, slab, which, one_launch):
    eng, Q, Qt, q_terms, q_ptr = engines[which]
    corpus, gi = world[0][which]
    if which == "rand":
        phrases = PC.scope_phrases(corpus)
        fam = PC.scope_family(corpus, phrases)
    else:
        phrases = PC.tiles_phrases()
        fam = short_family(corpus)
    nq, k = int(Q.shape[0]), 10
    eng.scope = None  # a workspace reserved under this test's AMDR_SCOPE_SLAB
    qscope = (np.arange(nq) * 7 % len(fam.cons)).astype(np.int32)
    tt = phrase_table(fam, corpus, phrases, qscope)
    want_ptr, want_rows = PC.expected_table(corpus, fam, phrases)
    if one_launch:
        assert tt.cand_max <= 256 and np.all(np.diff(want_ptr) > 0)
        if slab is None:  # the step of this table is scope_hybrid_kernel's one launch
            assert nat.hybrid_scope_plan(nq, k, k, 0, tt.cand_max, tt.cand_max)[0]
    params = nat.make_fuse_params(min_final_score=0.0)

    def outputs(table):
        got = []
        for s, i in (eng.dense_topk_scoped(Q, k, table), eng.bm25_topk_scoped(q_terms, q_ptr, k, table),
                     eng.colbert_topk_scoped(Qt, k, table)):
            torch.cuda.synchronize()
            got += [s.cpu().numpy().copy(), i.cpu().numpy().copy()]
        for kw in (dict(q_tok=Qt, scopes=(table, table, table)), dict(scopes=(table, table, None))):  # with / without ColBERT
            res = eng.search_batch(params, k, q_emb=Q, q_terms=q_terms, q_ptr=q_ptr, **kw)
            torch.cuda.synchronize()
            got += [t.cpu().numpy().copy() for t in (res.ids, res.vals, res.mask, res.count, res.dense_ids, res.dense_scores,
                                                     res.bm25_ids, res.bm25_scores)]
        return got
    table, status = eng.term_scopes(tt)
    assert table[3] == len(fam.cons) and table[4] == tt.cand_max
    on_device = outputs(table)
    assert status.numel() == len(fam.cons) + len(phrases) and not status.cpu().numpy().any()
    assert np.array_equal(table[0].cpu().numpy(), want_ptr) and np.array_equal(table[1].cpu().numpy()[:want_ptr[-1]], want_rows)
    uploaded = outputs(eng.upload_scopes(want_ptr, want_rows, qscope))
    assert len(on_device) == len(uploaded) == 22
    for a, b in zip(on_device, uploaded):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (on_device[1] >= 0).any() and (on_device[6] >= 0).any()


# ---- capture -----------------------------------------------------------------------------------------------------------------
def test_captured_phrase_and_term_steps_replay_with_the_phrases_rewritten_in_place(nat, world):
    corpus, gi = world[0]["rand"]
    V, n_phr, L = corpus.n_terms, 5, 3
    cand_max, rows_cap = corpus.n_docs, n_phr * corpus.n_docs  # hold for every phrase over this corpus
    fam = TC.Family("each phrase alone", "rand", [TC.c([(TC.MUST, [V + p])]) for p in range(n_phr)])
    ops = TC.operands(fam)
    t = [dev_arr(a, dt) for a, dt in zip(ops, T_OPS)]
    pp = dev_arr(np.arange(0, n_phr * L + 1, L), torch.int64)
    pt = torch.zeros(n_phr * L, dtype=torch.int32, device=DEV)
    lp = torch.zeros(n_phr + 1, dtype=torch.int64, device=DEV)
    dc = torch.zeros(rows_cap, dtype=torch.int32, device=DEV)
    pst = torch.zeros(n_phr, dtype=torch.int32, device=DEV)
    sp = torch.zeros(n_phr + 1, dtype=torch.int64, device=DEV)
    rw = torch.zeros(rows_cap, dtype=torch.int64, device=DEV)
    st = torch.zeros(n_phr, dtype=torch.int32, device=DEV)
    pwb, wb = nat.phrase_lists_plan(n_phr, cand_max), nat.term_scope_plan(n_phr, cand_max)
    pwork = torch.empty(pwb, dtype=torch.uint8, device=DEV)
    work = torch.empty(wb, dtype=torch.uint8, device=DEV)

    def variant(seed):
        r = np.random.default_rng(seed)
        out = []
        while len(out) < n_phr:
            seq = corpus.docs[int(r.integers(0, corpus.n_docs))]
            if len(seq) >= L:
                s = int(r.integers(0, len(seq) - L + 1))
                out.append([int(x) for x in seq[s:s + L]])
        return out

    def step():
        s = stream_ptr()
        gi.phrase_lists_device(pp.data_ptr(), pt.data_ptr(), n_phr, cand_max, rows_cap, lp.data_ptr(), dc.data_ptr(),
                               pst.data_ptr(), pwork.data_ptr(), pwb, s)
        gi.term_scope_device([x.data_ptr() for x in t], 0, n_phr, n_phr, cand_max, rows_cap, sp.data_ptr(), rw.data_ptr(),
                             st.data_ptr(), work.data_ptr(), wb, s, lists=(lp.data_ptr(), dc.data_ptr(), n_phr))

    def write(phrases):
        pt.copy_(torch.from_numpy(np.asarray([x for p in phrases for x in p], np.int32)))

    def snapshot():
        torch.cuda.synchronize()
        return [x.cpu().numpy().copy() for x in (lp, dc, pst, sp, rw, st)]
    write(variant(1))
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
        phrases = variant(seed)
        write(phrases)
        graph.replay()
        got = snapshot()
        assert nat.workspace_growths() == g0
        want_ptr, want_docs = PC.expected_lists(corpus, phrases)
        assert want_ptr[-1] > 0
        assert np.array_equal(got[0], want_ptr) and np.array_equal(got[1][:want_ptr[-1]], want_docs) and not got[2].any()
        assert np.array_equal(got[3], want_ptr) and np.array_equal(got[4][:want_ptr[-1]], want_docs) and not got[5].any()
        step()  # the uncaptured call on the same operands
        exp = snapshot()
        for a, b, used in zip(got, exp, (None, want_ptr[-1], None, None, want_ptr[-1], None)):
            assert np.array_equal(a[:used], b[:used])

"""Proximity constraints resolved on the GPU (amdr_span_lists: csrc/phrase_scope.hip, csrc/near_rule.hpp) and read by the
term step as virtual posting lists: the device lists and the host twin's equal the reference of tests/near_cases.py exactly
— a plain scan of every window of every document — at the smallest shapes where the kernels can go wrong; the status words
at both bounds; argument errors and refusals; phrases through the mixed entry against amdr_phrase_lists; capture of the span
step and the term step behind it; a Near wherever a term id may stand in a constraint; the stream's life across updates;
the scoped channels on the device-built table against the host-uploaded one."""
import numpy as np
import pytest
import torch

import near_cases as NC
import phrase_cases as PC
import term_scope_cases as TC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = -77
T_OPS = (torch.int64, torch.int32, torch.int64, torch.int32, torch.int64, torch.int64, torch.int32)
S_OPS = (torch.int64, torch.int32, torch.int32, torch.int32)


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
    """name -> (corpus, its BM25Index with the token stream resident).  The references are computed once per corpus object
    (near_cases.item_list keeps them, read-only)."""
    edge, at = NC.edge_corpus()
    out = {"edge": edge, "tiles": PC.tiles_corpus(), "rand": PC.rand_corpus()}
    return {name: (c, make_index(nat, c)) for name, c in out.items()}, at


def dev_arr(a, dtype):
    t = torch.zeros(max(int(np.size(a)), 1), dtype=dtype, device=DEV)
    if np.size(a):
        t[:np.size(a)].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def run_device(nat, gi, items, cand_max, rows_cap):
    """amdr_span_lists_device on fresh tensors: (list_ptr, docs [rows_cap], status) as numpy arrays; what the call does not
    write keeps SENTINEL."""
    n = len(items)
    ops = [dev_arr(a, dt) for a, dt in zip(NC.operands(items), S_OPS)]
    lp = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    dc = torch.full((max(rows_cap, 1),), SENTINEL, dtype=torch.int32, device=DEV)
    st = torch.full((max(n, 1),), SENTINEL, dtype=torch.int32, device=DEV)
    wb = nat.span_lists_plan(n, cand_max)
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device=DEV)
    gi.span_lists_device(*[x.data_ptr() for x in ops], n, cand_max, rows_cap, lp.data_ptr(), dc.data_ptr(), st.data_ptr(),
                         work.data_ptr(), wb, stream_ptr())
    torch.cuda.synchronize()
    return lp.cpu().numpy(), dc.cpu().numpy()[:rows_cap], st.cpu().numpy()[:n]


def run_twin(gi, items, cand_max, rows_cap):
    return gi.span_lists(*NC.operands(items), cand_max, rows_cap)


def assert_lists(got, want_ptr, want_docs, device_cap=None):
    lp, docs, status = got
    assert np.array_equal(lp, want_ptr), (lp, want_ptr)
    assert docs.dtype == np.int32 and np.array_equal(docs[:want_ptr[-1]], want_docs)
    assert not status.any(), status
    if device_cap is not None:  # nothing is written past the lists
        assert np.all(docs[want_ptr[-1]:] == SENTINEL)


def check_both(nat, corpus, gi, items, alone=False):
    want_ptr, want_docs = NC.expected_lists(corpus, items)
    cand_max, rows_cap = NC.bounds(corpus, items)
    assert_lists(run_device(nat, gi, items, cand_max, rows_cap), want_ptr, want_docs, rows_cap)
    assert_lists(run_twin(gi, items, cand_max, rows_cap), want_ptr, want_docs)
    # bounds larger than needed (another tile count) and a rows_cap of exactly the lists change nothing
    assert_lists(run_device(nat, gi, items, cand_max + 700, int(want_ptr[-1])), want_ptr, want_docs)
    for p in range(len(items)):
        assert np.all(np.diff(want_docs[want_ptr[p]:want_ptr[p + 1]]) > 0)
    return want_ptr, want_docs


# ---- the lists ---------------------------------------------------------------------------------------------------------------
def test_edge_shapes_distances_boundaries_multiplicity_and_the_lane_stride(nat, world):
    (corpus, gi), at = world[0]["edge"], world[1]
    NC.edge_certificates(corpus, at)
    items = NC.edge_items()
    want_ptr, want_docs = check_both(nat, corpus, gi, items)
    got = run_device(nat, gi, items, *NC.bounds(corpus, items))
    lists = {(it[0], tuple(it[1]), it[2]): set(got[1][got[0][i]:got[0][i + 1]].tolist()) for i, it in enumerate(items)}
    L = lambda terms, n, o=False: lists[(NC.ORDERED if o else NC.UNORDERED, tuple(terms), n)]  # noqa: E731
    A, B, Y, Z = NC.A, NC.B, NC.Y, NC.Z
    for n in NC.DISTANCES:  # exactly n apart is a hit, n + 1 apart a miss, in both forms
        hits = {at[f"y z {g} apart"] for g in NC.GAPS if g <= n}
        assert L([Y, Z], n) == hits == L([Y, Z], n, True) and L([Z, Y], n, True) == set()
    assert not L([A, B], 5) & {at["boundary left"], at["boundary right"], at["empty"], at["one a"]}
    assert {0, corpus.n_docs - 1, at["clamped at the end"], at["b x a"], at["a x x b a"]} <= L([A, B], 5)
    assert at["b x a"] not in L([A, B], 5, True) and corpus.n_docs - 1 not in L([A, B], 5, True) and 0 in L([A, B], 5, True)
    assert at["a a b"] in L([A, B], 1, True) and at["a x x b a"] in L([A, B], 1) and at["a x x b a"] not in L([A, B], 1, True)
    assert at["one a"] not in L([A, A], 3) and at["a x a"] in L([A, A], 2) and at["a x x a"] not in L([A, A], 2)
    assert at["a x x a"] in L([A, A], 3) and at["a b a"] in L([A, A, B], 2) and at["a x b x a"] not in L([A, A, B], 3)
    assert at["a x b x a"] in L([A, A, B], 4) and 0 not in L([A, A, B], 4)
    assert L([NC.C_] * 8, 7) == {at["eight c"]} == L([NC.C_] * 8, 7, True) and L([NC.C_] * 8, 6) == set()
    assert L([NC.C_] * 8, 8) == {at["eight c"], at["four c x four c"]}
    assert L(NC.E8, 7) == {at["eight distinct, reversed"]} == L(NC.E8[::-1], 7, True) and L(NC.E8, 7, True) == set()
    assert L(NC.E8, 8, True) == {at["eight distinct, one gap"]}
    assert at["a b a"] in L([A, B, A], 2, True) and at["a a b"] not in L([A, B, A], 3, True)
    for n in (1, NC.STRIDE_N, NC.STRIDE_N + 1, 64, 128, 255):
        assert L([NC.P_, NC.Q_], n) == {at[f"stride len {ln} p {p} q {q}"] for ln, p, q in NC.STRIDE_DOCS if abs(q - p) <= n}
        assert L([NC.P_, NC.Q_], n, True) == {at[f"stride len {ln} p {p} q {q}"] for ln, p, q in NC.STRIDE_DOCS if 0 < q - p <= n}
    assert L([NC.U, NC.V], 5) == {at["long"]} == L([NC.U, NC.V], 3, True) and L([NC.U, NC.V], 2) == set()
    assert L([NC.U, NC.V], 255) == {at["long"], at["long none"]} and L([NC.V, NC.U], 255, True) == set()
    for it in items[::7]:  # alone: another grid, the same list
        check_both(nat, corpus, gi, [it])


def test_driver_lengths_around_the_tile_and_documents_0_and_n_minus_1(nat, world):
    corpus, gi = world[0]["tiles"]
    NC.tiles_certificates(corpus)
    items = NC.tiles_items()
    assert [NC.driver_len(corpus, it) for it in items] == list(NC.DRIVER_LENGTHS) * 2
    want_ptr, want_docs = check_both(nat, corpus, gi, items)
    last = want_docs[want_ptr[-2]:want_ptr[-1]]
    assert last[0] == 0 and last[-1] == corpus.n_docs - 1
    for it in items:  # alone: cand_max is the item's own driver length (0 tiles of work, 1 tile, 2 tiles, 3 tiles)
        check_both(nat, corpus, gi, [it])


@pytest.mark.parametrize("count", [1, 2, 65])
def test_one_two_and_65_items_nears_mixed_with_phrases(nat, world, count):
    corpus, gi = world[0]["rand"]
    items = NC.rand_items(corpus)
    if count == 65:
        NC.rand_certificates(corpus, items)
    picked = items[:count] if count != 2 else [items[0], items[1]]
    assert count == 1 or {it[0] for it in picked} >= {NC.PHRASE, NC.ORDERED}
    check_both(nat, corpus, gi, picked)


def test_the_two_identities(nat, world):
    corpus, gi = world[0]["rand"]
    terms = NC.identity_terms(corpus)
    wide = [NC.near(t, NC.MAX_DIST) for t in terms]          # n >= the longest document: the conjunction
    tight = [NC.near(t, 1, True) for t in terms if len(t) == 2]  # distance 1, ordered: the phrase
    lp, docs, status = run_device(nat, gi, wide + tight, *NC.bounds(corpus, wide + tight))
    assert not status.any()
    for i, t in enumerate(terms):
        assert np.array_equal(docs[lp[i]:lp[i + 1]], PC.conjunction(corpus, t)), t
    for j, it in enumerate(tight):
        i = len(wide) + j
        assert np.array_equal(docs[lp[i]:lp[i + 1]], PC.phrase_list(corpus, it[1])), it


def test_phrases_through_the_mixed_entry_are_amdr_phrase_lists(nat, world):
    for name in ("edge", "rand"):
        corpus, gi = world[0][name]
        phrases = ([[NC.A, NC.B], [NC.A, NC.A], [NC.A, NC.B, NC.A], [NC.B, NC.X, NC.A], [-1, NC.A]] if name == "edge"
                   else PC.rand_phrases(corpus)[:20])
        lens = [PC.driver_len(corpus, p) for p in phrases]
        old = gi.phrase_lists(*PC.operands(phrases), max(lens), sum(lens))
        items = [NC.phrase(p) for p in phrases]
        for new in (run_twin(gi, items, max(lens), sum(lens)), run_device(nat, gi, items, max(lens), sum(lens))):
            assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1][:old[0][-1]]) and np.array_equal(old[2], new[2])
        want_ptr, want_docs = PC.expected_lists(corpus, phrases)
        assert np.array_equal(old[0], want_ptr) and np.array_equal(old[1], want_docs)


def test_an_id_outside_the_vocabulary_and_sizes_outside_the_rule_give_empty_lists(nat, world):
    corpus, gi = world[0]["edge"]
    A, B = NC.A, NC.B
    good = NC.near([A, B], 2)
    items = [good]
    for j in range(3):
        for bad in (-1, corpus.n_terms, 2**31 - 1):
            for o in (False, True):
                t = [A, B, A]
                t[j] = bad
                items.append(NC.near(t, 3, o))
    want_ptr, _ = check_both(nat, corpus, gi, items)
    assert want_ptr[1] > 0 and want_ptr[-1] == want_ptr[1]
    size = NC.item_list(corpus, good).size
    # what the rule does not define gives an empty list from the device call; the twin refuses it in words
    odd = [((NC.UNORDERED, [A], 2), "fewer than 2 or more than 8"), ((NC.ORDERED, [A] * 9, 2), "fewer than 2 or more than 8"),
           ((NC.UNORDERED, [A, B], 0), "distance outside 1 .. 255"), ((NC.ORDERED, [A, B], 256), "distance outside 1 .. 255"),
           ((NC.UNORDERED, [A, B], -1), "distance outside 1 .. 255"), ((3, [A, B], 2), "kind outside 0 .. 2"),
           ((-1, [A, B], 2), "kind outside 0 .. 2"), ((NC.PHRASE, [A], 0), "fewer than 2 or more than 16"),
           ((NC.PHRASE, [A] * 17, 0), "fewer than 2 or more than 16")]
    for it, words in odd:
        lp, docs, status = run_device(nat, gi, [it, good], 100, 100)
        assert lp.tolist() == [0, 0, size] and not status.any(), it
        with pytest.raises(nat.NativeError, match=words):
            run_twin(gi, [it, good], 100, 100)
    assert run_twin(gi, [(NC.PHRASE, [A] * 9, -5), good], 100, 100)[0].tolist() == [0, 0, size]  # a phrase's dist is not read


# ---- the status words --------------------------------------------------------------------------------------------------------
def test_cand_max_one_below_the_longest_driver_sets_status_1_for_those_items_alone(nat, world):
    corpus, gi = world[0]["tiles"]
    items = NC.tiles_items()
    lens = [NC.driver_len(corpus, it) for it in items]
    cand_max, rows_cap = NC.bounds(corpus, items)
    over = [p for p, n in enumerate(lens) if n == cand_max]
    assert len(over) == 2
    lists = [NC.item_list(corpus, it) if p not in over else np.zeros(0, np.int32) for p, it in enumerate(items)]
    want_ptr = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.int64)
    want_docs = np.concatenate(lists)
    for lp, docs, status in (run_device(nat, gi, items, cand_max - 1, rows_cap), run_twin(gi, items, cand_max - 1, rows_cap)):
        assert status.tolist() == [1 if p in over else 0 for p in range(len(items))]
        assert np.array_equal(lp, want_ptr) and np.array_equal(docs[:want_ptr[-1]], want_docs)


def test_rows_cap_one_below_the_total_sets_status_2_from_the_first_item_that_does_not_fit(nat, world):
    corpus, gi = world[0]["tiles"]
    items = NC.tiles_items()
    cand_max, _ = NC.bounds(corpus, items)
    want_ptr, want_docs = NC.expected_lists(corpus, items)
    total = int(want_ptr[-1])
    for cap in (total - 1, int(want_ptr[-2]) - 1):  # the last item alone loses a document; the last two are cut
        first = int(np.searchsorted(want_ptr[1:], cap, side="right"))
        for lp, docs, status in (run_device(nat, gi, items, cand_max, cap), run_twin(gi, items, cand_max, cap)):
            assert status.tolist() == [2 if p >= first and want_ptr[p + 1] > want_ptr[p] else 0 for p in range(len(items))]
            assert np.array_equal(lp, np.minimum(want_ptr, cap)) and np.array_equal(docs[:cap], want_docs[:cap])


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing_and_leave_the_outputs_untouched(nat, world):
    corpus, gi = world[0]["tiles"]
    items = NC.tiles_items()
    cand_max, rows_cap = NC.bounds(corpus, items)
    n = len(items)
    ops = [dev_arr(a, dt) for a, dt in zip(NC.operands(items), S_OPS)]
    lp = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    dc = torch.full((rows_cap,), SENTINEL, dtype=torch.int32, device=DEV)
    st = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    wb = nat.span_lists_plan(n, cand_max)
    work = torch.empty(wb, dtype=torch.uint8, device=DEV)
    good = dict(ip=ops[0].data_ptr(), it=ops[1].data_ptr(), ik=ops[2].data_ptr(), id=ops[3].data_ptr(), n=n, cand_max=cand_max,
                rows_cap=rows_cap, lp=lp.data_ptr(), dc=dc.data_ptr(), st=st.data_ptr(), work=work.data_ptr(), wb=wb)

    def call(index=gi, **over):
        a = dict(good, **over)
        index.span_lists_device(a["ip"], a["it"], a["ik"], a["id"], a["n"], a["cand_max"], a["rows_cap"], a["lp"], a["dc"],
                                a["st"], a["work"], a["wb"], stream_ptr())
    for over in (dict(n=-1), dict(cand_max=-1), dict(rows_cap=-1), dict(wb=-1), dict(wb=wb - 1), dict(work=0), dict(lp=0),
                 dict(dc=0), dict(st=0), dict(ip=0), dict(it=0), dict(ik=0), dict(id=0), dict(cand_max=65_536 * NC.TILE)):
        with pytest.raises(nat.NativeError):
            call(**over)
    bare = make_index(nat, corpus, stream=False)  # no resident stream: refused in the words amdr_phrase_lists uses
    for refused in (lambda: call(index=bare), lambda: run_twin(bare, items, cand_max, rows_cap)):
        with pytest.raises(nat.NativeError, match=r"no token stream is resident \(amdr_bm25_set_tokens; an update drops it\)"):
            refused()
    torch.cuda.synchronize()
    assert (lp == SENTINEL).all() and (dc == SENTINEL).all() and (st == SENTINEL).all()
    call()  # the same buffers with the arguments as they should be
    torch.cuda.synchronize()
    want_ptr, want_docs = NC.expected_lists(corpus, items)
    assert np.array_equal(lp.cpu().numpy(), want_ptr) and np.array_equal(dc.cpu().numpy()[:want_ptr[-1]], want_docs)
    z = np.zeros(19, np.int32)
    for bad_ptr in ([1, 2, 4], [0, 4, 2]):  # the twin validates the pointer array
        with pytest.raises(nat.NativeError, match="item_ptr"):
            gi.span_lists(np.asarray(bad_ptr, np.int64), z, np.ones(2, np.int32), np.ones(2, np.int32), cand_max, rows_cap)
    with pytest.raises(ValueError):
        gi.span_lists(np.asarray([0, 2, 4], np.int64), z, np.ones(1, np.int32), np.ones(2, np.int32), cand_max, rows_cap)
    lp0, docs0, st0 = gi.span_lists(np.zeros(1, np.int64), z[:0], z[:0], z[:0], 0, 0)  # no item: an empty table
    assert lp0.tolist() == [0] and docs0.size == 0 and st0.size == 0


# ---- the token stream across updates -----------------------------------------------------------------------------------------
def test_every_update_drops_the_stream_and_a_near_needs_it_made_again(nat):
    corpus = PC.SeqCorpus("small", 4, [[0, 1, 2], [1, 3, 0], [], [2, 2, 0, 3, 1], [3, 0, 1], [1]])
    V = corpus.n_terms
    idf = np.linspace(0.5, 3.0, V)
    one = PC.SeqCorpus("one", V, [[1, 2, 0]])
    a_ptr, a_doc, a_tf, _, a_len, _ = one.postings()
    item = NC.near([0, 1], 2)

    def gone(gi, after):
        assert gi.tokens_info() == (False, 0)
        with pytest.raises(nat.NativeError, match="no token stream"):
            run_twin(gi, [item], 8, 8)
        gi.set_tokens(*after.stream())
        assert run_twin(gi, [item], 8, 8)[1].tolist() == NC.item_list(after, item).tolist()
    gi = make_index(nat, corpus)
    assert run_twin(gi, [item], 8, 8)[1].tolist() == [0, 1, 3, 4]
    gi.add(a_ptr, a_doc, a_tf, idf, a_len, 2.0)
    gone(gi, PC.SeqCorpus("added", V, corpus.docs + one.docs))
    gi = make_index(nat, corpus)
    gi.remove(np.asarray([3], np.int64), idf, 2.0)
    gone(gi, PC.SeqCorpus("removed", V, corpus.docs[:3] + corpus.docs[4:]))
    gi = make_index(nat, corpus)
    gi.replace(np.asarray([5], np.int64), a_ptr, a_doc, a_tf, a_len, idf, 2.0)
    after = PC.SeqCorpus("replaced", V, corpus.docs[:5] + one.docs)
    assert NC.item_list(after, item).tolist() == [0, 1, 3, 4, 5]
    gone(gi, after)


# ---- through the term step ---------------------------------------------------------------------------------------------------
def term_bounds(fam, corpus, ub):
    from legal_rag_amd.retrieval.terms import driver_length
    lens = [driver_length(g, ub, None if b < 0 else int(fam.bases[b].size), corpus.n_docs) for g, b in fam.cons]
    return lens, max(lens), sum(lens)


def test_a_near_stands_wherever_a_term_id_may_and_upper_bounds_never_overflow(nat, world):
    """MUST and driver, MUST beside a rarer plain term, two items as MUST, ANY, NOT, inside a tuple group, an id past the
    lists, and inside a base scope — against set algebra over the window scan."""
    corpus, gi = world[0]["rand"]
    items = NC.scope_items(corpus)
    fam = NC.scope_family(corpus)
    NC.scope_certificates(corpus, fam, items)
    ops = TC.operands(fam)
    want_ptr, want_rows = NC.expected_table(corpus, fam, items)
    lens, cand_max, rows_cap = term_bounds(fam, corpus, NC.upper_bounds(corpus, items))
    p_max, p_cap = NC.bounds(corpus, items)
    lp, docs, p_status = run_twin(gi, items, p_max, p_cap)
    assert not p_status.any() and all(lp[i + 1] - lp[i] < NC.driver_len(corpus, it) for i, it in enumerate(items))
    sp, rows, status = gi.term_scope(ops, cand_max, rows_cap, lists=(lp, docs))
    assert not status.any() and np.array_equal(sp, want_ptr) and np.array_equal(rows, want_rows)
    # the same through the engine: one span step in front of the term step on one stream, the operands in one staging copy
    from legal_rag_amd.retrieval.engine import HybridEngine
    from legal_rag_amd.retrieval.terms import Near, Phrase, TermTable
    name = lambda it: (Phrase(*[f"t{t}" for t in it[1]]) if it[0] == NC.PHRASE  # noqa: E731
                       else Near(*[f"t{t}" for t in it[1]], distance=it[2], ordered=it[0] == NC.ORDERED))
    # the packer's order: the phrases first as kind 0, then the Nears — so the family's virtual ids are renumbered
    order = [i for i, it in enumerate(items) if it[0] == NC.PHRASE] + [i for i, it in enumerate(items) if it[0] != NC.PHRASE]
    new_id = {corpus.n_terms + old: corpus.n_terms + new for new, old in enumerate(order)}
    fam2 = TC.Family(fam.name, fam.corpus, [([(k, [new_id.get(t, t) for t in ids]) for k, ids in g], b) for g, b in fam.cons],
                     fam.bases)
    packed = [items[i] for i in order]
    phr = [it for it in packed if it[0] == NC.PHRASE]
    nears = [it for it in packed if it[0] != NC.PHRASE]
    qscope = np.arange(len(fam.cons), dtype=np.int32)
    ops2 = TC.operands(fam2)
    tt = TermTable(ops2, qscope, len(fam.cons), int(ops2[1].size), len(fam.bases), np.asarray(lens, np.int64), cand_max, rows_cap,
                   PC.operands([it[1] for it in phr]), tuple(name(it) for it in phr), *NC.bounds(corpus, phr),
                   NC.operands(packed), tuple(name(it) for it in nears), *NC.bounds(corpus, nears))
    eng = HybridEngine(None, gi, None)
    table, st = eng.term_scopes(tt)
    torch.cuda.synchronize()
    assert st.numel() == len(fam.cons) + len(items) and not st.cpu().numpy().any()
    assert np.array_equal(table[0].cpu().numpy(), want_ptr) and np.array_equal(table[1].cpu().numpy()[:want_ptr[-1]], want_rows)
    # an overflow of the span step's bound lands behind the constraints' words, at the item's place
    small = TermTable(ops2, qscope, len(fam.cons), int(ops2[1].size), len(fam.bases), np.asarray(lens, np.int64), cand_max, rows_cap,
                      tt.phr_ops, tt.phrases, tt.phr_cand_max, tt.phr_rows_cap, tt.span_ops, tt.nears,
                      tt.near_cand_max, int(lp[-1]) - 1 - tt.phr_rows_cap)
    _, st2 = eng.term_scopes(small)
    torch.cuda.synchronize()
    assert st2.cpu().numpy()[len(fam.cons):].tolist()[-1] == 2


# ---- the scoped channels on the device-built table -----------------------------------------------------------------------------
@pytest.mark.parametrize("which, one_launch", [("rand", False), ("tiles", True)], ids=["nears-in-constraints", "short-lists"])
def test_scoped_channels_over_a_nears_rows_return_the_uploaded_tables_bits(nat, world, which, one_launch):
    """Dense, BM25, ColBERT and the hybrid step (its one launch for the short lists) over the device-built table of Near
    constraints: the bits of the same searches over the host-uploaded rows of the window scan."""
    from legal_rag_amd.retrieval.engine import HybridEngine
    from legal_rag_amd.retrieval.terms import Near, TermTable
    corpus, gi = world[0][which]
    rng = np.random.default_rng(33)
    n = corpus.n_docs
    X = (rng.integers(-8, 9, size=(n, 64)) / 8.0).astype(np.float32)
    ptr = np.concatenate([[0], np.cumsum(rng.integers(1, 4, size=n))]).astype(np.int64)
    D = (rng.integers(-8, 9, size=(int(ptr[-1]), 128)) / 8.0).astype(np.float32)
    eng = HybridEngine(nat.DenseIndex(X), gi, nat.MaxSimIndex(D, ptr))
    nq, k = 24, 10
    Q = torch.from_numpy((rng.integers(-8, 9, size=(nq, 64)) / 8.0).astype(np.float32)).to(DEV)
    Qt = torch.from_numpy((rng.integers(-8, 9, size=(nq, 32, 128)) / 8.0).astype(np.float32)).to(DEV)
    qt, qp = nat.BM25Index.pack_queries([[int(t) for t in rng.integers(0, corpus.n_terms, size=5)] for _ in range(nq)])
    q_terms, q_ptr = torch.from_numpy(qt).to(DEV), torch.from_numpy(qp).to(DEV)
    V = corpus.n_terms
    if which == "rand":
        items = [it for it in NC.scope_items(corpus) if it[0] != NC.PHRASE]
        cons = [TC.c([(TC.MUST, [V + 0])]), TC.c([(TC.MUST, [V + 1]), (TC.NOT, [V + 0])]), TC.c([(TC.ANY, [V + 0]), (TC.ANY, [V + 1])])]
    else:
        items = NC.tiles_items()[1:4]  # drivers of 1, 255 and 256 candidates
        cons = [TC.c([(TC.MUST, [V + j])]) for j in range(3)] + [TC.c([(TC.MUST, [V + 2]), (TC.NOT, [V + 1])])]
    fam = TC.Family("nears", which, cons)
    ops = TC.operands(fam)
    lens, cand_max, rows_cap = term_bounds(fam, corpus, NC.upper_bounds(corpus, items))
    qscope = (np.arange(nq) * 7 % len(cons)).astype(np.int32)
    nears = tuple(Near(*[f"t{t}" for t in it[1]], distance=it[2], ordered=it[0] == NC.ORDERED) for it in items)
    tt = TermTable(ops, qscope, len(cons), int(ops[1].size), 0, np.asarray(lens, np.int64), cand_max, rows_cap,
                   span_ops=NC.operands(items), nears=nears, near_cand_max=NC.bounds(corpus, items)[0],
                   near_rows_cap=NC.bounds(corpus, items)[1])
    want_ptr, want_rows = NC.expected_table(corpus, fam, items)
    assert np.all(np.diff(want_ptr) > 0)
    if one_launch:
        assert tt.cand_max <= 256 and nat.hybrid_scope_plan(nq, k, k, 0, tt.cand_max, tt.cand_max)[0]
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
    on_device = outputs(table)
    assert status.numel() == len(cons) + len(items) and not status.cpu().numpy().any()
    assert np.array_equal(table[0].cpu().numpy(), want_ptr) and np.array_equal(table[1].cpu().numpy()[:want_ptr[-1]], want_rows)
    uploaded = outputs(eng.upload_scopes(want_ptr, want_rows, qscope))
    assert len(on_device) == len(uploaded) == 22
    for a, b in zip(on_device, uploaded):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (on_device[1] >= 0).any() and (on_device[6] >= 0).any()


# ---- capture -----------------------------------------------------------------------------------------------------------------
def test_captured_span_and_term_steps_replay_with_the_items_rewritten_in_place(nat, world):
    """One linear chain on one stream: the span step's three launches, then the term step's."""
    corpus, gi = world[0]["rand"]
    V, n, M = corpus.n_terms, 6, 3
    cand_max, rows_cap = corpus.n_docs, n * corpus.n_docs  # hold for every item over this corpus
    fam = TC.Family("each item alone", "rand", [TC.c([(TC.MUST, [V + p])]) for p in range(n)])
    t = [dev_arr(a, dt) for a, dt in zip(TC.operands(fam), T_OPS)]
    ip = dev_arr(np.arange(0, n * M + 1, M), torch.int64)
    it_, ik, id_ = (torch.zeros(n * M if j == 0 else n, dtype=torch.int32, device=DEV) for j in range(3))
    lp = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    dc = torch.zeros(rows_cap, dtype=torch.int32, device=DEV)
    pst = torch.zeros(n, dtype=torch.int32, device=DEV)
    sp = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    rw = torch.zeros(rows_cap, dtype=torch.int64, device=DEV)
    st = torch.zeros(n, dtype=torch.int32, device=DEV)
    pwb, wb = nat.span_lists_plan(n, cand_max), nat.term_scope_plan(n, cand_max)
    pwork = torch.empty(pwb, dtype=torch.uint8, device=DEV)
    work = torch.empty(wb, dtype=torch.uint8, device=DEV)

    def variant(seed):
        r = np.random.default_rng(seed)
        out = []
        while len(out) < n:
            seq = corpus.docs[int(r.integers(0, corpus.n_docs))]
            if len(seq) >= M + 2:
                s = int(r.integers(0, len(seq) - M - 1))
                terms = [int(seq[s]), int(seq[s + 2]), int(seq[s + M + 1])]
                kind = len(out) % 3  # a phrase, a Near unordered, a Near ordered, and again
                out.append((kind, terms[::-1] if kind == NC.UNORDERED else terms, 0 if kind == NC.PHRASE else int(r.integers(2, 9))))
        return out

    def step():
        s = stream_ptr()
        gi.span_lists_device(ip.data_ptr(), it_.data_ptr(), ik.data_ptr(), id_.data_ptr(), n, cand_max, rows_cap, lp.data_ptr(),
                             dc.data_ptr(), pst.data_ptr(), pwork.data_ptr(), pwb, s)
        gi.term_scope_device([x.data_ptr() for x in t], 0, n, n, cand_max, rows_cap, sp.data_ptr(), rw.data_ptr(),
                             st.data_ptr(), work.data_ptr(), wb, s, lists=(lp.data_ptr(), dc.data_ptr(), n))

    def write(items):
        _, terms, kind, dist = NC.operands(items)
        it_.copy_(torch.from_numpy(terms)), ik.copy_(torch.from_numpy(kind)), id_.copy_(torch.from_numpy(dist))

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
        items = variant(seed)
        write(items)
        graph.replay()
        got = snapshot()
        assert nat.workspace_growths() == g0
        want_ptr, want_docs = NC.expected_lists(corpus, items)
        assert want_ptr[-1] > 0
        assert np.array_equal(got[0], want_ptr) and np.array_equal(got[1][:want_ptr[-1]], want_docs) and not got[2].any()
        assert np.array_equal(got[3], want_ptr) and np.array_equal(got[4][:want_ptr[-1]], want_docs) and not got[5].any()

"""Mixed constraint expressions end to end on the GPU: Terms -> pack() -> HybridEngine.term_scopes -> the scope table, equal
to the plain evaluator of tests/query_fuzz_cases.py row for row, with every status word 0 — three seeded batches of a hundred
expressions over all seven member kinds; the sixteen combinations of list steps on one engine, large and small tables in
turn; base scopes around the tile; calls enqueued back to back; an index edited three times with the token stream carried;
and one consumer on the device-built table.  The certificates that these inputs tell a subtly wrong resolver from a right
one are the CPU test's (tests/test_query_fuzz.py)."""
import numpy as np
import pytest
import torch

import query_fuzz_cases as Q

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


@pytest.fixture(scope="module")
def gi(nat):
    corpus = Q.world()[0]
    tp, pd, pt, idf, dl, avgdl = corpus.postings()
    g = nat.BM25Index(tp, pd, pt, idf, dl, avgdl)
    g.set_tokens(*corpus.stream())
    return g


@pytest.fixture(scope="module")
def eng(gi):
    from legal_rag_amd.retrieval.engine import HybridEngine
    return HybridEngine(None, gi, None)


@pytest.fixture(scope="module")
def ev():
    return Q.base_evaluator()


def snapshot(table, status):
    """Clones of a call's outputs, enqueued on the current stream."""
    return tuple(t.clone() for t in table[:3]) + (status.clone(),)


def lists_of(engine, tt):
    """The list array the list steps of the engine's last term_scopes call wrote: (list_ptr i64 [n_x + 1], docs i32)."""
    n_x = tt.n_phr + tt.n_near + tt.n_union + tt.n_cspan
    raw = engine._bufs[("grow", "pho")].cpu().numpy()
    ptr = raw[:8 * (n_x + 1)].view(np.int64)
    return ptr, raw[8 * (n_x + 1):8 * (n_x + 1) + 4 * int(ptr[-1])].view(np.int32)


def check(tt, got, want, ev, lists=None):
    """got: (scope_ptr, rows, qscope, status) as tensors; want: query_fuzz_cases.expected_table.  lists: the list array."""
    want_ptr, want_rows, want_qscope, cons = want
    ptr, rows, qscope, status = (t.cpu().numpy() for t in got)
    n_x = tt.n_phr + tt.n_near + tt.n_union + tt.n_cspan
    assert status.dtype == np.int32 and status.size == tt.n_cons + n_x and not status.any(), status
    if lists is not None:  # the steps' lists first: a wrong list names its item
        lp, docs = lists
        for i in range(n_x):
            one = ev.rows(tt.list_item(i))
            assert lp[i + 1] - lp[i] == one.size and np.array_equal(docs[lp[i]:lp[i + 1]], one), (i, tt.list_item(i))
    assert ptr.dtype == np.int64 and rows.dtype == np.int64 and qscope.dtype == np.int32
    ok = np.array_equal(ptr, want_ptr) and np.array_equal(rows[:want_ptr[-1]], want_rows)
    assert ok, Q.explain(cons, ev, want_ptr, want_rows, ptr, rows)
    assert np.array_equal(qscope, want_qscope) and np.array_equal(qscope, tt.qscope)


def run(engine, pairs, ev, base_rows=None, lists=False):
    tt = Q.pack_base(pairs, base_rows)
    want = Q.expected_table(pairs, ev, base_rows)
    table, status = engine.term_scopes(tt)
    torch.cuda.synchronize()
    assert table[3] == tt.n_cons and table[4] == tt.cand_max
    check(tt, table[:3] + (status,), want, ev, lists_of(engine, tt) if lists else None)
    return tt, table, want


# ---- a: the batches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", Q.BATCH_SEEDS)
def test_a_batch_of_mixed_expressions_is_the_evaluators_table(eng, ev, seed):
    kept = Q.random_batch(seed)[0]
    pairs = [(None, t) for t in kept]
    try:
        tt, _, _ = run(eng, pairs, ev, lists=True)
    except AssertionError as err:  # the smallest expression of the batch that still differs, on its own
        def fails(t):
            try:
                run(eng, [(None, t)], ev)
            except AssertionError:
                return True
            return False
        bad = [t for t in kept if fails(t)]
        raise AssertionError(f"{err}\nsmallest failing expression: {Q.shrink(bad[0], fails)!r}" if bad else
                             f"{err}\n(every expression passes on its own: the batch's numbering is at fault)") from err
    assert tt.n_cons == len(kept) and min(tt.n_phr, tt.n_near, tt.n_union, tt.n_cspan) >= 20


# ---- b: every step combination on one engine ------------------------------------------------------------------------------------
def test_the_sixteen_step_combinations_on_one_engine_with_large_and_small_tables_in_turn(gi, ev):
    from legal_rag_amd.retrieval.engine import HybridEngine
    engine = HybridEngine(None, gi, None)  # its buffers grow from nothing, then serve tables of changing sizes
    seen = set()
    for name, subset, terms in Q.directed_tables():
        tt, _, _ = run(engine, [(None, t) for t in terms], ev, lists=bool(subset))
        assert Q.steps_of(tt) == subset, name
        seen.add(subset)
    assert len(seen) == 16


# ---- c: base scopes -------------------------------------------------------------------------------------------------------------
def test_base_scopes_of_0_1_255_256_257_and_every_document_drive_or_are_driven(eng, ev):
    pairs = Q.scoped_pairs()
    tt, _, want = run(eng, pairs, ev, Q.rows_of_scope)
    assert tt.n_base == len(Q.BASE_SIZES) and tt.n_cons == len(pairs)
    sizes = np.diff(want[0])
    assert (sizes > 0).sum() >= len(pairs) // 3 and sizes.max() > Q.TILE


# ---- d: back-to-back calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("calls", [2, 3])
def test_calls_enqueued_back_to_back_keep_their_operands_and_hand_over_their_outputs(eng, ev, calls):
    """Operands hold until two more term_scopes calls, outputs until the next: each call's table is cloned on the stream
    before the next call is enqueued, and nothing synchronises until the last is in."""
    work = []
    for seed in Q.BATCH_SEEDS[:calls]:
        pairs = [(None, t) for t in Q.random_batch(seed)[0]]
        work.append((Q.pack_base(pairs), Q.expected_table(pairs, ev)))
    torch.cuda.synchronize()
    kept = []
    for tt, _ in work:
        table, status = eng.term_scopes(tt)
        kept.append(snapshot(table, status))
    torch.cuda.synchronize()
    for (tt, want), got in zip(work, kept):
        check(tt, got, want, ev)


# ---- e: a live index ------------------------------------------------------------------------------------------------------------
def test_an_index_edited_with_the_stream_carried_resolves_the_same_expressions_over_the_new_documents(nat):
    from legal_rag_amd.bm25_model import BM25Okapi
    from legal_rag_amd.retrieval.engine import HybridEngine
    from legal_rag_amd.retrieval.terms import pack
    words = Q.world()[1]
    model = BM25Okapi(words)
    g = model.gpu()
    g.set_tokens(*model.token_stream(words))
    engine = HybridEngine(None, g, None)
    terms = Q.live_terms()
    docs, evs = words, Q.base_evaluator()
    for op, after in [(None, words)] + Q.edit_rounds(words):
        if op is not None:
            Q.apply_edit(model, op, carry=True)
            docs, evs = after, Q.Evaluator(after)
        assert model.gpu() is g and g.n_docs == len(docs)
        want_ptr, want_tok = model.token_stream(docs)
        got_ptr, got_tok = g.read_tokens()
        assert g.tokens_info() == (True, int(want_ptr[-1]))
        assert np.array_equal(got_ptr, want_ptr) and np.array_equal(got_tok, want_tok)
        vocab, df = model.vocab(), model._doc_frequencies()
        pairs = [(None, t) for t in terms if not Q.refused(t, vocab, df, len(docs))]
        assert len(pairs) >= len(terms) - 5
        tt = pack(pairs, vocab, df, len(docs), sorted_vocab=model.sorted_vocab())
        assert min(tt.n_phr, tt.n_near, tt.n_union, tt.n_cspan) >= 10
        table, status = engine.term_scopes(tt)
        torch.cuda.synchronize()
        check(tt, table[:3] + (status,), Q.expected_table(pairs, evs), evs, lists_of(engine, tt))


# ---- f: one consumer ------------------------------------------------------------------------------------------------------------
def test_scoped_bm25_and_the_scoped_batch_step_on_the_device_built_table_return_the_uploaded_tables_bits(nat, gi, ev):
    from legal_rag_amd.retrieval.engine import HybridEngine
    corpus = Q.world()[0]
    rng = np.random.default_rng(33)
    n, nq, k = corpus.n_docs, 70, 10
    X = (rng.integers(-8, 9, size=(n, 64)) / 8.0).astype(np.float32)
    engine = HybridEngine(nat.DenseIndex(X), gi, None)
    Qe = torch.from_numpy((rng.integers(-8, 9, size=(nq, 64)) / 8.0).astype(np.float32)).to(DEV)
    q_terms, q_ptr = nat.BM25Index.pack_queries([[int(t) for t in rng.integers(0, corpus.n_terms, size=5)] for _ in range(nq)])
    q_terms, q_ptr = torch.from_numpy(q_terms).to(DEV), torch.from_numpy(q_ptr).to(DEV)
    kept = Q.random_batch(Q.BATCH_SEEDS[0])[0]
    pairs = [(None, kept[i * 7 % 40]) for i in range(nq)]  # 40 constraints; questions share them
    params = nat.make_fuse_params(min_final_score=0.0)

    def outputs(table):
        s, i = engine.bm25_topk_scoped(q_terms, q_ptr, k, table)
        torch.cuda.synchronize()
        got = [s.cpu().numpy().copy(), i.cpu().numpy().copy()]
        res = engine.search_batch(params, k, q_emb=Qe, q_terms=q_terms, q_ptr=q_ptr, scopes=(table, table, None))
        torch.cuda.synchronize()
        return got + [t.cpu().numpy().copy() for t in (res.ids, res.vals, res.mask, res.count, res.dense_ids, res.dense_scores,
                                                       res.bm25_ids, res.bm25_scores)]
    tt, table, want = run(engine, pairs, ev)
    assert tt.n_cons == 40 and len(set(want[2].tolist())) == 40
    on_device = outputs(table)
    uploaded = outputs(engine.upload_scopes(want[0], want[1], want[2]))
    assert len(on_device) == len(uploaded) == 10
    for a, b in zip(on_device, uploaded):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (on_device[1] >= 0).any() and (on_device[2] >= 0).any()

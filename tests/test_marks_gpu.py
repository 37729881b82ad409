"""Marks and best passages on the GPU (amdr_bm25_marks: csrc/marks.hip, csrc/marks_rule.hpp): every output array of the
"_device" form (on torch tensors) and of the host twin equals the plain-Python restatement of tests/marks_cases.py, the
score bit for bit, at the smallest shapes where the kernel can go wrong — documents of 0 .. 1 500 tokens, phrases over a
round edge, at a document's end and across two documents, overlapping occurrences, loose and phrase-only slots, windows of
1 and of more than the document, equal windows, weights whose sum depends on the order, the mark cap, hit ids that are no
document, batches of 1 and 70 queries, empty tables, a class of 3 000 terms — plus determinism without workspace growth, the
refusals, and a live index under carrying updates."""
import numpy as np
import pytest
import torch

import marks_cases as MC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = -77
OP_TYPES = (torch.int64, torch.int32, torch.int32, torch.float64, torch.int32, torch.int64, torch.int64, torch.int32)


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


def make_index(nat, corpus):
    tp, pd, pt, idf, dl, avgdl = corpus.postings()
    gi = nat.BM25Index(tp, pd, pt, idf, dl, avgdl)
    gi.set_tokens(*corpus.stream())
    return gi


@pytest.fixture(scope="module")
def edge(nat):
    corpus, at = MC.edge_corpus()
    return corpus, at, make_index(nat, corpus), MC.edge_queries()


def dev_arr(a, dtype):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.zeros(max(int(a.size), 1), dtype=dtype, device=DEV)  # (one element at least: no null operand)
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a.ravel()))
    return t


def run_device(gi, hits, queries, window, cap, ld_docs=None):
    """amdr_bm25_marks_device on fresh tensors filled with SENTINEL: the five outputs as numpy arrays."""
    hits = np.asarray(hits, np.int64)
    nq, k = hits.shape
    ld = k if ld_docs is None else ld_docs
    padded = np.full((nq, ld), 2 ** 40, np.int64)  # (what lies behind a row's k ids is not read)
    padded[:, :k] = hits
    ops = [dev_arr(a, dt) for a, dt in zip(MC.operands(queries), OP_TYPES)]
    d = dev_arr(padded, torch.int64)
    pairs = max(nq * k, 1)
    win = torch.full((pairs * 4,), SENTINEL, dtype=torch.int32, device=DEV)
    score = torch.full((pairs,), float(SENTINEL), dtype=torch.float64, device=DEV)
    slots = torch.full((pairs * 2,), SENTINEL, dtype=torch.int32, device=DEV)
    marks = torch.full((pairs * max(cap, 1) * 2,), SENTINEL, dtype=torch.int32, device=DEV)
    status = torch.full((pairs,), SENTINEL, dtype=torch.int32, device=DEV)
    gi.marks_device(d.data_ptr(), nq, k, ld, *[x.data_ptr() for x in ops], window, cap, win.data_ptr(), score.data_ptr(),
                    slots.data_ptr(), marks.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n = nq * k
    tail = marks.cpu().numpy()[n * cap * 2:]
    assert np.all(tail == SENTINEL)  # nothing is written past the pairs' marks
    return (win.cpu().numpy()[:n * 4].reshape(nq, k, 4), score.cpu().numpy()[:n].reshape(nq, k),
            slots.cpu().numpy()[:n * 2].view(np.uint32).reshape(nq, k, 2), marks.cpu().numpy()[:n * cap * 2].reshape(nq, k, cap, 2),
            status.cpu().numpy()[:n].reshape(nq, k))


def same(got, want, what):
    names = ("win", "score", "slots", "marks", "status")
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)[:4].tolist()
            raise AssertionError((what, name, bad, [g[tuple(b)] for b in bad], [w[tuple(b)] for b in bad]))


def check_both(corpus, gi, hits, queries, window, cap, what, twin=True):
    want = MC.expected(corpus.docs, hits, queries, window, cap)
    same(run_device(gi, hits, queries, window, cap), want, (what, "device"))
    if twin:
        same(gi.marks(hits, *MC.operands(queries), window, cap), want, (what, "twin"))
    return want


# ---- the rule's edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window, cap", [(1, 0), (5, 2), (48, 32), (4096, 64)])
def test_every_edge_query_on_every_edge_document(edge, window, cap):
    """Document lengths 0, 1, 63, 64, 65, 79, 128 and 1 500; W = 1 and W >= the length; marks_cap 0, below the window's
    mark count, and 64."""
    corpus, at, gi, queries = edge
    names = list(queries)
    hits = np.tile(np.arange(corpus.n_docs, dtype=np.int64), (len(names), 1))
    want = check_both(corpus, gi, hits, [queries[n] for n in names], window, cap, (window, cap))
    win, score, slots, marks, status = want
    lens = sorted(len(corpus.docs[at[n]]) for n in at if n.startswith("len"))
    assert tuple(sorted(set(lens))) == MC.LENGTHS
    if cap == 2:
        assert (win[:, :, 2] > cap).any()  # marks_cap below the window's mark count


def test_the_cases_are_what_they_claim(edge):
    """The certificates of the edge cases, on the expected values the GPU is compared with above."""
    corpus, at, gi, Q = edge
    docs = corpus.docs

    def one(query, doc, window=48, cap=8):
        return MC.pair(docs[at[doc]], Q[query], window, cap)

    win, score, slots, marks, status = one("seven", "len79_straddle", window=7, cap=8)          # a round edge
    assert win == [60, 67, 7, 7] and marks[:7, 0].tolist() == list(range(60, 67))
    win, *_ = one("ab_phrase_only", "len63_ends_ab")                                             # ends at the document's end
    assert win == [61, 63, 2, 2]
    assert one("ab_phrase_only", "len64_tail_next")[0][3] == 0                                  # the tail is in the next document
    assert docs[at["len64_tail_next"]][-1] == MC.A and docs[at["len65_starts_b"]][0] == MC.B
    assert at["len65_starts_b"] == at["len64_tail_next"] + 1
    assert [p for p, _ in MC.marks_of(docs[at["len65_starts_b"]], Q["ab_phrase_only"])] == [31, 32]  # b at 0 stands alone
    assert [p for p, _ in MC.marks_of(docs[at["len128_overlap"]], Q["aa"])] == [10, 11, 12, 63, 64]  # overlapping; over 63 | 64
    both = MC.marks_of(docs[at["len128_overlap"]], Q["ab_a_loose"])                              # loose and a member
    assert (50, 1) not in both and (10, 0) in both and not any(s == 1 for _, s in both)          # b alone: unmarked
    win, score, *_ = one("abc_loose", "len128_overlap", window=3, cap=8)
    assert win[:3] == [100, 103, 3] and score == 0.1 + 0.2 + 0.3 and score != 0.3 + 0.2 + 0.1   # the addition order
    win, *_ = one("abc_loose", "len128_overlap", window=1)
    assert win[:3] == [10, 11, 1]                                                               # equal windows: the earlier
    win, _, _, _, status = one("abc_loose", "len1500_all_a", window=4096, cap=64)
    assert status == 1 and win == [0, 1500, MC.MAX_MARKS, 1500]                                 # the true count
    assert one("empty", "len1500_mixed")[0] == [0, 48, 0, 0]
    cls = MC.marks_of(docs[at["class_then_a"]], Q["prefix_class"])
    assert cls == [(3, 0), (4, 1), (40, 0), (41, 1), (50, 0), (51, 31), (69, 0)] and len(Q["prefix_class"].table) == 3002


@pytest.mark.parametrize("nq, k", [(1, 1), (1, 16), (70, 1), (70, 3)])
def test_batch_shapes_with_random_queries(edge, nq, k):
    corpus, at, gi, _ = edge
    queries = MC.rand_queries(corpus, nq, seed=nq * 10 + k)
    rng = np.random.default_rng(nq + k)
    hits = rng.integers(0, corpus.n_docs, size=(nq, k)).astype(np.int64)
    hits[0, 0] = at["len128_overlap"]
    check_both(corpus, gi, hits, queries, 48, 32, (nq, k))


def test_hit_ids_that_are_no_document_and_a_leading_dimension(edge):
    corpus, at, gi, Q = edge
    queries = [Q["ab_a_loose"], Q["abc_loose"]]
    hits = np.asarray([[at["len128_overlap"], -1, at["len1"]], [-1, at["len79_straddle"], -1]], np.int64)
    want = check_both(corpus, gi, hits, queries, 48, 4, "minus one")
    assert not want[0][0, 1].any() and want[1][0, 1] == 0.0 and np.all(want[3][0, 1] == -1)
    # the "_device" form takes ids as they are: n_docs, -7 and 2^40 read nothing
    wild = hits.copy()
    wild[0, 1], wild[1, 0], wild[1, 2] = corpus.n_docs, -7, 2 ** 40
    same(run_device(gi, wild, queries, 48, 4, ld_docs=5), want, "wild ids, ld_docs = 5")


def test_a_repeated_call_gives_identical_bytes_and_grows_no_workspace(nat, edge):
    corpus, at, gi, Q = edge
    names = list(Q)
    hits = np.tile(np.arange(corpus.n_docs, dtype=np.int64), (len(names), 1))
    queries = [Q[n] for n in names]
    first = run_device(gi, hits, queries, 48, 32)
    twin = gi.marks(hits, *MC.operands(queries), 48, 32)
    g0 = nat.workspace_growths()
    same(run_device(gi, hits, queries, 48, 32), first, "device again")
    same(gi.marks(hits, *MC.operands(queries), 48, 32), twin, "twin again")
    assert nat.workspace_growths() == g0
    assert gi.marks_kernel_ms() > 0.0


def test_refusals(nat, edge):
    corpus, at, gi, Q = edge
    q = [Q["ab_a_loose"]]
    ops = list(MC.operands(q))
    hits = np.asarray([[0, 1]], np.int64)
    gi.marks(hits, *ops, 48, 4)

    def refused(h=hits, o=ops, window=48, cap=4, match=None):
        with pytest.raises(nat.NativeError, match=match):
            gi.marks(h, *o, window, cap)

    refused(window=0, match="window"), refused(window=4097, match="window")
    refused(cap=-1, match="marks_cap"), refused(cap=65, match="marks_cap")
    refused(h=np.asarray([[0, corpus.n_docs]], np.int64), match="hit id"), refused(h=np.asarray([[-2, 0]], np.int64), match="hit id")

    def with_(i, value):
        o = list(ops)
        o[i] = np.asarray(value, dtype=ops[i].dtype)
        return o

    refused(o=with_(0, [1, 2]), match="monotonically")
    refused(o=with_(1, [1, 0]), match="ascending"), refused(o=with_(1, [0, 0]), match="ascending")
    refused(o=with_(1, [0, corpus.n_terms]), match="n_terms")
    refused(o=with_(2, [0, 32]), match="slot"), refused(o=with_(7, [0, 32]), match="slot")
    w = ops[3].copy()
    w[0, 5] = np.inf
    refused(o=with_(3, w), match="finite")
    refused(o=with_(6, [0, 1]), match="sequence")
    # the "_device" form: sizes and nulls
    d = dev_arr(hits, torch.int64)
    t = [dev_arr(a, dt) for a, dt in zip(ops, OP_TYPES)]
    out = [torch.zeros(64, dtype=torch.int64, device=DEV) for _ in range(5)]

    def device(nq=1, k=2, ld=2, window=48, cap=4, null=None):
        p = [d.data_ptr(), nq, k, ld] + [x.data_ptr() for x in t] + [window, cap] + [x.data_ptr() for x in out]
        if null is not None:
            p[null] = 0
        gi.marks_device(*p, torch.cuda.current_stream().cuda_stream)

    device()
    for kw in (dict(window=0), dict(window=4097), dict(cap=-1), dict(cap=65), dict(nq=-1), dict(k=-1), dict(ld=1), dict(null=0),
               dict(null=4), dict(null=11), dict(null=14), dict(null=18)):
        with pytest.raises(nat.NativeError):
            device(**kw)
    device(cap=0, null=17)  # no marks are written: out_marks may be null
    torch.cuda.synchronize()
    bare = nat.BM25Index(*corpus.postings())  # no token stream
    with pytest.raises(nat.NativeError, match="token stream"):
        bare.marks(hits, *ops, 48, 4)


def test_marks_on_a_live_index_equal_a_fresh_create(nat, edge):
    """After amdr_bm25_add_carry and amdr_bm25_remove_carry the marks equal those on a fresh create of the same index, and
    both equal the restatement on the edited documents."""
    import phrase_cases as PC
    corpus, at, _, Q = edge
    head, tail, gone = corpus.docs[:9], corpus.docs[9:], [1, 4, 12]
    live = make_index(nat, PC.SeqCorpus("head", corpus.n_terms, head))
    tp, pd, pt, idf, dl, avgdl = corpus.postings()
    a_tp, a_pd, a_pt, _, a_dl, _ = PC.SeqCorpus("tail", corpus.n_terms, tail).postings()
    live.add(a_tp, a_pd, a_pt, idf, a_dl, avgdl, tokens=PC.SeqCorpus("tail", corpus.n_terms, tail).stream())
    names = list(Q)
    queries = [Q[n] for n in names]
    hits = np.tile(np.arange(corpus.n_docs, dtype=np.int64), (len(names), 1))
    want = MC.expected(corpus.docs, hits, queries, 48, 16)
    same(live.marks(hits, *MC.operands(queries), 48, 16), want, "after add_carry")
    same(run_device(live, hits, queries, 48, 16), want, "after add_carry, device")
    left = PC.SeqCorpus("left", corpus.n_terms, [d for i, d in enumerate(corpus.docs) if i not in gone])
    live.remove(np.asarray(gone, np.int64), idf, left.postings()[5], carry=True)
    assert live.tokens_info()[0] and live.n_docs == left.n_docs
    fresh = make_index(nat, left)
    hits = hits[:, :left.n_docs]
    want = MC.expected(left.docs, hits, queries, 48, 16)
    got_live, got_fresh = run_device(live, hits, queries, 48, 16), run_device(fresh, hits, queries, 48, 16)
    same(got_live, got_fresh, "live against fresh")
    same(got_live, want, "after remove_carry")
    same(live.marks(hits, *MC.operands(queries), 48, 16), want, "after remove_carry, twin")
    live.close(), fresh.close()

"""amdr_shard_pack_device / amdr_shard_merge_device (csrc/shard.hip) on the cases of tests/shard_adversary.py, and on
emulated worlds over the real channels.

Part 1 — every generated case: the packed rows word for word against sharding.pack_channels(to_global(...)), the merged
ids and score BITS against the fp64 reference (oracle.dense.merge_topk; the documented differences are -0.0 -> +0.0 and the
payload of a NaN), against merge_parts_kernel on the unpacked channel bit for bit, exact padding, sentinel words around
every buffer the launches write, the gathered buffer unchanged by the merge, and the edges counted IN THE RESULTS.

Part 2 — one process, no process group: a corpus cut by hand into 3 and 8 uneven contiguous blocks (one shorter than k,
one of a single row, one larger than all the others together), one handle per block, the blocks' search outputs packed
with their offsets and merged in one launch, compared with the handle of the whole corpus and with the oracle."""
import functools

import numpy as np
import pytest
import torch

import shard_adversary as SA
from shard_adversary import F32, F64, bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GUARD = 256   # sentinel bytes either side of a guarded buffer
SENTINEL = 0xA5
MAXSIM_TOL = 1e-4  # test_kernels_gpu.py TOL: MaxSim against its fp64 oracle


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


def stream():
    return int(torch.cuda.current_stream().cuda_stream)


def tdtype(dt):
    return torch.float32 if dt == F32 else torch.float64


class Guarded:
    """A tensor in the middle of a larger sentinel-filled allocation."""

    def __init__(self, shape, dtype):
        self.n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((GUARD + self.n + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.n].view(dtype).view(shape)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == SENTINEL).all()) and bool((self.raw[GUARD + self.n:] == SENTINEL).all())


def ibits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ---------------------------------------------------------------------------------------------------------------------
# Part 1: the generated cases

def run_case(nat, case):
    """pack (one launch per emulated rank) + merge (one launch) of a case with every check; -> [(scores, ids)] numpy"""
    from legal_rag_amd.retrieval import sharding
    world, nq, ks = case.world, case.nq, case.ks
    row = nat.shard_row_words(ks)
    assert row == 2 * sum(ks)
    S = [torch.from_numpy(np.stack([case.lists[r][c][0] for r in range(world)])).to(DEV) for c in range(len(ks))]
    I = [torch.from_numpy(np.stack([case.lists[r][c][1] for r in range(world)])).to(DEV) for c in range(len(ks))]
    gathered = Guarded((world, nq, row), torch.int64)
    # the last rank first: a pack that wrote past its own [nq, row] block would spoil rows that are already there
    for r in reversed(range(world)):
        nat.shard_pack_device([(S[c][r].data_ptr(), I[c][r].data_ptr(), k, dt == F64) for c, (k, dt) in enumerate(case.chans)],
                              nq, case.offsets[r], gathered.t[r].data_ptr(), device=0, stream=stream())
    torch.cuda.synchronize()
    assert gathered.guards_intact(), case.name
    for r in range(world):
        ref = sharding.pack_channels([(S[c][r], sharding.to_global(I[c][r], case.offsets[r])) for c in range(len(ks))])
        assert torch.equal(gathered.t[r], ref), (case.name, r)
    before = gathered.t.clone()
    out = [(Guarded((nq, k), tdtype(dt)), Guarded((nq, k), torch.int64)) for k, dt in case.chans]
    nat.shard_merge_device(gathered.t.data_ptr(), world, nq,
                           [(s.t.data_ptr(), i.t.data_ptr(), k, dt == F64) for (s, i), (k, dt) in zip(out, case.chans)],
                           device=0, stream=stream())
    torch.cuda.synchronize()
    assert torch.equal(gathered.t, before) and gathered.guards_intact(), case.name
    assert all(s.guards_intact() and i.guards_intact() for s, i in out), case.name
    unpacked = sharding.unpack_channels(gathered.t, ks, [tdtype(dt) for _, dt in case.chans])
    res = []
    for c, (k, dt) in enumerate(case.chans):
        what = (case.name, c, k, dt.__name__, SA.path_of(world, k))
        es, ei = SA.reference_cached(case, c)
        want, nan = SA.kernel_view(es, ei, dt)
        gs, gi = out[c][0].t.cpu().numpy(), out[c][1].t.cpu().numpy()
        assert np.array_equal(gi, ei), what
        assert np.array_equal(bits(gs)[~nan], bits(want)[~nan]), what  # hits: the bits that went in; padding: -MAX
        assert np.isnan(gs[nan]).all(), what
        pad = ei < 0
        assert np.all(gi[pad] == -1) and np.all(bits(gs)[pad] == bits(np.asarray(-SA.fmax(dt)))), what
        # merge_parts_kernel (topk_merge.hip) shares topk.hpp with this kernel: bit for bit, a NaN's payload included
        os_, oi = sharding.native_merge(unpacked[c][0], unpacked[c][1], k)
        torch.cuda.synchronize()
        assert torch.equal(oi, out[c][1].t), what
        diff = (ibits(os_) != ibits(out[c][0].t)).nonzero()
        assert diff.numel() == 0, (what, "first difference at", diff[0].tolist(),
                                   hex(int(ibits(os_)[tuple(diff[0])]) & (2 ** 64 - 1)),
                                   hex(int(ibits(out[c][0].t)[tuple(diff[0])]) & (2 ** 64 - 1)))
        res.append((gs, gi))
    return res


# the edges a family is there for: non-zero in the GPU RESULTS (and equal to what the reference holds)
FAMILY_EDGES = {
    "depth": ("tie", "row_short", "row_empty", "row_exactly_k"),
    "short": ("row_empty", "row_short", "row_exactly_k", "row_k_plus_1"),
    "values": ("nan_hit", "zero_pair_in_id_order", "pad_valued_hit", "inf_hit", "subnormal_hit", "tie", "row_short",
               "row_exactly_k"),
    "wide": ("id_ge_2_32", "tie_high_word_only", "tie_low_words_reversed", "tie", "row_short"),
    "layouts": ("tie", "row_short", "row_exactly_k", "row_k_plus_1"),
}


@pytest.mark.parametrize("family", SA.FAMILIES)
def test_generated_cases_equal_the_reference_bit_for_bit(nat, family):
    seen, expected, paths = {}, {}, set()
    for case in SA.cases(family):
        res = run_case(nat, case)
        for c, (k, dt) in enumerate(case.chans):
            es, ei = SA.reference_cached(case, c)
            SA.add_counts(seen, SA.edge_counts(case, c, es, res[c][0], res[c][1]))
            SA.add_counts(expected, SA.edge_counts(case, c, es, SA.kernel_view(es, ei, dt)[0], ei))
            paths.add((SA.path_of(case.world, k), case.staged_launch))
    print(f"\nshard adversary [{family}]: {len(SA.cases(family))} cases, edges in the GPU results: {seen}")
    assert seen == expected
    for key in FAMILY_EDGES[family]:
        assert seen[key] > 0, (family, key, seen)
    assert {p for p, _ in paths} == {"one_sort", "two_halves", "staged"}
    if family == "layouts":  # the register paths inside the staged launch
        assert ("one_sort", True) in paths and ("two_halves", True) in paths and ("one_sort", False) in paths


def test_a_negative_id_other_than_minus_one_is_padding_and_passes_the_pack_unchanged(nat):
    """ids -2 and -(2^40) under a non-zero offset: the packed word is the id itself, the merge treats it as no entry"""
    s = np.array([[3.0, 2.0, 9e9, 9e9]], dtype=np.float32)
    i = np.array([[5, 1, -2, -(1 << 40)]], dtype=np.int64)
    ds, di = torch.from_numpy(s).to(DEV), torch.from_numpy(i).to(DEV)
    send = Guarded((1, 1, 8), torch.int64)
    nat.shard_pack_device([(ds.data_ptr(), di.data_ptr(), 4, False)], 1, (1 << 33) + 11, send.t.data_ptr(), stream=stream())
    os_, oi = Guarded((1, 4), torch.float32), Guarded((1, 4), torch.int64)
    nat.shard_merge_device(send.t.data_ptr(), 1, 1, [(os_.t.data_ptr(), oi.t.data_ptr(), 4, False)], stream=stream())
    torch.cuda.synchronize()
    assert send.t[0, 0, 4:].tolist() == [(1 << 33) + 16, (1 << 33) + 12, -2, -(1 << 40)]
    assert send.t[0, 0, :4].view(torch.float64).tolist() == [float(v) for v in s[0]]  # fp32 widens exactly
    assert oi.t[0].tolist() == [(1 << 33) + 16, (1 << 33) + 12, -1, -1]
    assert bits(os_.t.cpu().numpy())[0].tolist() == bits(np.array([3.0, 2.0, -SA.FLT_MAX, -SA.FLT_MAX], np.float32)).tolist()
    assert send.guards_intact() and os_.guards_intact() and oi.guards_intact()


# ---------------------------------------------------------------------------------------------------------------------
# Part 2: emulated worlds over the real channels

N = 300
BOUNDS = {3: (0, 7, 8, N), 8: (0, 5, 6, 20, 40, 75, 95, 110, N)}  # by hand: uneven, not sharding.shard_bounds
DUP = {3: (3, 150), 8: (45, 100)}  # MaxSim: document DUP[W][1] repeats document DUP[W][0]; different blocks, see below


def test_the_hand_made_bounds_are_the_uneven_ones():
    from legal_rag_amd.retrieval import sharding
    for W, b in BOUNDS.items():
        sizes = np.diff(b)
        assert len(sizes) == W and b[0] == 0 and b[-1] == N and (sizes > 0).all()
        assert [tuple(x) for x in zip(b[:-1], b[1:])] != sharding.shard_bounds(N, W)
        assert (sizes < 10).any() and (sizes == 1).any() and sizes.max() > sizes.sum() - sizes.max()
        block_of = lambda d: int(np.searchsorted(b, d, side="right")) - 1
        assert block_of(DUP[W][0]) != block_of(DUP[W][1])


def exchange(nat, blocks, offsets):
    """blocks[r][c] = (scores, LOCAL ids) as block r's handle returned them (numpy): uploaded, packed with the block's
    offset into one [W, nq, row] buffer, merged in ONE launch for all channels -> [(scores, ids)] numpy"""
    W, nq = len(blocks), blocks[0][0][0].shape[0]
    ks = [i.shape[1] for _, i in blocks[0]]
    f64 = [s.dtype == np.float64 for s, _ in blocks[0]]
    gathered = torch.empty((W, nq, nat.shard_row_words(ks)), dtype=torch.int64, device=DEV)
    for r in range(W):
        up = [(torch.from_numpy(np.array(s)).to(DEV), torch.from_numpy(np.array(i)).to(DEV)) for s, i in blocks[r]]
        nat.shard_pack_device([(s.data_ptr(), i.data_ptr(), k, d) for (s, i), k, d in zip(up, ks, f64)], nq, int(offsets[r]),
                              gathered[r].data_ptr(), stream=stream())
        torch.cuda.synchronize()  # `up` is released below
    out = [(torch.empty((nq, k), dtype=torch.float64 if d else torch.float32, device=DEV),
            torch.empty((nq, k), dtype=torch.int64, device=DEV)) for k, d in zip(ks, f64)]
    nat.shard_merge_device(gathered.data_ptr(), W, nq, [(s.data_ptr(), i.data_ptr(), k, d) for (s, i), k, d in zip(out, ks, f64)],
                           stream=stream())
    torch.cuda.synchronize()
    return [(s.cpu().numpy(), i.cpu().numpy()) for s, i in out]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Corpus:
    """One channel's corpus: the whole handle, a handle per block of BOUNDS[W], and their searches (each run once)."""

    def __init__(self, make_handle, search):
        self.make_handle, self.search_fn = make_handle, search
        self.handles, self.results = {}, {}

    def handle(self, lo, hi):
        if (lo, hi) not in self.handles:
            self.handles[(lo, hi)] = self.make_handle(lo, hi)
        return self.handles[(lo, hi)]

    def search(self, lo, hi, k):
        if (lo, hi, k) not in self.results:
            s, i = self.search_fn(self.handle(lo, hi), k)
            s.setflags(write=False)
            i.setflags(write=False)
            self.results[(lo, hi, k)] = (s, i)
        return self.results[(lo, hi, k)]

    def blocks(self, W, k):
        b = BOUNDS[W]
        return [self.search(lo, hi, k) for lo, hi in zip(b[:-1], b[1:])]

    def close(self):
        for h in self.handles.values():
            h.close()


NQ = 5  # queries of every channel, so that the three can share one launch


@pytest.fixture(scope="module")
def dense(nat):
    from test_topk_merge_gpu import small_int_rows
    rng = np.random.default_rng(4300)
    X = small_int_rows(rng, 37, N, 64)  # every dot exact in any order; every score again 37 rows on: in every block
    Q = rng.integers(-2, 3, size=(NQ, 64)).astype(np.float32)
    c = Corpus(lambda lo, hi: nat.DenseIndex(X[lo:hi]), lambda h, k: h.search(Q, k))
    c.X, c.Q = X, Q
    yield c
    c.close()


@pytest.fixture(scope="module")
def bm25(nat):
    from bm25_update_cases import make_docs
    from legal_rag_amd.bm25_model import shard_csr
    from oracle import bm25 as OB
    rng = np.random.default_rng(4301)
    docs = make_docs(rng, N)
    for W in BOUNDS:  # the 1-row blocks hold a document of their own words
        docs[BOUNDS[W][1]] = ["all", "solo", "solo"]
    ob = OB.BM25Okapi(docs)
    csr = OB.to_csr(ob)
    df = {w: sum(w in d for d in ob.doc_freqs) for w in csr["vocab"]}
    rare = sorted(w for w, n in df.items() if w.startswith("z") and 2 <= n <= 6)[:1]
    assert len(rare) == 1 and df["z0"] > 80
    # "z0": no document of a 1-row block holds it; `rare`: most documents stay at +0.0 — ties at the cut and across
    # every boundary; "all": every document scores; an unknown word and an empty query: +0.0 everywhere
    queries = [["z0"], rare, ["z1", "z0", "solo", "all", "z1"], ["nothing"], []]
    assert len(queries) == NQ
    tid = [[csr["vocab"].get(t, -1) for t in q] for q in queries]

    def make(lo, hi):  # the block's postings under the WHOLE corpus's idf and avgdl
        tp, pd, pt, dl = shard_csr(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["doc_len"], lo, hi)
        return nat.BM25Index(tp, pd, pt, csr["idf"], dl, ob.avgdl, ob.k1, ob.b)

    c = Corpus(make, lambda h, k: h.search(tid[:NQ], k))
    c.ob, c.queries, c.tid, c.docs = ob, queries, tid, docs
    yield c
    c.close()


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def maxsim_store(W, k):
    """Unit-norm tokens, 2-9 per document, document DUP[W][1] a copy of DUP[W][0]; NQ queries whose fp64 top-(k+1) scores
    lie further apart than 2 * MAXSIM_TOL (checked here, on the CPU) — the repeated pair, exactly tied, excepted.  Query
    0 is made of the repeated document's tokens, so the pair leads it."""
    from oracle import maxsim as OM
    rng = np.random.default_rng(4302 + W)
    a, b = DUP[W]
    lens = rng.integers(2, 10, size=N)
    lens[b] = lens[a]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    D = unit_rows(rng, int(ptr[-1]), 128)
    D[ptr[b]:ptr[b + 1]] = D[ptr[a]:ptr[a + 1]]
    q_len = 8
    cand = unit_rows(rng, 16 * q_len, 128).reshape(16, q_len, 128)
    for q in range(4):  # four tries at the query of the repeated document's tokens: the first that passes is kept
        own = D[ptr[a] + np.arange(q_len) % lens[a]] + 0.3 * unit_rows(rng, q_len, 128)
        cand[q] = own / np.linalg.norm(own, axis=1, keepdims=True)
    ref = OM.maxsim_scores(cand, D, ptr)
    keep = []
    for q in range(len(cand)):
        order = np.lexsort((np.arange(N), -ref[q]))[:k + 1]
        gap = -np.diff(ref[q, order])
        tied = (order[:-1] == a) & (order[1:] == b)
        if np.all((gap > 2 * MAXSIM_TOL) | tied):
            keep.append(q)
    keep = keep[:1] + [q for q in keep[1:] if q >= 4]
    assert keep[0] < 4 and len(keep) >= NQ, keep
    Q = np.ascontiguousarray(cand[keep[:NQ]])
    top = np.lexsort((np.arange(N), -ref[keep[0]]))[:2]
    assert top.tolist() == [a, b] and ref[keep[0], a] == ref[keep[0], b]
    return D, ptr, Q, ref[keep[:NQ]]


@pytest.fixture(scope="module", params=sorted(BOUNDS))
def maxsim(nat, request):
    W = request.param
    D, ptr, Q, ref = maxsim_store(W, 10)
    c = Corpus(lambda lo, hi: nat.MaxSimIndex(D[ptr[lo]:ptr[hi]], ptr[lo:hi + 1] - ptr[lo]), lambda h, k: h.search(Q, k))
    c.W, c.D, c.ptr, c.Q, c.ref = W, D, ptr, Q, ref
    yield c
    c.close()


@pytest.mark.parametrize("k", [10, 80])
@pytest.mark.parametrize("W", sorted(BOUNDS))
def test_emulated_world_dense(nat, dense, W, k):
    from oracle import dense as OD
    (gs, gi), = exchange(nat, [[blk] for blk in dense.blocks(W, k)], BOUNDS[W][:-1])
    es, ei = OD.flatip_topk(dense.X, dense.Q, k)
    ws, wi = dense.search(0, N, k)
    assert np.array_equal(gi, ei) and same_bits(gs, es), (W, k)
    assert np.array_equal(gi, wi) and same_bits(gs, ws), (W, k)
    sizes = np.diff(BOUNDS[W])
    assert (sizes < k).any()  # a block's own -1 / -FLT_MAX tail went through the exchange
    ties = (gs[:, 1:] == gs[:, :-1]) & (np.searchsorted(BOUNDS[W], gi[:, 1:], side="right")
                                        != np.searchsorted(BOUNDS[W], gi[:, :-1], side="right"))
    assert ties.any()  # equal scores from different blocks, next to each other in the result


@pytest.mark.parametrize("k", [10, 80])
@pytest.mark.parametrize("W", sorted(BOUNDS))
def test_emulated_world_bm25(nat, bm25, W, k):
    from oracle import bm25 as OB
    (gs, gi), = exchange(nat, [[blk] for blk in bm25.blocks(W, k)], BOUNDS[W][:-1])
    ws, wi = bm25.search(0, N, k)
    assert gs.dtype == np.float64 and np.array_equal(gi, wi) and same_bits(gs, ws), (W, k)
    for qn, q in enumerate(bm25.queries[:NQ]):
        exp = OB.search(bm25.ob, q, k)
        assert gi[qn].tolist() == [e[0] for e in exp], (W, k, q)
        assert bits(gs[qn]).tolist() == bits(np.asarray([e[1] for e in exp], dtype=np.float64)).tolist(), (W, k, q)
    one = BOUNDS[W][1]  # the 1-row block's document
    assert "z0" not in bm25.docs[one] and not (set(bm25.queries[1]) & set(bm25.docs[one]))
    zeros = (gs == 0).sum(axis=1)
    assert zeros[1] >= k - 6 and zeros[3] == k and zeros[4] == k  # +0.0 fills the list up to the cut: lowest ids first
    assert gi[3].tolist() == list(range(k)) and gi[4].tolist() == list(range(k))


def test_emulated_world_maxsim(nat, maxsim):
    from oracle import dense as OD
    W, k = maxsim.W, 10
    a, b = DUP[W]
    bounds = BOUNDS[W]
    whole = maxsim.handle(0, N)
    spans = list(zip(bounds[:-1], bounds[1:]))
    # precondition: every block's store reports the power-of-two scale of the whole store
    assert all(maxsim.handle(lo, hi).info()[3] == whole.info()[3] for lo, hi in spans)
    (gs, gi), = exchange(nat, [[blk] for blk in maxsim.blocks(W, k)], bounds[:-1])
    es, ei = OD.topk_desc(maxsim.ref, k)  # oracle.maxsim.maxsim_topk of the whole store (ref = its maxsim_scores)
    assert np.array_equal(gi, ei)
    assert np.max(np.abs(gs - es)) <= MAXSIM_TOL
    ws, wi = maxsim.search(0, N, k)
    assert np.array_equal(gi, wi)
    # the repeated document: its two hits next to each other, the lower global id first
    assert gi[0, :2].tolist() == [a, b]
    block_of = lambda d: spans[int(np.searchsorted(bounds, d, side="right")) - 1]
    plans = [maxsim.handle(*block_of(d)).plan_info(NQ) for d in (a, b)]
    print(f"\nmaxsim W={W}: plans of the repeated document's blocks: {plans}")
    if plans[0] == plans[1]:
        assert bits(gs[0, :1]) == bits(gs[0, 1:2])


@pytest.mark.parametrize("W", sorted(BOUNDS))
def test_emulated_world_three_channels_in_one_launch(nat, dense, bm25, W):
    """dense (fp32, k = 80), BM25 (fp64, k = 10), MaxSim (fp32, k = 40) through ONE pack per block and ONE merge: every
    channel as if it had been merged alone.  k = 80 and 40 exceed most blocks' rows: the channels' own tail padding goes
    through the exchange."""
    from oracle import bm25 as OB
    from oracle import dense as OD
    D, ptr, Q, _ = maxsim_store(W, 10)
    ms = Corpus(lambda lo, hi: nat.MaxSimIndex(D[ptr[lo]:ptr[hi]], ptr[lo:hi + 1] - ptr[lo]), lambda h, k: h.search(Q, k))
    try:
        per = [dense.blocks(W, 80), bm25.blocks(W, 10), ms.blocks(W, 40)]
    finally:
        ms.close()
    assert [p[0][0].dtype for p in per] == [np.float32, np.float64, np.float32]
    assert all((blk[1][:, -1] == -1).all() for blk in per[0][:2] + per[2][:2])  # padded tails go in
    together = exchange(nat, [[per[c][r] for c in range(3)] for r in range(W)], BOUNDS[W][:-1])
    for c in range(3):
        (s, i), = exchange(nat, [[blk] for blk in per[c]], BOUNDS[W][:-1])
        assert np.array_equal(together[c][1], i) and same_bits(together[c][0], s), (W, c)
    es, ei = OD.flatip_topk(dense.X, dense.Q, 80)
    assert np.array_equal(together[0][1], ei) and same_bits(together[0][0], es)
    for qn, q in enumerate(bm25.queries[:NQ]):
        exp = OB.search(bm25.ob, q, 10)
        assert together[1][1][qn].tolist() == [e[0] for e in exp]
        assert bits(together[1][0][qn]).tolist() == bits(np.asarray([e[1] for e in exp], dtype=np.float64)).tolist()
    assert (together[2][1] >= 0).all() and all(len(set(r.tolist())) == 40 for r in together[2][1])

"""The register top-k selectors (csrc/topk.hpp wave_select_small, wave_select_small_pair32) and the staged selector behind
the same launches, on rows whose survivor count at the selectors' cut is chosen (tests/selector_adversary.py): both sides of
every sort-width switch and of the slot limit, give-ups without a tie, mass ties, fewer populated lanes than k, every
keys-per-lane switch at n and n +- 1, special values.  Every comparison is == against oracle.dense.topk_desc of the score
row: ids, and scores by bits.  Each case asserts through the model that its input is in the regime it is there for, and
through plan_info or the environment pins which kernel ranks it."""

import numpy as np
import pytest

import selector_adversary as SA
from selector_adversary import PAIR, SINGLE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    return _native


class Refs:
    """reference(column, k) and the model's survivor count, computed once per (column, k)."""

    def __init__(self, cs, selector):
        self.cs, self.selector, self.ref, self.surv = cs, selector, {}, {}

    def expect(self, c, k):
        if (c, k) not in self.ref:
            self.ref[c, k] = SA.reference(self.cs.cols[c], k)
        return self.ref[c, k]

    def survivors(self, c, k):
        if (c, k) not in self.surv:
            self.surv[c, k] = SA.survivors(self.cs.cols[c], k, self.selector)
        return self.surv[c, k]

    def check(self, s, i, ids, k, what):
        """Rows of a result against the oracle; a crafted row searched at its own k has the survivors it was built for."""
        for b, c in enumerate(ids):
            m = self.cs.meta[c]
            got = self.survivors(c, k)
            if m["k"] == k and m["kind"] in ("craft", "all_survive"):
                assert got == m["s"], (what, m, got)
            SA.assert_same(s[b], i[b], *self.expect(c, k), what=(what, k, m, f"survivors={got}"))


def _slab_plan(info):
    return "scores_slab_topk_kernel" in info and "merge" not in info and "scores_pair_topk_kernel" not in info


# ---- A. one row per wave: scores_slab_topk_kernel<1> -------------------------------------------------------------------
@pytest.mark.parametrize("n", SA.A_N)
def test_single_selector(nat, monkeypatch, n):
    """Every column of the n at every k in a batch (AMDR_TOPK_PAIR=0: one query per wave whatever the shape), and each
    crafted row alone at its own k (one query: no pair to share a wave).  k > n pads."""
    cs = SA.case_columns(n, SINGLE)
    refs = Refs(cs, SINGLE)
    regimes = set()
    for c0, X in cs.matrices():
        ids = list(range(c0, min(c0 + cs.d, len(cs.cols))))
        Q = cs.queries(ids, c0)
        idx = nat.DenseIndex(X)
        monkeypatch.setenv("AMDR_TOPK_PAIR", "0")
        for k in SA.A_K:
            assert _slab_plan(idx.plan_info(len(ids), k)), idx.plan_info(len(ids), k)
            s, i = idx.search(Q, k)
            refs.check(s, i, ids, k, (n, "batch"))
            if k > n:
                assert np.all(i[:, n:] == -1) and np.all(s[:, n:] == -SA.FLT_MAX)
        monkeypatch.delenv("AMDR_TOPK_PAIR")
        for b, c in enumerate(ids):
            m = cs.meta[c]
            if m["kind"] not in ("craft", "all_survive", "tie_all"):
                continue
            k = m["k"]
            assert _slab_plan(idx.plan_info(1, k)), idx.plan_info(1, k)
            s, i = idx.search(Q[b:b + 1], k)
            refs.check(s, i, [c], k, (n, "alone"))
            if m["kind"] != "tie_all":
                regimes.add((SA.gives_up(cs.cols[c], k, SINGLE), SA.sort_width(min(m["s"], 64), SINGLE)))
        idx.close()
    if n >= 257:  # rows enough for 100 survivors: both sides of the slot limit, all three sort widths
        assert regimes >= {(False, 16), (False, 32), (False, 64), (True, 64)}, regimes


# ---- B. two rows per wave: scores_pair_topk_kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("n", SA.B_N)
def test_pair_selector(nat, monkeypatch, n):
    """Every column at every k, two per wave in the order given; behind them a row that gives up and one that does not
    as (gives up, stays), (stays, gives up) and a last wave with one query; the first three queries as a short batch
    (other scores kernel, odd count).  Both AMDR_TOPK_PAIR settings agree with the oracle, hence with each other."""
    cs = SA.case_columns(n, PAIR)
    refs = Refs(cs, PAIR)
    mixed_seen = False
    for c0, X in cs.matrices():
        base = list(range(c0, min(c0 + cs.d, len(cs.cols))))
        idx = nat.DenseIndex(X)
        for k in SA.B_K:
            ids = base + base[:len(base) % 2]  # an even count: the pairs below start on a wave
            up = [c for c in base if refs.survivors(c, k) > 32]
            stay = [c for c in base if refs.survivors(c, k) <= 32]
            if up and stay:
                g, f = up[-1], stay[-1]
                ids += [g, f, f, g, g]
                mixed_seen = True
            elif len(ids) > 1:
                ids = ids[:-1]
            gave = [refs.survivors(c, k) > 32 for c in ids]
            if up and stay:
                assert gave[-5:] == [True, False, False, True, True] and len(ids) % 2 == 1
            Q = cs.queries(ids, c0)
            for pin in (None, "0"):
                if pin is None:
                    monkeypatch.delenv("AMDR_TOPK_PAIR", raising=False)
                else:
                    monkeypatch.setenv("AMDR_TOPK_PAIR", pin)
                for nq in sorted({len(ids), min(3, len(ids))}):
                    info = idx.plan_info(nq, k)
                    assert ("scores_pair_topk_kernel" in info) == (pin is None and nq >= 2), (nq, k, pin, info)
                    assert pin is None and nq >= 2 or _slab_plan(info), info
                    s, i = idx.search(Q[:nq], k)
                    refs.check(s, i, ids[:nq], k, (n, nq, pin))
                    if k > n:
                        assert np.all(i[:, n:] == -1) and np.all(s[:, n:] == -SA.FLT_MAX)
        monkeypatch.delenv("AMDR_TOPK_PAIR", raising=False)
        assert "scores_pair_topk_kernel" not in idx.plan_info(1, 10)  # one query has no partner
        idx.close()
    assert mixed_seen == (n > 32)  # (<= 32 rows fit the slots whatever the cut)
    if n in (33, 100, 127):  # fewer populated lanes than k: the cut is padding, every row survives, the wave gives up
        for k in (31, 32):
            if k > SA.lanes_populated(n, PAIR):
                assert all(refs.survivors(c, k) == n for c in range(len(cs.cols)))


def test_plan_info_names_the_topk_kernel_that_runs(nat, monkeypatch):
    """scores_pair_topk_kernel exactly where dense_mfma_launch_topk launches it: a single slab, n <= 1024, k <= 32,
    nq >= 2, not pinned off — through all three scores kernels."""
    monkeypatch.delenv("AMDR_TOPK_PAIR", raising=False)
    for n in (1024, 1025):
        idx = nat.DenseIndex(np.zeros((n, 64), np.float32))
        for nq in (1, 2, 4, 5, 95, 96, 300):
            for k in (32, 33):
                info = idx.plan_info(nq, k)
                assert ("scores_pair_topk_kernel" in info) == (n <= 1024 and k <= 32 and nq >= 2), (n, nq, k, info)
                assert ("scores_slab_topk_kernel" in info) != ("scores_pair_topk_kernel" in info), info
        monkeypatch.setenv("AMDR_TOPK_PAIR", "0")
        assert _slab_plan(idx.plan_info(7, 10))
        monkeypatch.delenv("AMDR_TOPK_PAIR")
        idx.close()


# ---- C. the staged selector behind the same launch ------------------------------------------------------------------------------
def _staged_columns(n):
    cs = SA.Columns(n)
    for name, col in SA.plain_patterns(n).items():
        cs.add(col, k=None, kind=name)
    cs.add(SA.spread_ties(n), k=None, kind="spread_ties")
    cs.add(np.random.default_rng(n).permutation(n).astype(np.float32) - n // 2, k=None, kind="permutation")
    return cs


@pytest.mark.parametrize("n,ks", [(2048, (65, 191, 192, 193, 256)), (2049, (10, 64, 65, 256)), (4100, (10, 64, 65, 256))])
def test_staged_selector_behind_the_slab_launch(nat, monkeypatch, n, ks):
    """n = 2048, k > 64: one wave, the register selector does not apply.  n > 2048: four waves, each sweeping every
    fourth piece of 256 rows, their lists combined — tie blocks spread over all four waves' pieces."""
    monkeypatch.delenv("AMDR_TOPK_PAIR", raising=False)
    cs = _staged_columns(n)
    refs = Refs(cs, SINGLE)
    (c0, X), = cs.matrices()
    ids = list(range(len(cs.cols)))
    Q = cs.queries(ids)
    idx = nat.DenseIndex(X)
    for k in ks:
        for nq in (len(ids), 1):
            assert _slab_plan(idx.plan_info(nq, k)), idx.plan_info(nq, k)
        s, i = idx.search(Q, k)
        for b, c in enumerate(ids):
            SA.assert_same(s[b], i[b], *refs.expect(c, k), what=(n, k, cs.meta[c]))
        s, i = idx.search(Q[5:6], k)  # the spread ties alone
        SA.assert_same(s[0], i[0], *refs.expect(5, k), what=(n, k, "alone"))
    idx.close()


# ---- D. the other consumers of the selectors: the dense lists only --------------------------------------------------------------
@pytest.mark.parametrize("n", (100, 257, 641, 1024))
def test_fused_search_dense_lists(nat, monkeypatch, n):
    """amdr_dense_search_fuse_device: dense_select_fuse_kernel (AMDR_DENSE_FUSE=1: the pair selector and its staged
    fallback inside the fusion kernel) and the two launches (=0), on the pair selector's crafted rows."""
    import torch
    from legal_rag_amd.retrieval.engine import HybridEngine
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(n)
    cs = SA.case_columns(n, PAIR)
    refs = Refs(cs, PAIR)
    params = nat.make_fuse_params(min_final_score=0.2)
    gave_up = 0
    for c0, X in cs.matrices():
        ids = list(range(c0, min(c0 + cs.d, len(cs.cols))))
        if len(ids) % 2 == 0:
            ids = ids[:-1]  # the last wave holds one query
        nq = len(ids)
        dense = nat.DenseIndex(X, device=0)
        eng = HybridEngine(dense, None, None, device=0)
        q_emb = torch.from_numpy(cs.queries(ids, c0)).to(dev)
        for k, kb in ((5, 10), (10, 10), (16, 16), (31, 1)):
            bs = torch.from_numpy(np.sort(rng.random((nq, kb)) * 30.0, axis=1)[:, ::-1].copy()).to(dev)
            bi = torch.from_numpy(np.stack([rng.permutation(n)[:kb] for _ in range(nq)]).astype(np.int64)).to(dev)
            gave_up += sum(refs.survivors(c, k) > 32 for c in ids)
            for flag in ("1", "0"):
                monkeypatch.setenv("AMDR_DENSE_FUSE", flag)
                dch, _ = eng.dense_topk_fuse(params, q_emb, k, (bs, bi))
                torch.cuda.synchronize()
                refs.check(dch[0].cpu().numpy(), dch[1].cpu().numpy(), ids, k, (n, "fuse", flag))
        monkeypatch.delenv("AMDR_DENSE_FUSE")
        dense.close()
    assert gave_up > 0


@pytest.mark.parametrize("n", (65, 641, 1281, 2048))
def test_one_launch_serving_call_dense_lists(nat, monkeypatch, n):
    """hybrid_small_kernel (HybridEngine.search_batch, 1-4 queries, AMDR_HYBRID_SMALL=1): the single selector on the
    whole row and its staged fallback, on the single selector's crafted rows at their own k (kd + kb = 2 k <= 32)."""
    import torch
    from legal_rag_amd.retrieval.engine import HybridEngine
    from oracle import bm25 as OB
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(n)
    words = [f"w{i}" for i in range(50)]
    ob = OB.BM25Okapi([[words[j] for j in rng.integers(0, 50, size=int(rng.integers(3, 12)))] for _ in range(n)])
    csr = OB.to_csr(ob)
    V = len(csr["vocab"])
    cs = SA.case_columns(n, SINGLE)
    refs = Refs(cs, SINGLE)
    params = nat.make_fuse_params()
    monkeypatch.setenv("AMDR_HYBRID_SMALL", "1")
    gave_up = 0
    for c0, X in cs.matrices():
        eng = HybridEngine(nat.DenseIndex(X), nat.BM25Index(csr["term_ptr"], csr["post_doc"], csr["post_tf"], csr["idf"],
                                                             csr["doc_len"], ob.avgdl, ob.k1, ob.b), None)
        for k in (1, 2, 10, 16):
            ids = [c for c in range(c0, min(c0 + cs.d, len(cs.cols))) if cs.meta[c]["k"] in (None, k)]
            at, nq = 0, 1
            while at < len(ids):
                grp = ids[at:at + nq]
                toks = [[int(t) for t in rng.integers(0, V, size=4)] for _ in grp]
                qt_h, qp_h = nat.BM25Index.pack_queries(toks)
                r = eng.search_batch(params, k, q_emb=torch.from_numpy(cs.queries(grp, c0)).to(dev),
                                     q_terms=torch.from_numpy(qt_h).to(dev), q_ptr=torch.from_numpy(qp_h).to(dev))
                torch.cuda.synchronize()
                refs.check(r.dense_scores.cpu().numpy(), r.dense_ids.cpu().numpy(), grp, k, (n, "one launch", len(grp)))
                gave_up += sum(refs.survivors(c, k) > 64 for c in grp)
                at, nq = at + len(grp), nq % 4 + 1
        eng.dense.close()
        eng.bm25.close()
    assert gave_up > 0 or n < 257


def test_two_level_form_on_the_patterns(nat, monkeypatch):
    """The exact two-level form pinned (AMDR_DENSE_TWO_LEVEL=1, AMDR_DENSE_HI=0) at n = 2048: its top-k passes rank tile
    maxima and re-scored columns (re-mapped to row ids: no survivor model), with the same selectors."""
    monkeypatch.setenv("AMDR_DENSE_TWO_LEVEL", "1")
    monkeypatch.setenv("AMDR_DENSE_HI", "0")
    cs = _staged_columns(2048)
    refs = Refs(cs, SINGLE)
    (c0, X), = cs.matrices()
    ids = list(range(len(cs.cols)))
    idx = nat.DenseIndex(X)
    for k in (1, 10, 17, 32):
        assert "two-level" in idx.plan_info(len(ids), k), idx.plan_info(len(ids), k)
        s, i = idx.search(cs.queries(ids), k)
        for b, c in enumerate(ids):
            SA.assert_same(s[b], i[b], *refs.expect(c, k), what=("two-level", k, cs.meta[c]))
    idx.close()


@pytest.mark.parametrize("n", (257, 640, 1024))
def test_two_pass_small_form_on_the_patterns(nat, monkeypatch, n):
    """The fp16 two-pass form of a long batch (AMDR_DENSE_SMALL_HI_MIN lowered; d = 128, k <= 12): dense_hi_select_fuse_kernel's
    own copy of the pair selector, the exact re-scoring behind it.  Equality with the oracle is required; how many
    queries re-scored their whole row is printed, not asserted."""
    monkeypatch.setenv("AMDR_DENSE_SMALL_HI", "1")
    monkeypatch.setenv("AMDR_DENSE_SMALL_HI_MIN", "96")
    cs = _staged_columns(n)
    cs.d = 128
    refs = Refs(cs, PAIR)
    (c0, X), = cs.matrices()
    ids = [c % len(cs.cols) for c in range(97)]  # 97 queries: the last wave holds one
    idx = nat.DenseIndex(X)
    for k in (1, 10, 12):
        assert idx.plan_info(len(ids), k).startswith("dsh_scores_kernel"), idx.plan_info(len(ids), k)
        before = idx.two_pass_fallbacks()
        s, i = idx.search(cs.queries(ids), k)
        print(f"two-pass small form n={n} k={k}: {idx.two_pass_fallbacks() - before} of {len(ids)} queries re-scored their whole row")
        for b, c in enumerate(ids):
            SA.assert_same(s[b], i[b], *refs.expect(c, k), what=("two-pass", n, k, cs.meta[c]))
    idx.close()


# ---- E. special values ------------------------------------------------------------------------------------------------------------
SCALES = (1.0, 0.5, 0.125, 2.0)  # (x 2: +-FLT_MAX overflow and tie with the infinities)


def _special(nat, n, k, nq, expect=SA.topk_full_order):
    """One column with +-inf, +-FLT_MAX and NaN rows; query b = SCALES[b % 4] x its unit vector."""
    col = SA.special_column(n, np.random.default_rng(n))
    X = np.zeros((n, 64), np.float32)
    X[:, 0] = col
    Q = np.zeros((nq, 64), np.float32)
    Q[:, 0] = [SCALES[b % 4] for b in range(nq)]
    idx = nat.DenseIndex(X)
    info = idx.plan_info(nq, k)
    s, i = idx.search(Q, k)
    idx.close()
    with np.errstate(over="ignore"):
        for b in range(nq):
            SA.assert_same(s[b], i[b], *expect(np.float32(Q[b, 0]) * col, k), what=(n, k, nq, b, info))
    return info


def test_special_values_in_the_full_forms(nat, monkeypatch):
    """NaN ranks behind -inf and ahead of the padding, the lower id first among NaNs and among equal infinities."""
    monkeypatch.setenv("AMDR_TOPK_PAIR", "0")
    for n in (65, 641, 2048):  # A
        for k in (1, 10, 33, 64):
            for nq in (1, 4, 9):
                assert _slab_plan(_special(nat, n, k, nq))
    monkeypatch.delenv("AMDR_TOPK_PAIR")
    for n in (20, 33, 100, 513, 1024):  # B
        for k in (5, 31, 32):
            for nq in (3, 9):
                assert "scores_pair_topk_kernel" in _special(nat, n, k, nq)
    for n, ks in ((2048, (65, 256)), (2049, (10, 256)), (4100, (10, 256))):  # C
        for k in ks:
            for nq in (1, 9):
                assert _slab_plan(_special(nat, n, k, nq))


def test_special_values_in_the_two_level_form(nat, monkeypatch):
    """The two-level form's documented convention: a NaN score is padding."""
    monkeypatch.setenv("AMDR_DENSE_TWO_LEVEL", "1")
    monkeypatch.setenv("AMDR_DENSE_HI", "0")
    for k in (10, 32):
        assert "two-level" in _special(nat, 2048, k, 9, expect=SA.topk_nan_is_padding)

"""The builders of tests/fusion_adversary.py do what the GPU tests rely on (tests/test_fusion_adversary_gpu.py would pass
vacuously otherwise): every route is reached, crafted ties tie, crafted spans fall on their side of 1e-12, the count edges
are hit — and oracle.fusion.fuse's keep_order keyword is pinned against a hand-computed example."""
import math

import numpy as np

import fusion_adversary as FA
from oracle import fusion as F


def test_value_order_is_the_abi_order():
    from legal_rag_amd import _native
    assert _native.FUSE_NVALS == FA.NVALS
    assert [_native.FV[n] for n in ("score", "rrf_norm", "weighted_sum")] == [0, 1, 2]
    assert FA.FV[3:6] == ("dense_norm", "bm25_norm", "colbert_norm") and FA.FV[6:] == ("contrib_dense", "contrib_bm25", "contrib_colbert")
    assert tuple(_native.FUSE_METHODS[m] for m in FA.METHODS) == (0, 1, 2, 3)


def test_every_route_is_reached_and_the_table_holds():
    table = {(5, 5, 5): FA.P16, (8, 8, 0): FA.P16, (10, 0, 0): FA.P16, (10, 7, 0): FA.P32, (10, 10, 10): FA.P32,
             (16, 16, 0): FA.P32, (11, 11, 11): FA.LONG_REG, (32, 32, 0): FA.LONG_REG, (22, 22, 21): FA.LONG_LDS,
             (256, 256, 256): FA.LONG_LDS}
    assert set(table) == set(FA.SHAPES)
    assert [sum(s) for s in FA.SHAPES] == [15, 16, 10, 17, 30, 32, 33, 64, 65, 768]
    seen = set()
    for shape, want in table.items():
        b = FA.mixed_batch(shape)
        u = b.unions()
        assert b.nq == FA.NQ_MAX == 67 and b.kinds[:5] == list(FA.KINDS)
        assert FA.route(b.max_out, u[0]) == want and u[0] == b.max_out  # query 0: disjoint ids, U = max_out (also at nq = 1)
        seen |= b.routes()
        if want == FA.LONG_LDS:  # long lists with a small union take the register branch inside the same launch
            assert FA.LONG_REG in b.routes()
    assert seen == {FA.P16, FA.P32, FA.LONG_REG, FA.LONG_LDS}
    assert {FA.route(sum(s), sum(s)) for s in FA.ROUTE_SHAPES} == seen


def test_mixed_batches_mix_what_a_wave_holds():
    for shape in FA.SHAPES:
        b = FA.mixed_batch(shape)
        for q, (kind, chans) in enumerate(zip(b.kinds, b.lists)):
            lens = [len(c) for c in chans]
            if kind == "disjoint":
                assert lens == list(shape)
            if kind == "empty":
                assert lens == [0, 0, 0]
            if kind == "no_middle":
                assert lens[1] == 0 and lens[0] > 0
            assert all(FA.is_descending(c) for c in chans)
        # the packed layout: -1 tail, garbage (not 0) under it, float32 values in dense / ColBERT
        for c, k in enumerate(shape):
            valid = np.arange(k)[None, :] < np.array([[len(q[c])] for q in b.lists])
            assert ((b.ids[c] >= 0) == valid).all() and (b.ids[c][~valid] == -1).all()
            assert (b.scores[c][~valid] != 0.0).all()
            if c != 1:
                assert (b.scores[c].astype(np.float32).astype(np.float64) == b.scores[c]).all()
        if len([k for k in shape if k]) > 1:
            u = b.unions()
            assert min(u[q] for q in range(b.nq) if b.kinds[q] == "overlap") < b.max_out == max(u)
            ragged = [len(q[0]) for q in b.lists]
            assert len(set(ragged)) > 2
    # a wave of the packed forms needs the LONGEST union among its queries as the bound of the union search
    for shape, per_wave in (((5, 5, 5), 4), ((8, 8, 0), 4), ((10, 7, 0), 2), ((10, 10, 10), 2), ((16, 16, 0), 2)):
        assert FA.needs_the_longest_union(FA.mixed_batch(shape).lists, per_wave), shape
    # every kind sits in every segment
    assert {(q % 4, k) for q, k in enumerate(FA.mixed_batch((5, 5, 5)).kinds)} == {(s, k) for s in range(4) for k in FA.KINDS}


def test_expected_arrays_layout_and_count_edges():
    shape = (10, 10, 10)
    b = FA.mixed_batch(shape)
    ids, vals, mask, count = FA.expected_mixed(shape, "rrf_norm_blend")
    u = b.unions()
    for q in range(b.nq):
        assert (ids[q, :u[q]] >= 0).all() and (ids[q, u[q]:] == -1).all()
        assert (vals[q, u[q]:] == 0.0).all() and (mask[q, u[q]:] == 0).all() and (mask[q, :u[q]] > 0).all()
        assert 0 <= count[q] <= u[q]
        s = vals[q, :u[q], 0]
        assert (s[:-1] >= s[1:]).all() and (s[:count[q]] >= FA.MIN_FINAL).all() and (s[count[q]:] < FA.MIN_FINAL).all()
        pos = FA.union_positions(b.lists[q])
        for r in range(u[q]):
            assert mask[q, r] == sum(1 << c for c in range(3) if any(i == ids[q, r] for i, _ in b.lists[q][c]))
        assert set(pos) == set(ids[q, :u[q]].tolist())
    assert (count == 0).any() and (count < np.array(u)).any() and (count > 0).any()
    # min_final exactly at a candidate's score keeps it, the next double drops it; +inf keeps nothing, -inf everything
    for shape in FA.ROUTE_SHAPES:
        lists = FA.mixed_batch(shape).lists[:5]
        kn = FA.knobs()
        at, above, inf, ninf = FA.min_final_edges(lists, kn)
        c = [FA.expected_arrays(lists, kn, mf, sum(shape))[3] for mf in (at, above, inf, ninf)]
        assert c[0][0] == c[1][0] + 1 and (c[2] == 0).all()
        assert c[3].tolist() == FA.mixed_batch(shape).unions()[:5]


def test_knob_edges_reach_the_branches():
    lists = FA.mixed_batch((10, 10, 10)).lists[:5]
    by_name = dict(FA.KNOB_EDGES)
    # a zero weight under wrrf: candidates whose RRF total is exactly 0
    kn = by_name["wrrf w=(0,0,.35)"]
    totals, _ = F.rrf_with_breakdown({"dense": [i for i, _ in lists[0][0]], "bm25": [i for i, _ in lists[0][1]],
                                      "colbert": [i for i, _ in lists[0][2]]}, k=60,
                                     weights={"dense": 0.0, "bm25": 0.0, "colbert": 0.35})
    assert min(totals.values()) == 0.0 < max(totals.values())
    # the negative weight: a total of exactly 0 with rrf_norm > 0 -> the empty allocation decides (t <= 1e-18, not t < 0)
    kn = by_name["wrrf w=(-.5,0,.35)"]
    hits = F.fuse(*lists[0], kn)
    zero_total = [h for h in hits if h["breakdown"]["channel"] == ["bm25"]]
    assert zero_total and all(h["score"] > 0.0 and set(h["breakdown"]["channel_contrib"].values()) == {0.0} for h in zero_total)
    # all weights 0 under wrrf: every total 0, the RRF norm degenerates
    assert all(h["score"] == 0.0 for h in F.fuse(*lists[0], by_name["wrrf w=(0,0,0)"]))
    assert {kn["rrf_k"] for _, kn in FA.KNOB_EDGES} >= {0, 1, 1000} and {kn["rrf_alpha"] for _, kn in FA.KNOB_EDGES} >= {0.0, 1.0}


def test_value_edges_fall_on_their_side():
    assert FA.SPAN_BELOW < 1e-12 < FA.SPAN_ABOVE
    for shape in FA.ROUTE_SHAPES:
        b = FA.value_edge_batch(shape)
        assert b.nq == 5 and b.kinds == list(FA.VALUE_KINDS)
        for q, kind in enumerate(b.kinds):
            hits = F.fuse(*b.lists[q], FA.knobs())
            norm = {c: [h["breakdown"][f"{c}_norm"] for h in hits] for c in F.CHANNELS}
            spans = [max(s for _, s in ch) - min(s for _, s in ch) for ch in b.lists[q]]
            if kind == "span_below":
                assert spans == [FA.SPAN_BELOW, FA.SPAN_ABOVE, FA.SPAN_BELOW]
                assert set(norm["dense"]) == {0.0} == set(norm["colbert"]) and max(norm["bm25"]) == 1.0
            if kind == "span_above":
                assert spans == [FA.SPAN_ABOVE, FA.SPAN_BELOW, FA.SPAN_ABOVE]
                assert max(norm["dense"]) == 1.0 == max(norm["colbert"]) and set(norm["bm25"]) == {0.0}
                assert 0.0 < sorted(set(norm["dense"]))[1] < 1.0  # (values between the ends)
            if kind == "one_entry":
                assert [len(ch) for ch in b.lists[q]] == [1, 1, 1] and all(set(v) == {0.0} for v in norm.values())
            if kind == "negative":
                assert all(s < 0 for ch in b.lists[q] for _, s in ch) and max(norm["dense"]) == 1.0
            if kind == "flat":
                assert spans == [0.0, 0.0, 0.0] and all(set(v) == {0.0} for v in norm.values())


def test_crafted_ties_tie_in_the_oracle():
    for shape in FA.ROUTE_SHAPES:
        b = FA.tie_batch(shape)
        assert b.kinds[1:4] == ["mirrored", "flat", "disjoint"]  # segments 1..3 of the first <16> wave
        for q, kind in enumerate(b.kinds):
            hits = F.fuse(*b.lists[q], FA.knobs("rrf"))
            groups = FA.tie_groups(hits)
            pos = FA.union_positions(b.lists[q])
            assert groups or kind == "flat", (shape, q, kind)  # (flat ties under weighted_sum, below)
            for g in groups:  # first appearance decides inside a tie
                assert [pos[i] for i in g] == sorted(pos[i] for i in g)
            if kind == "mirrored":
                a0, a1 = b.lists[q][0][0][0], b.lists[q][0][1][0]
                assert [b.lists[q][1][0][0], b.lists[q][1][1][0]] == [a1, a0]
                assert [a0, a1] in [g[:2] for g in groups] and hits[0]["id"] == a0 and hits[1]["id"] == a1
            if kind == "disjoint" and FA.route(b.max_out, len(pos)) == FA.LONG_LDS:
                assert any(len({pos[i] // 64 for i in g}) > 1 for g in groups)  # ties across 64-chunks of the union
            if kind == "flat":
                ws = F.fuse(*b.lists[q], FA.knobs("weighted_sum"))
                assert {h["score"] for h in ws} == {0.0} and [h["id"] for h in ws] == sorted(pos, key=pos.get)
    big = FA.mixed_batch((256, 256, 256))
    pos = FA.union_positions(big.lists[0])
    assert any(len({pos[i] // 64 for i in g}) > 1 for g in FA.tie_groups(F.fuse(*big.lists[0], FA.knobs("rrf"))))


def test_shuffled_lists_and_maps():
    for shape in FA.ROUTE_SHAPES:
        base = FA.mixed_batch(shape).head(8)
        sh = FA.shuffled(base, [1, 6])
        for q in range(8):
            for c in range(3):
                a, s = base.lists[q][c], sh.lists[q][c]
                assert sorted(a) == sorted(s)
                if q in (1, 6) and len(a) >= 2:
                    assert not FA.is_descending(s) and s[0][1] < max(x for _, x in s)
                if q not in (1, 6):
                    assert a == s
        assert any(len(c) >= 2 for q in (1, 6) for c in sh.lists[q])
        # keep_order changes nothing for a descending list, and something for a shuffled one
        kn = FA.knobs()
        assert F.fuse(*base.lists[0], kn) == F.fuse(*base.lists[0], kn, keep_order=True)
        assert F.fuse(*sh.lists[1], kn) != F.fuse(*sh.lists[1], kn, keep_order=True)
        b, maps = FA.map_batch(shape)
        assert all(sorted(m.tolist()) == list(range(len(m))) for m in maps) and not (maps[0] == maps[1]).all()
        ml = FA.mapped_lists(b.lists, maps)
        # different rows of different channels meet at one uid; the same row means different uids
        d, bm = dict(b.lists[0][0]), dict(b.lists[0][1])
        met = [(r0, r1) for r0 in d for r1 in bm if maps[0][r0] == maps[1][r1]]
        assert any(r0 != r1 for r0, r1 in met) and any(maps[0][r] != maps[1][r] for r in set(d) & set(bm))
        assert len(F.fuse(*ml[0], kn)) < sum(shape)
        half = FA.mapped_lists(b.lists, (maps[0], None, maps[2]))
        assert half[0][1] == b.lists[0][1] and half[0][0] != b.lists[0][0]


def test_keep_order_pinned_by_hand():
    """Three ids, dense not descending: with keep_order rank = list position (b first) and min / max still span the list."""
    dense = [("b", 1.0), ("a", 3.0), ("c", 2.0)]
    bm25 = [("c", 10.0), ("a", 10.0)]
    kn = {"fusion_method": "rrf_norm_blend", "rrf_k": 1, "rrf_alpha": 0.5, "dense_weight": 1.0, "bm25_weight": 0.5,
          "colbert_weight": 0.0}
    hits = {h["id"]: h for h in F.fuse(dense, bm25, [], kn, keep_order=True)}
    # RRF totals, k = 1: b = 1/2, a = 1/3 + 1/3, c = 1/4 + 1/2 -> min 1/2 (b), max 3/4 (c)
    t = {"b": 1 / 2, "a": 1 / 3 + 1 / 3, "c": 1 / 4 + 1 / 2}
    for i, h in hits.items():
        sb = h["breakdown"]
        assert sb["rrf_norm"] == (t[i] - 0.5) / (0.75 - 0.5)
        assert sb["dense_norm"] == {"b": 0.0, "a": 1.0, "c": 0.5}[i] and sb["bm25_norm"] == 0.0  # BM25 flat
        assert sb["weighted_sum"] == 1.0 * sb["dense_norm"] + 0.0 + 0.0
        assert h["score"] == 0.5 * sb["rrf_norm"] + 0.5 * sb["weighted_sum"]
    assert [h["id"] for h in F.fuse(dense, bm25, [], kn, keep_order=True)] == ["a", "c", "b"]
    assert (hits["c"]["score"], hits["b"]["score"]) == (0.5 * 1.0 + 0.5 * 0.5, 0.0)
    assert hits["a"]["score"] == 0.5 * ((2 / 3 - 0.5) / 0.25) + 0.5
    # the default re-sorts: a takes rank 1 of dense, and c (first of the BM25 tie) rank 1 of BM25
    srt = {h["id"]: h for h in F.fuse(dense, bm25, [], kn)}
    assert srt["a"]["breakdown"]["rrf_norm"] == ((1 / 2 + 1 / 3) - (1 / 4)) / ((1 / 3 + 1 / 2) - (1 / 4))
    assert F.fuse(sorted(dense, key=lambda p: -p[1]), bm25, [], kn, keep_order=True) == F.fuse(dense, bm25, [], kn)


def test_rerank_builders_hit_the_count_and_top_n_edges():
    for shape in FA.RERANK_SHAPES:
        mo = sum(shape)
        ids, vals, mask, count = FA.rerank_input(shape, "rrf")
        assert count.min() == 0 and count.max() == mo
        if mo > 1:
            u = np.array(FA.mixed_batch(shape).unions())
            assert ((count > 0) & (count < u)).any()
        tn = FA.top_ns(count, mo)
        assert tn[0] == 1 and tn[-1] > mo and mo in tn
        rel = {(t < c, t == c, t > c) for t in tn for c in count if c > 0}
        assert len(rel) == (3 if mo > 1 else 2)
    assert [sum(s) for s in FA.RERANK_SHAPES] == [1, 20, 64, 65, 768]
    ce = FA.ce_scores(10, 8)
    assert len(set(ce[1])) == 1 and ce[2].max() - ce[2].min() == FA.SPAN_BELOW and ce[3].max() - ce[3].min() == FA.SPAN_ABOVE
    assert len(set(ce[4])) < 8 and len(set(ce[0])) == 8
    assert F.minmax(list(ce[2])) == [0.0] * 8 and max(F.minmax(list(ce[3]))) == 1.0


def test_expected_rerank_orders_ties_through_both_sorts():
    """beta = 0 over tied fused scores: the candidates come out by CE norm, the tied tail hit behind them; beta = 1 with
    duplicate CE scores keeps the input order inside a duplicate; rows past count are the input's."""
    mo = 6
    ids = np.arange(100, 100 + mo, dtype=np.int64)[None, :].copy()
    vals = np.zeros((1, mo, FA.NVALS))
    vals[0, :, 0] = [0.5, 0.5, 0.5, 0.5, 0.25, 0.125]
    vals[0, :, 1] = np.arange(mo)  # travels with the id
    mask = np.arange(1, mo + 1, dtype=np.int32)[None, :].copy()
    count = np.array([5], dtype=np.int32)
    ce = np.array([[1.0, 3.0, 2.0]])
    oi, ov, om, rer = FA.expected_rerank(ids, vals, mask, count, ce, 3, 0.0)
    assert oi[0].tolist() == [101, 102, 100, 103, 104, 105]  # CE order 3, 2, 1; the tied tail hit 103 stays behind
    assert ov[0, :, 1].tolist() == [1, 2, 0, 3, 4, 5] and om[0].tolist() == [2, 3, 1, 4, 5, 6]
    assert rer[0, :3].tolist() == [[3.0, 1.0], [2.0, 0.5], [1.0, 0.0]] and np.isnan(rer[0, 3:]).all()
    assert ov[0, :4, 0].tolist() == [0.5] * 4 and ov[0, 5, 0] == 0.125
    oi, ov, om, rer = FA.expected_rerank(ids, vals, mask, count, np.array([[2.0, 2.0, 7.0, 2.0, 0.0, 9.0]]), 9, 1.0)
    assert oi[0].tolist() == [102, 100, 101, 103, 104, 105] and ov[0, :5, 0].tolist() == [1.0, 2 / 7, 2 / 7, 2 / 7, 0.0]
    assert not np.isnan(rer[0, :5]).any() and np.isnan(rer[0, 5]).all() and ov[0, 5, 0] == 0.125
    # a blended candidate that ties exactly with a tail hit: the candidate stays ahead (it precedes in the pre-sort sequence)
    oi, _, _, _ = FA.expected_rerank(ids, vals, mask, count, np.array([[1.0, 3.0]]), 2, 0.0)
    assert oi[0].tolist() == [101, 100, 102, 103, 104, 105]


def test_compact_cases_cover_the_block_edges():
    totals = sorted(nq * w for nq, w in FA.COMPACT_CASES)
    for edge in (256, 512):
        assert edge in totals and any(edge - 3 <= t < edge for t in totals) and any(edge < t <= edge + 3 for t in totals)
    assert {w for _, w in FA.COMPACT_CASES} == {1, 3, FA.COMPACT_MAX_OUT}
    _, _, _, count = FA.compact_record(7)
    assert count.tolist() == [0, 1, 2, 3, 4, 0, 1]

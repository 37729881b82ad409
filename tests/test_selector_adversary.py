"""CPU checks of tests/selector_adversary.py: the model of the register selectors' cut and the rows built to steer it."""
import numpy as np
import pytest

import selector_adversary as SA
from selector_adversary import PAIR, SINGLE


@pytest.mark.parametrize("selector", [SINGLE, PAIR])
def test_lane_maps_are_bijections(selector):
    """(lane, key register) -> row is one-to-one, onto [0, n), inside the V registers the selector compiles for n rows —
    also for a slab of the single selector that does not start at row 0."""
    for n in sorted(set(SA.A_N if selector == SINGLE else SA.B_N) | {2, 129}):
        lane, slot = SA.lane_slot(n, selector)
        assert len(lane) == n and lane.min() >= 0 and lane.max() < SA.LANES[selector]
        assert slot.min() >= 0 and slot.max() < SA.keys_per_lane(n, selector)
        assert len(set(zip(lane.tolist(), slot.tolist()))) == n
        if selector == SINGLE:  # inverse: lo + lane + 64 slot
            assert np.array_equal(lane + 64 * slot, np.arange(n))
        else:  # inverse: 128 (slot // 4) + 4 lane + slot % 4
            assert np.array_equal(128 * (slot // 4) + 4 * lane + slot % 4, np.arange(n))
    lane, slot = SA.lane_slot(1000, SINGLE, lo=192)
    assert np.array_equal(192 + lane + 64 * slot, np.arange(192, 1000))


def test_ord32_orders_like_the_scores():
    x = np.array([-np.inf, -SA.FLT_MAX, -3.0, -0.0, 0.0, 1e-40, 2.0, SA.FLT_MAX, np.inf], np.float32)
    key = SA.ord32(x)
    assert key[3] == key[4] and np.all(np.diff(key.astype(np.int64)) >= 0) and len(set(key.tolist())) == len(x) - 1
    assert SA.ord32(np.float32(np.nan)) == 1 and key.min() > 1


@pytest.mark.parametrize("selector,ns", [(SINGLE, SA.A_N), (PAIR, SA.B_N)])
def test_craft_gives_the_requested_survivors(selector, ns):
    """Every (n, k, S) the GPU file runs: exactly S survivors under the model, distinct integers inside +-VMAX; and the
    set covers both sides of every boundary it is there for."""
    seen = set()
    for n in ns:
        cs = SA.case_columns(n, selector)
        for col, m in zip(cs.cols, cs.meta):
            assert np.all(np.abs(col) <= SA.VMAX) and np.array_equal(col, np.round(col))
            if m["kind"] in ("craft", "all_survive"):
                assert len(set(col.tolist())) == n
                assert SA.survivors(col, m["k"], selector) == m["s"], (n, m)
                seen.add((m["k"], m["s"]) if m["kind"] == "craft" else (0, 0))
                if m["kind"] == "all_survive":
                    assert m["k"] > SA.lanes_populated(n, selector) and m["s"] == n
    slots = SA.SLOTS[selector]
    ks = SA.A_K if selector == SINGLE else SA.B_K
    assert (0, 0) in seen  # (an all_survive row)
    for k in ks:
        want = {k, 16, 17, 32, 33} | ({64, 65, 100} if selector == SINGLE else {40})
        assert {s for kk, s in seen if kk == k} == {s for s in want if s >= k and s - 1 <= 32 * (k - 1)}, k
    if selector == PAIR:  # fewer populated lanes than k: the pair selector always gives up
        for n in (33, 100, 127):
            for k in (31, 32):
                if k > SA.lanes_populated(n, PAIR):
                    assert n > slots and SA.gives_up(np.arange(n, dtype=np.float32), k, PAIR)


def test_model_on_rows_worked_by_hand():
    # 64 distinct values, one per lane: the k-th best is the cut, k survivors
    row = np.random.default_rng(0).permutation(64).astype(np.float32)
    assert [SA.survivors(row, k, SINGLE) for k in (1, 10, 64)] == [1, 10, 64]
    # the period-64 sawtooth: lane l holds the value l in all its V = 10 registers; the cut is lane 64 - k's lowest id, the
    # other rows of that lane are equal scores with higher ids -> (k - 1) V + 1 survivors
    saw = SA.plain_patterns(640)["sawtooth64"]
    assert SA.survivors(saw, 3, SINGLE) == 21 and SA.gives_up(saw, 8, SINGLE) and not SA.gives_up(saw, 7, SINGLE)
    # rows 64 apart share a lane: 64 distinct best scores in lanes 0 and 1 and one in lane 2 -> k = 3 gives up without a tie
    row = np.zeros(2048, np.float32)
    row[:] = -np.arange(2048) - 1.0
    row[0:2048:64] = 1000.0 + np.arange(32)
    row[1:2048:64] = 2000.0 + np.arange(32)
    row[2] = 900.0
    assert SA.survivors(row, 2, SINGLE) == 33 and SA.survivors(row, 3, SINGLE) == 65 and SA.gives_up(row, 3, SINGLE)
    # all equal: the single selector's composites cut at the k-th lowest id, the pair selector keeps every row
    eq = SA.plain_patterns(300)["all_equal"]
    assert SA.survivors(eq, 10, SINGLE) == 10 and SA.survivors(eq, 10, PAIR) == 300
    # the pair map: rows 0-3 share lane 0, row 128 joins them
    row = -np.arange(300, dtype=np.float32)
    assert SA.survivors(row, 1, PAIR) == 1 and SA.survivors(row, 2, PAIR) == 5  # T = row 4's score: rows 0 .. 4
    # fewer populated lanes than k
    assert SA.survivors(np.arange(100, dtype=np.float32), 32, PAIR) == 100
    assert SA.survivors(np.arange(5, dtype=np.float32), 10, SINGLE) == 5
    assert [SA.sort_width(s, SINGLE) for s in (16, 17, 32, 33, 64)] == [16, 32, 32, 64, 64]
    assert [SA.sort_width(s, PAIR) for s in (16, 17, 32)] == [16, 32, 32]


@pytest.mark.parametrize("selector", [SINGLE, PAIR])
def test_oracle_topk_does_not_depend_on_the_lane_placement(selector):
    """The expected result of a crafted row is a function of the (value, id) pairs alone: moving the values to other
    lanes changes the survivor count, not what the oracle returns for the moved rows — and rows of one value class
    exchanged among themselves leave the score list as it is and the ids in ascending order inside the class."""
    rng = np.random.default_rng(5)
    for n, k, s in ((641, 10, 33), (1024, 17, 40), (257, 2, 5)):
        if not SA.realisable(n, k, s, selector):
            continue
        row = SA.craft(n, k, s, selector, rng)
        es, ei = SA.reference(row, k)
        perm = rng.permutation(n)  # row r moves to perm[r]
        moved = np.empty_like(row)
        moved[perm] = row
        ms, mi = SA.reference(moved, k)
        assert np.array_equal(ms, es) and np.array_equal(mi, perm[ei])
        tied = SA.tie_block(row, k)
        ts, ti = SA.reference(tied, k)
        for v in np.unique(ts):
            cls = np.nonzero(tied == v)[0]
            hit = ti[ts == v]
            assert np.array_equal(hit, cls[:len(hit)])  # the lowest ids of the class, ascending
        sw = tied.copy()
        cls = np.nonzero(tied == ts[-1])[0]
        sw[cls] = sw[cls[rng.permutation(len(cls))]]  # a permutation inside a value class is the same row
        assert np.array_equal(SA.reference(sw, k)[1], ti)


def test_references_agree_and_state_the_nan_conventions():
    rng = np.random.default_rng(9)
    for n, k in ((300, 10), (7, 10), (64, 64)):
        col = rng.integers(-50, 50, size=n).astype(np.float32)  # ties, no NaN: the two references are one
        a, b = SA.reference(col, k), SA.topk_full_order(col, k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    col = np.array([1.0, np.nan, -np.inf, np.inf, np.nan, SA.FLT_MAX, -SA.FLT_MAX], np.float32)
    s, i = SA.topk_full_order(col, 9)
    assert i.tolist() == [3, 5, 0, 6, 2, 1, 4, -1, -1] and np.isnan(s[5:7]).all() and np.all(s[7:] == -SA.FLT_MAX)
    s, i = SA.topk_nan_is_padding(col, 7)
    assert i.tolist() == [3, 5, 0, 6, 2, -1, -1] and np.all(s[5:] == -SA.FLT_MAX)
    sp = SA.special_column(300, rng)
    assert np.isnan(sp).sum() == 5 and np.isinf(sp).sum() == 10 and (np.abs(sp) == SA.FLT_MAX).sum() == 10


def test_spread_ties_reach_every_wave():
    for n in (2049, 4100):
        row = SA.spread_ties(n)
        best = np.nonzero(row == 4000.0)[0]
        assert {int(r) // 256 % 4 for r in best[:8]} == {0, 1, 2, 3}
        second = np.nonzero(row == 3000.0)[0]
        assert len(best) + len(second) > 256 and {int(r) // 256 % 4 for r in second[:256 - len(best)]} == {0, 1, 2, 3}
        _, ei = SA.reference(row, 256)
        assert np.array_equal(ei, np.concatenate([best, second])[:256])

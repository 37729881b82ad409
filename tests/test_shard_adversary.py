"""CPU checks of tests/shard_adversary.py: what keeps tests/test_shard_adversary_gpu.py from passing vacuously.  Every item
is counted on the REFERENCE's outputs (the lists the kernel has to return), not on the inputs, and asserted; there is no
tolerance in this file."""
import numpy as np

import shard_adversary as SA
from shard_adversary import F32, F64


def expected_counts(family):
    total = {}
    for case in SA.cases(family):
        for c, (k, dtype) in enumerate(case.chans):
            es, ei = SA.reference_cached(case, c)
            s, _ = SA.kernel_view(es, ei, dtype)
            SA.add_counts(total, SA.edge_counts(case, c, es, s, ei))
    return total


def test_ord64_orders_like_the_scores_and_keeps_key_zero_for_padding():
    x = np.array([-np.inf, -SA.DBL_MAX, -float(SA.FLT_MAX), -3.0, -2.2e-310, -5e-324, -0.0, 0.0, 5e-324, 2.0, SA.DBL_MAX,
                  np.inf])
    key = SA.ord64(x)
    assert key[6] == key[7] and np.all(key[1:] >= key[:-1]) and len(set(key.tolist())) == len(x) - 1
    assert SA.ord64(SA.NAN64) == 1 and SA.ord64(SA.OTHER_NAN64) == 1 and SA.ord64(np.float64(np.nan)) == 1
    assert key.min() > 1  # every number ranks ahead of a NaN, and a NaN ahead of padding (key 0)


def test_channel_order_is_the_order_of_the_keys():
    """the generator sorts with numpy (lexsort on the negated fp64 score); the kernel with ord64 keys: the same order,
    NaNs and both zeros included"""
    rng = np.random.default_rng(5)
    s = rng.choice(np.array([np.nan, SA.NAN64, -0.0, 0.0, 1.0, -np.inf, np.inf, -SA.DBL_MAX, 5e-324, -5e-324]), size=200)
    i = rng.permutation(200).astype(np.int64)
    o = SA.channel_order(s, i)
    key = SA.ord64(s[o]).astype(object)  # python ints: exact comparisons
    pairs = [(-int(k), int(j)) for k, j in zip(key, i[o])]
    assert pairs == sorted(pairs)


def test_every_list_is_what_a_channel_returns():
    """sorted by (score descending, id ascending), local ids, padding (any negative id) only at the tail — the rogue
    variants too"""
    below_minus_one = {f: 0 for f in SA.FAMILIES}
    for case in SA.all_cases():
        assert SA.lists_are_channel_shaped(case), case.name
        assert len(case.offsets) == case.world and len(case.lists) == case.world and min(case.offsets) >= 0
        pad = [(s[i < 0], i[i < 0]) for per_rank in case.lists for s, i in per_rank]
        if case.rogue:  # a large score word, and ids below -1, on padded entries
            assert all(np.all(s == SA.ROGUE_SCORE) for s, _ in pad), case.name
            below_minus_one[case.family] += sum(int((i < -1).sum()) for _, i in pad)
        else:
            assert all(np.all(i == -1) for _, i in pad), case.name
    for f in SA.FAMILIES:
        assert below_minus_one[f] > 0, f
        assert any(not c.rogue for c in SA.cases(f)), f


def test_depth_borders_are_all_there_in_both_dtypes():
    cs = SA.cases("depth")
    pairs = {(c.world, c.chans[0][0]) for c in cs}
    assert set(SA.BORDER_PAIRS) <= pairs
    assert set(SA.TOTALS) <= {w * k for w, k in pairs} and set(SA.KS) <= {k for _, k in pairs}
    for c in cs:
        assert [dt for _, dt in c.chans] == [F32, F64] and c.chans[0][0] == c.chans[1][0]
    paths = {SA.path_of(w, k) for w, k in pairs}
    assert paths == {"one_sort", "two_halves", "staged"}
    # the conditions of shard_merge_kernel / amdr_shard_merge_device, on both sides
    assert SA.path_of(1, 64) == "one_sort" and SA.path_of(65, 1) == "two_halves" and SA.path_of(2, 64) == "two_halves"
    assert SA.path_of(129, 1) == "staged" and SA.path_of(1, 65) == "staged" and SA.path_of(16, 8) == "two_halves"


def test_depth_cases_fill_every_lane_and_every_output_slot():
    """query 0 of a depth case is full on every rank (world * k candidates: no lane holds padding), query 3 has exactly k"""
    for case in SA.cases("depth"):
        for c, (k, _) in enumerate(case.chans):
            assert case.n_valid(c)[0] == case.world * k and case.n_valid(c)[3] == k, case.name
            _, ei = SA.reference_cached(case, c)
            assert np.all(ei[0] >= 0) and np.all(ei[3] >= 0)


def test_short_lists_hit_every_total_on_every_path_from_one_rank_and_from_many():
    seen = set()
    for case in SA.cases("short"):
        (k, _), world = case.chans[0], case.world
        totals = SA.short_totals(world, k)
        for c in range(len(case.chans)):
            nv = case.n_valid(c)
            assert nv.tolist() == [t for t in totals for _ in range(2)], case.name
            _, ei = SA.reference_cached(case, c)
            assert ((ei >= 0).sum(axis=1) == np.minimum(nv, k)).all()
            for j, t in enumerate(totals):
                per_rank = lambda q: np.array([(case.lists[r][c][1][q] >= 0).sum() for r in range(world)])
                long_, thin = per_rank(2 * j), per_rank(2 * j + 1)
                assert (long_ > 0).sum() == -(-t // k) and thin.max() <= 2 and (thin > 0).sum() == min(t, world)
        seen.add(SA.path_of(world, k))
        if SA.path_of(world, k) == "staged":
            assert {63, 64, 65} <= set(totals)
    assert seen == {"one_sort", "two_halves", "staged"}
    staged = [c for c in SA.cases("short") if SA.path_of(c.world, c.chans[0][0]) == "staged"]
    assert any(c.chans[0][0] > 64 for c in staged) and any(c.chans[0][0] <= 64 for c in staged)
    n = expected_counts("short")
    assert n["row_empty"] and n["row_short"] and n["row_exactly_k"] and n["row_k_plus_1"]


def test_value_edges_are_in_the_expected_outputs():
    n = expected_counts("values")
    for key in ("nan_hit", "zero_pair_in_id_order", "pad_valued_hit", "inf_hit", "subnormal_hit", "tie", "row_short",
                "row_exactly_k"):
        assert n[key] > 0, (key, n)
    for case in SA.cases("values"):
        for c, (k, dtype) in enumerate(case.chans):
            es, ei = SA.reference_cached(case, c)
            s, nan = SA.kernel_view(es, ei, dtype)
            hit = ei >= 0
            # query 0: both NaNs, of different payloads and from different ranks, close the hits; padding follows
            assert nan[0].sum() == 2 and hit[0].sum() == k - 1 and nan[0, k - 3:k - 1].all(), case.name
            a, b = ei[0, k - 3], ei[0, k - 2]
            assert a < b and len({bytes(es[0, k - 3]), bytes(es[0, k - 2])}) == 2
            # queries 1 and 2: the zero pair, adjacent, the lower id first whichever sign it carries
            for q, first_negative in ((1, True), (2, False)):
                z = np.nonzero(es[q] == 0)[0]
                assert len(z) == 2 and z[1] == z[0] + 1 and ei[q, z[0]] < ei[q, z[1]]
                assert bool(np.signbit(es[q, z[0]])) == first_negative and bool(np.signbit(es[q, z[1]])) != first_negative
                assert np.all(SA.bits(s[q, z]) == 0)  # ... and both come back as +0.0
            # query 3: +inf leads, -inf is the last hit; query 4: a hit with the padding's score, then real padding
            assert es[3, 0] == np.inf and es[3, k - 2] == -np.inf and ei[3, k - 2] >= 0 and ei[3, k - 1] == -1
            assert s[4, k - 3] == -SA.fmax(dtype) and ei[4, k - 3] >= 0 and ei[4, k - 2] == -1 and s[4, k - 2] == s[4, k - 3]
            # query 5: subnormals of both signs either side of the zero
            tiny = np.finfo(dtype).tiny
            sub = np.nonzero((np.abs(es[5]) < tiny) & (es[5] != 0))[0]
            assert len(sub) == 4 and (es[5, sub[:2]] > 0).all() and (es[5, sub[2:]] < 0).all() and es[5, sub[1] + 1] == 0
            # query 6: five values over world * k candidates; query 7: exactly k candidates, every slot a hit
            assert len(set(es[6].tolist())) <= 5 and case.n_valid(c)[6] == case.world * k
            assert case.n_valid(c)[7] == k and hit[7].all() and np.isnan(es[7, k - 1]) and es[7, k - 2] == -SA.fmax(dtype)
    assert {SA.path_of(c.world, c.chans[0][0]) for c in SA.cases("values")} == {"one_sort", "two_halves", "staged"}


def test_wide_ids_are_ordered_by_the_high_word_in_the_expected_outputs():
    per_variant = {}
    for case in SA.cases("wide"):
        variant = case.name.split("-")[1]
        n = per_variant.setdefault(variant, {})
        for c, (k, dtype) in enumerate(case.chans):
            es, ei = SA.reference_cached(case, c)
            s, _ = SA.kernel_view(es, ei, dtype)
            SA.add_counts(n, SA.edge_counts(case, c, es, s, ei))
    assert set(per_variant) == set(SA.WIDE_VARIANTS)
    for variant, n in per_variant.items():
        assert n["id_ge_2_32"] > 0, variant
    assert per_variant["high"]["tie_high_word_only"] > 0        # equal low words: only the high word tells them apart
    assert per_variant["high_rev"]["tie_low_words_reversed"] > 0  # the low words alone would order them the wrong way
    assert per_variant["high_perm"]["tie_high_word_only"] > 0
    assert per_variant["at_2_40"]["tie"] > 0
    # a block across 2^32: hits on both sides of the word boundary in one list
    for case in SA.cases("wide"):
        if "across_2_32" in case.name:
            _, ei = SA.reference_cached(case, 0)
            assert (ei[ei >= 0] < (1 << 32)).any() and (ei >= (1 << 32)).any()
    assert {SA.path_of(c.world, c.chans[0][0]) for c in SA.cases("wide")} == {"one_sort", "two_halves", "staged"}


def test_layouts_cover_channel_counts_orders_and_last_block_waves():
    cs = SA.cases("layouts")
    assert {len(c.chans) for c in cs} == {1, 2, 3, 4}
    assert {c.nq for c in cs} == {1, 2, 3, 5, 53}
    assert {(c.nq * len(c.chans)) % 4 for c in cs} == {0, 1, 2, 3}  # waves in the last block of four
    two = [[SA.path_of(c.world, k) for k in c.ks] for c in cs if len(c.chans) == 2]
    assert ["one_sort", "staged"] in two and ["staged", "one_sort"] in two  # shallow beside deep, both orders
    assert any({dt for _, dt in c.chans} == {F32, F64} for c in cs)
    assert any(len(set(c.ks)) == len(c.ks) == 4 for c in cs)


def test_the_union_of_all_cases_holds_every_edge():
    total = {}
    for f in SA.FAMILIES:
        SA.add_counts(total, expected_counts(f))
    for key in ("nan_hit", "zero_pair_in_id_order", "pad_valued_hit", "id_ge_2_32", "tie_high_word_only", "row_short",
                "row_empty", "row_exactly_k"):
        assert total[key] > 0, (key, total)

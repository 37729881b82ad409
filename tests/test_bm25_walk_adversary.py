"""The data of tests/bm25_walk_adversary.py is what it claims (CPU only), so that the GPU tests built on it cannot pass
vacuously: every case's edge is evaluated on its arrays, every wrong restatement of the walk (a wrong order, a folded
repeat, a fused multiply-add, a dropped token, a border off by one) changes the top k of the cases built to catch it, no
case is caught by no model, no partial sum leaves the safe range, and the numpy reference is tied to oracle/bm25.py."""
import collections

import numpy as np
import pytest

import bm25_image_adversary as IA
import bm25_walk_adversary as WA

# what each family must catch (W5 keeps every posting factor at 1.0, so its products are exact and a fused multiply-add
# computes the same bits: the test below asserts that too, instead of listing a model that cannot differ)
MUST_CATCH = {
    "W1": {"term-order", "fold-repeats", "fma", "pairwise"},
    "W2": {"term-order", "fold-repeats", "fma", "pairwise"},
    "W3": {"term-order", "fold-repeats", "fma", "pairwise", "drop-33rd", "stop-at-empty-group"},
    "W4": {"term-order", "fold-repeats", "fma", "pairwise", "hi-counted", "lo-left-out"},
    "W5": {"term-order", "fold-repeats", "pairwise", "negative-zero-last"},
}


@pytest.fixture(scope="module")
def cases():
    return WA.all_cases()


def _groups(cases):
    """One case per (index, query list): the cases of a group differ in k only."""
    seen, out = set(), []
    for c in cases:
        if (id(c.csr), id(c.queries)) not in seen:
            seen.add((id(c.csr), id(c.queries)))
            out.append(c)
    return out


@pytest.mark.parametrize("family", WA.FAMILIES)
def test_every_case_reaches_its_edge(cases, family):
    mine = [c for c in cases if c.family == family]
    assert mine and {c.k for c in mine} == set(WA.DEPTHS)
    said = collections.OrderedDict()
    for c in mine:
        assert c.n <= 4200 and c.edge
        said.setdefault((c.group, c.n, c.edge), []).append((c.k, c.reached(c)))
    for (group, n, edge), found in said.items():
        texts = sorted({t for _, t in found})
        print(f"{family} {group} n={n}: {edge}\n    " + "\n    ".join(texts))


def test_the_families_hold_what_the_walk_has_edges_for(cases):
    c1 = next(c for c in cases if c.family == "W1")
    lens = {WA._len_of(c1.csr, t) for t in range(c1.csr["idf"].shape[0])}
    assert set(WA.LENGTHS) <= lens and len(WA.slabs_of(WA.W1_N, 1)) == len(WA.slabs_of(WA.W1_N, 256)) == 1
    assert {len(q) for c in cases if c.family == "W3" and c.group == "all-kept" for q in c.queries} == set(WA.TOKEN_COUNTS)
    assert set(WA.W4_N) >= {2049, 4097, 4100} and any(n <= 2048 and n % 16 for n in WA.W4_N)
    for n in WA.W4_N:  # a shallow plan of <= 2 048 documents per slab and a deep one of <= 4 096
        assert IA.bm_plan(n, 10)[0] <= 2048 and IA.bm_plan(n, 10)[2] and not IA.bm_plan(n, 256)[2]
    assert len(WA.slabs_of(4097, 10)) == 3 and len(WA.slabs_of(4097, 256)) == 2 and len(WA.slabs_of(2049, 10)) == 2
    # the four rankings behind the walk: bm25_select_f32 (arg-max plan, k <= 64, unless switched off), the arg-max rounds
    # alone at k = 65 ... 96, and the staged selector
    kinds = collections.Counter()
    for c in cases:
        _, _, argmax = IA.bm_plan(c.n, c.k)
        kinds["select / arg-max" if argmax and c.k <= 64 else "96-deep arg-max" if argmax else "staged"] += 1
    print(dict(kinds))
    assert kinds["select / arg-max"] >= 100 and kinds["staged"] >= 100 and kinds["96-deep arg-max"] >= 12
    assert {c.family for c in cases if c.k > 64 and IA.bm_plan(c.n, c.k)[2]} == {"W3", "W4", "W5"}  # (W1, W2 need n > 1 000)
    for c in cases:
        slabs, path = IA.plan_text(c.n, c.k)
        assert slabs.startswith(f"slabs={len(WA.slabs_of(c.n, c.k))} of") and path in (IA.ARGMAX, IA.STAGED)


def test_values_make_the_order_visible(cases):
    for c in _groups(cases):
        idf, w = c.csr["idf"], IA.posting_factor(c.csr)
        assert np.all(np.isfinite(idf)), c.name
        if c.family == "W5":
            assert np.all(w == 1.0)
            continue
        nz = idf[idf != 0.0]
        e = np.frexp(np.abs(nz))[1]
        assert e.min() <= -2 and e.max() >= 38 and (nz > 0).any() and (nz < 0).any(), c.name
        assert np.mean(w == 1.0) < 0.05 and len(set(w.tolist())) > 50, c.name
        m = np.frexp(np.abs(nz))[0]
        assert np.mean((m * 2.0 ** 53) % 2.0 ** 20 != 0) > 0.9, c.name  # mantissas that use their low bits
        s = np.sort(np.abs(nz))
        assert np.any((np.diff(s) > 0) & (np.diff(s) < s[:-1] * 2.0 ** -30)), c.name  # a near-cancelling pair
    spread = np.concatenate([c.csr["idf"] for c in _groups(cases) if c.family in ("W1", "W2", "W3")])
    e = np.frexp(np.abs(spread[spread != 0]))[1]
    assert e.min() <= -28 and e.max() >= 40


def test_the_restated_walk_is_the_reference(cases):
    for c in _groups(cases):
        rows = IA.ref_scores(c.csr, c.queries)
        for k in (10, 256):
            for qi in range(0, len(c.queries), 3):
                got = WA.model_scores(c.csr, c.queries[qi], WA.slabs_of(c.n, k))
                assert np.array_equal(got.view(np.uint64), rows[qi].view(np.uint64)), (c.name, qi, k)


@pytest.mark.parametrize("family", WA.FAMILIES)
def test_wrong_models_change_the_top_k(cases, family):
    mine = [c for c in cases if c.family == family]
    hits = collections.Counter()
    for c in mine:
        assert c.catches, f"{c.name} is built to catch no model"
        assert set(c.catches) <= set(WA.MODELS)
        for model in c.catches:
            qi = WA.caught(c, model)
            assert qi is not None, f"{c.name}: the model '{model}' returns the reference's top {c.k} for every query"
            hits[model] += 1
    print(f"{family}: {len(mine)} cases, wrong models caught: " + ", ".join(f"{m} {hits[m]}" for m in WA.MODELS if hits[m]))
    assert {m for m in hits} >= MUST_CATCH[family], (family, dict(hits))
    for k in WA.DEPTHS:  # at every depth
        at_k = set().union(*(c.catches for c in mine if c.k == k))
        need = {m for m in MUST_CATCH[family] if m not in WA.BORDER_MODELS or any(WA.applicable(c, m) for c in mine if c.k == k)}
        assert at_k >= need, (family, k, need - at_k)
    if family == "W4":  # a border model is asked of every plan that has a border, and only there
        for c in mine:
            if c.group == "borders":
                assert (WA.bm_plan(c.n, c.k)[1] > 1) == ("hi-counted" in c.catches) == ("lo-left-out" in c.catches), c.name
    if family == "W5":  # factor 1.0: the products are exact, a fused multiply-add changes nothing
        for c in mine[::len(WA.DEPTHS)]:
            for qi in range(len(c.queries)):
                assert np.array_equal(WA.model_row(c, qi, "fma").view(np.uint64), WA.model_row(c, qi, None).view(np.uint64))


def test_every_model_is_caught_somewhere():
    assert set().union(*MUST_CATCH.values()) == set(WA.MODELS)


def test_partial_sums_stay_far_from_the_sentinels(cases):
    worst = 0.0
    for c in _groups(cases):
        w, tp, pd, idf = IA.posting_factor(c.csr), c.csr["term_ptr"], c.csr["post_doc"], c.csr["idf"]
        for q in c.queries:
            row = np.zeros(c.n)
            for t in q:
                if 0 <= t < idf.shape[0]:
                    row[pd[tp[t]:tp[t + 1]]] += idf[t] * w[tp[t]:tp[t + 1]]
                    assert np.all(np.isfinite(row))
                    worst = max(worst, float(np.abs(row).max()))
    print(f"largest partial sum: 2^{np.log2(worst):.1f}")
    assert worst < WA.LIMIT


def test_zero_sums_are_positive_zero(cases):
    """x + y is -0.0 only for x = y = -0.0 and the accumulator starts at +0.0: whatever cancels, and whatever product is
    -0.0, the raw score is +0.0.  The reference shows it on the W5 data; the GPU test compares the sign bit too."""
    products = 0
    for c in _groups([c for c in cases if c.family == "W5"]):
        rows = IA.ref_scores(c.csr, c.queries)
        assert not np.any(np.signbit(rows) & (rows == 0.0))
        products += int(np.sum(np.signbit(c.csr["idf"]) & (c.csr["idf"] == 0.0)))
    assert products >= 2 and -0.0 + 0.0 == 0.0 and not np.signbit(np.float64(0.0) + np.float64(-0.0))


def test_the_reference_agrees_with_the_oracle_on_ordinary_text():
    from conftest import load_golden
    from oracle import bm25 as OB
    g = load_golden("bm25_toy.json")
    docs = [OB.tokenize_en(t) for t in g["docs"]]
    rng = np.random.default_rng(3)
    words = sorted({w for d in docs for w in d})
    docs += [[words[j] for j in rng.integers(0, len(words), size=int(rng.integers(3, 25)))] for _ in range(60)]
    ob = OB.BM25Okapi(docs)
    csr = OB.to_csr(ob)
    csr.update(avgdl=ob.avgdl, k1=ob.k1, b=ob.b)
    queries = [c["tokens"] for c in g["queries"]] + [[words[j] for j in rng.integers(0, len(words), size=n)] for n in (1, 7, 33, 70)]
    queries.append([words[2], "zzz", words[2], words[5], "qqq"])
    tids = [[csr["vocab"].get(t, -1) for t in q] for q in queries]
    rows = IA.ref_scores(csr, tids)
    for q, row in zip(queries, rows):
        assert np.array_equal(row.view(np.uint64), ob.get_scores(q).view(np.uint64)), q
    assert np.count_nonzero(rows) > 100


def test_the_scopes_of_the_twin():
    for n in (1100, 4097):
        B = WA.borders_of(n)
        lists = WA.scope_lists(n, B)
        assert {len(r) for r in lists} >= {n, (n + 1) // 2, 0, 1, 64, 65, 1024, 1025}
        assert all(np.all(np.diff(r) > 0) for r in lists)
        if B:
            assert set(lists[2].tolist()) == {d for b in B for d in range(b - 8, b + 8)}
    row = np.array([0.5, -0.0, 3.0, 0.0, 3.0, -1.0])
    ids, sc = WA.ref_scoped_topk(row, np.array([1, 3, 4, 5]), 5)
    assert ids.tolist() == [4, 1, 3, 5, -1] and sc[:4].tolist() == [3.0, 0.0, 0.0, -1.0] and not np.signbit(sc[1])

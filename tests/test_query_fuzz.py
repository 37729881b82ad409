"""The host side of the mixed-expression differential test (tests/query_fuzz_cases.py): the certificates of the corpus, the
batches and the directed tables; that six deliberately wrong evaluators each change the expected tables, so the inputs tell
a subtly wrong resolver from a right one; Terms.matches against the plain evaluator on every document; and pack()'s
invariants against the evaluator — bounds, drivers, placeholder ids, list_item, equal items stored once, folded items — on
the base corpus and after each edit round of the live-index test, on the host model alone."""
import time

import numpy as np
import pytest

import query_fuzz_cases as Q
from legal_rag_amd.retrieval.terms import Near, NearOf, OneOf, Phrase, PhraseOf, Prefix, Terms, pack


@pytest.fixture(scope="module")
def ev():
    return Q.base_evaluator()


@pytest.fixture(scope="module")
def batches():
    return [Q.random_batch(seed) for seed in Q.BATCH_SEEDS]


@pytest.fixture(scope="module")
def everything(batches):
    return [t for kept, _ in batches for t in kept]


def test_the_corpus_holds_what_the_cases_say():
    Q.corpus_certificates()
    Q.scoped_certificates()
    Q.edit_certificates(Q.edit_rounds(Q.world()[1]))


def test_holds_on_hand_made_documents():
    """The evaluator itself, on documents small enough to check by eye (docstrings of terms.py)."""
    h = Q.holds
    d = "x a b a c y".split()
    assert h(Phrase("a", "b"), d) and not h(Phrase("b", "c"), d) and h(Phrase("c", "y"), d) and not h(Phrase("y", "x"), d)
    assert h(Phrase("y"), d) and not h(Phrase("a", "b"), ["a"]) and not h(Phrase("a", "b"), [])
    assert h(Near("a", "c", distance=1), d) and h(Near("c", "a", distance=1), d) and not h(Near("b", "c", distance=1), d)
    assert h(Near("b", "c", distance=2), d) and not h(Near("c", "b", distance=2, ordered=True), d)
    assert h(Near("a", "a", "b", distance=2), d) and not h(Near("a", "a", "b", distance=1), d)  # two a and one b in one run
    assert not h(Near("b", "b", distance=5), d) and h(Near("x", "y", distance=5), d) and not h(Near("x", "y", distance=4), d)
    assert h(Near("a", "a", distance=2, ordered=True), d) and not h(Near("a", "a", distance=1, ordered=True), d)
    assert h(Prefix("a"), ["ab"]) and not h(Prefix("ab"), ["a"]) and h(OneOf("q", Prefix("c")), d) and not h(OneOf("q"), d)
    sel = "the seller sells goods".split()
    assert h(PhraseOf(Prefix("sell"), Prefix("sell")), sel) and not h(PhraseOf(Prefix("sell"), "goods", "x"), sel)
    assert h(PhraseOf(OneOf("a", "the"), Prefix("sel")), sel) and not h(PhraseOf("goods", Prefix("sel")), sel)
    assert h(NearOf(Prefix("sell"), Prefix("sell"), distance=1), sel)  # two DISTINCT positions
    assert not h(NearOf(Prefix("sell"), Prefix("sell"), distance=1), "the seller goods".split())
    assert h(NearOf(Prefix("sell"), Prefix("sell"), distance=1), "the seller goods".split(), wrong="somewhere")
    assert h(NearOf("seller", Prefix("sell"), distance=3), sel) and not h(NearOf("seller", Prefix("sell"), distance=3), ["seller"])
    assert h(NearOf("goods", Prefix("sel"), distance=2), sel) and not h(NearOf("goods", Prefix("sel"), distance=2, ordered=True), sel)
    assert h(NearOf(Prefix("sel"), "goods", distance=2, ordered=True), sel)
    assert not h(NearOf(Prefix("sel"), "goods", distance=1, ordered=True), "seller x goods".split())
    # a window ends with its document
    assert not h(Phrase("a", "b"), ["a"], ()) and h(Phrase("a", "b"), ["a"], ["b"]) and not h(Phrase("a", "b"), ["x"], ["a", "b"])
    assert h(Near("a", "b", distance=3), ["a", "x"], ["x", "b"]) and not h(Near("a", "b", distance=3), ["a", "x"])


def test_the_batches_reach_every_resolver_on_both_sides_of_a_tile(ev, batches, everything):
    t0 = time.perf_counter()
    fresh = Q.Evaluator(Q.world()[1])
    ptr = Q.expected_table([(None, t) for t in batches[0][0]], fresh)[0]
    print(f"the evaluator on one batch of {len(batches[0][0])} expressions, nothing cached: {time.perf_counter() - t0:.2f} s")
    assert ptr[-1] > 0
    sizes = []
    for kept, dropped in batches:
        pairs = [(None, t) for t in kept]
        tt = Q.pack_base(pairs)
        ptr, rows, qscope, cons = Q.expected_table(pairs, ev)
        assert np.array_equal(qscope, tt.qscope) and len(cons) == tt.n_cons
        assert min(tt.n_phr, tt.n_near, tt.n_union, tt.n_cspan) >= 20, (tt.n_phr, tt.n_near, tt.n_union, tt.n_cspan)
        print("items per kind", tt.n_phr, tt.n_near, tt.n_union, tt.n_cspan, "refused", len(dropped))
        sizes.append(np.diff(ptr))
    sizes = np.concatenate(sizes)
    share = lambda m: float(np.mean(m))  # noqa: E731
    print(f"neither empty nor full {share((sizes > 0) & (sizes < Q.N_DOCS)):.2f}, longer than a tile {share(sizes > Q.TILE):.2f}, "
          f"empty {share(sizes == 0):.2f}")
    assert share((sizes > 0) & (sizes < Q.N_DOCS)) >= 0.5 and share(sizes > Q.TILE) >= 0.2 and share(sizes == 0) <= 0.4
    assert (sizes > 2 * Q.TILE + 1).any() and (sizes == Q.N_DOCS).any()
    # every kind and every edge member the generator is to draw
    members = [m for t in everything for _, g in t.groups() for m in g]
    for kind in (str, Phrase, Near, Prefix, OneOf, PhraseOf, NearOf):
        assert sum(isinstance(m, kind) for m in members) >= 20, kind
    assert Q.UNKNOWN in members and Prefix(Q.NO_STEM) in members
    assert any(isinstance(m, Near) and len(set(m.tokens)) < len(m.tokens) for m in members)
    assert any(isinstance(m, NearOf) and len(set(m.members)) < len(m.members) and not m.ordered for m in members)
    plain = lambda m: all(isinstance(s, str) for s in m.members)  # noqa: E731
    assert any(isinstance(m, PhraseOf) and plain(m) for m in members) and any(isinstance(m, NearOf) and plain(m) for m in members)
    assert {m.distance for m in members if isinstance(m, (Near, NearOf))} == set(Q.DISTANCES)
    assert {m.ordered for m in members if isinstance(m, Near)} == {m.ordered for m in members if isinstance(m, NearOf)} == {True, False}
    assert any(len(g) == 3 for t in everything for _, g in t.groups()) and any(len(t.groups()) >= 5 for t in everything)
    # (a Phrase of one token and a OneOf of one member are that token in a Terms: the generator's own draws hold them)
    rng = np.random.default_rng(Q.BATCH_SEEDS[0])
    g = Q.Grammar(Q.world()[1])
    drawn = [g.member(rng, kind) for kind in ("Phrase", "OneOf") for _ in range(80)]
    assert any(isinstance(m, Phrase) and len(m) == 1 for m in drawn) and any(isinstance(m, OneOf) and len(m) == 1 for m in drawn)


def test_pack_refuses_exactly_the_unordered_near_ofs_with_overlapping_unequal_slots(batches):
    _, _, vocab, df = Q.world()
    dropped = [t for _, d in batches for t in d]
    assert dropped
    for t in dropped:
        assert Q.overlapping_pair(t, Q.VOCAB), t
        with pytest.raises(ValueError, match="overlapping, unequal"):
            pack([(None, t)], vocab, df, Q.N_DOCS)
    for kept, _ in batches:
        assert not any(Q.overlapping_pair(t, Q.VOCAB) for t in kept)


@pytest.mark.parametrize("wrong", Q.WRONG)
def test_a_wrong_evaluator_changes_the_expected_tables(ev, everything, wrong):
    """What a resolver with this mistake would return differs from the expected table for at least five constraints."""
    bad = Q.Evaluator(Q.world()[1], wrong, ev)
    changed = 0
    for t in everything:
        changed += not np.array_equal(bad.terms_docs(t), ev.terms_docs(t))
        if changed >= 5:
            break
    assert changed >= 5, (wrong, changed)


def test_terms_matches_is_the_evaluator_on_every_document(ev, everything):
    words = Q.world()[1]
    for t in everything:
        want = ev.terms_docs(t)
        for d, ws in enumerate(words):
            assert t.matches(ws) == want[d], (t, d, " ".join(ws))


def test_holds_without_the_cache_is_the_cached_evaluator(ev, batches):
    """`Evaluator.docs` hands `holds` the fillers and skips documents that lack one: the same answers as `holds` alone."""
    words = Q.world()[1]
    some = list(range(0, Q.N_DOCS, 11))
    for m in list(ev.kept)[::7]:
        got = ev.docs(m)
        for d in some:
            assert Q.holds(m, words[d]) == got[d], (m, d)


# ---- pack() against the evaluator ---------------------------------------------------------------------------------------------
def item_bound(item, vocab, df, n_docs) -> int:
    """The upper bound pack() gives one item: the driver of the constraint that has it as its only MUST term."""
    return int(pack([(None, Terms(all_of=[item]))], vocab, df, n_docs).driver_lens[0])


def check_pack(pairs, ev, vocab, df, n_docs, base_rows=None):
    tt = pack(pairs, vocab, df, n_docs, base_rows=base_rows)
    ptr, rows, qscope, cons = Q.expected_table(pairs, ev, base_rows)
    n_vocab = len(vocab)
    # the constraints: one per distinct pair; the drivers bound the rows; rows_cap is their sum
    assert tt.n_cons == len(cons) and np.array_equal(tt.qscope, qscope)
    assert np.all(tt.driver_lens >= np.diff(ptr)), [repr(cons[c][1]) for c in np.flatnonzero(tt.driver_lens < np.diff(ptr))]
    assert tt.rows_cap == int(tt.driver_lens.sum()) and tt.cand_max == int(tt.driver_lens.max())
    # the items: list i is the evaluator's list of list_item(i); every bound holds; the caps are their sums
    kinds = [(tt.n_phr, Phrase), (tt.n_near, Near), (tt.n_union, (Prefix, OneOf)), (tt.n_cspan, (PhraseOf, NearOf))]
    bounds, i = [], 0
    for count, cls in kinds:
        part = []
        for _ in range(count):
            item = tt.list_item(i)
            assert isinstance(item, cls), (i, item)
            b = item_bound(item, vocab, df, n_docs)
            assert b >= int(ev.docs(item).sum()), (item, b)
            part.append(b)
            i += 1
        bounds.append(part)
    assert tt.phr_rows_cap == sum(bounds[0]) and tt.phr_cand_max == max(bounds[0], default=0)
    assert tt.near_rows_cap == sum(bounds[1]) and tt.near_cand_max == max(bounds[1], default=0)
    assert tt.union_rows_cap == sum(bounds[2])
    assert tt.cspan_rows_cap == sum(bounds[3]) and tt.cspan_cand_max == max(bounds[3], default=0)
    # the placeholder ids: phrases, Nears, unions, class spans behind the vocabulary, in that order
    first = {Phrase: n_vocab, Near: n_vocab + tt.n_phr, "u": n_vocab + tt.n_phr + tt.n_near,
             "c": n_vocab + tt.n_phr + tt.n_near + tt.n_union}
    grp_ptr, _, grp_term_ptr, grp_terms = tt.ops[:4]
    folded = shared = 0
    items = [tt.list_item(x) for x in range(i)]
    for c, (_, terms) in enumerate(cons):
        groups = terms.groups()
        assert grp_ptr[c + 1] - grp_ptr[c] == len(groups)
        for gi, (_, g) in enumerate(groups, int(grp_ptr[c])):
            ids = grp_terms[grp_term_ptr[gi]:grp_term_ptr[gi + 1]]
            assert len(ids) == len(g)
            for t, m in zip(ids.tolist(), g):
                if isinstance(m, str):
                    assert t == vocab.get(m, -1)
                    continue
                want = ev.docs(m)
                if t < n_vocab:  # a Prefix or a OneOf that names one token or none
                    assert isinstance(m, (Prefix, OneOf)) and (t >= 0 or not want.any())
                    assert t < 0 or np.array_equal(want, ev.docs(next(w for w, x in vocab.items() if x == t)))
                    continue
                item = items[t - n_vocab]
                assert np.array_equal(ev.docs(item), want), (m, item)
                if isinstance(m, (Phrase, Near)):
                    assert item == m and t == first[type(m)] + (tt.phrases if isinstance(m, Phrase) else tt.nears).index(m)
                elif isinstance(m, (Prefix, OneOf)):
                    assert first["u"] <= t < first["c"]
                    shared += item != m
                elif t < first["u"]:  # a PhraseOf / NearOf of plain slots: the plain item's list
                    assert isinstance(item, Phrase if isinstance(m, PhraseOf) else Near)
                    folded += 1
                else:
                    assert t >= first["c"] and isinstance(item, type(m))
    # a class span's slots name union lists where the union step writes them
    c_ptr, c_slots = tt.cspan_ops[0], tt.cspan_ops[1]
    for k in range(tt.n_cspan):
        obj = tt.cspans[k]
        for s, m in zip(c_slots[c_ptr[k]:c_ptr[k + 1]].tolist(), obj.members):
            if s >= n_vocab:
                assert first["u"] <= s < first["c"] and np.array_equal(ev.docs(items[s - n_vocab]), ev.docs(m)), (obj, m)
            else:
                assert (s < 0 and not ev.docs(m).any()) or np.array_equal(ev.docs(m), ev.docs(next(w for w, x in vocab.items() if x == s)))
    return tt, folded, shared


def test_pack_keeps_its_invariants_on_every_batch(ev, batches):
    corpus, _, vocab, df = Q.world()
    folded = shared = 0
    for kept, _ in batches:
        tt, f, s = check_pack([(None, t) for t in kept], ev, vocab, df, corpus.n_docs)
        folded, shared = folded + f, shared + s
        assert len(set(tt.unions)) == tt.n_union and len(set(tt.cspans)) == tt.n_cspan
    assert folded >= 1 and shared >= 1  # a folded PhraseOf / NearOf; equal items written differently, stored once
    print("folded", folded, "members that share another member's union", shared)


def test_pack_keeps_its_invariants_with_base_scopes_and_in_every_directed_table(ev):
    corpus, _, vocab, df = Q.world()
    tt, _, _ = check_pack(Q.scoped_pairs(), ev, vocab, df, corpus.n_docs, Q.rows_of_scope)
    assert tt.n_base == len(Q.BASE_SIZES)
    tables = Q.directed_tables()
    assert len(tables) == 17 and len({subset for _, subset, _ in tables}) == 16
    for name, subset, terms in tables:
        tt, _, _ = check_pack([(None, t) for t in terms], ev, vocab, df, corpus.n_docs)
        assert Q.steps_of(tt) == subset, (name, Q.steps_of(tt))
    lone = next(terms for name, _, terms in tables if name.startswith("cspan whose union"))
    assert not any(t.has_union for t in lone) and Q.pack_base([(None, t) for t in lone]).n_union == 3
    sizes = [len(terms) for _, _, terms in tables]
    assert all((a - b) * (b - c) < 0 for a, b, c in zip(sizes, sizes[1:], sizes[2:-2]))  # large, small, large, ...


def test_equal_pairs_and_equal_items_are_stored_once(ev):
    corpus, _, vocab, df = Q.world()
    a = Terms(all_of=[Prefix("sell")], none_of=[("w00", Phrase("w01"))])
    b = Terms(all_of=(Prefix("sell"),), none_of=[(OneOf("w00"), "w01")])
    assert a == b
    tt = pack([(None, a), (None, b), (None, a)], vocab, df, corpus.n_docs)
    assert tt.n_cons == 1 and tt.qscope.tolist() == [0, 0, 0] and tt.rows_cap == int(tt.driver_lens[0])
    sell = [w for w in Q.VOCAB if w.startswith("sell")]
    same = [Prefix("sell"), OneOf(*sell), OneOf(*reversed(sell)), OneOf(Prefix("seller"), "sell", "selling", Q.UNKNOWN)]
    tt = pack([(None, Terms(all_of=[m])) for m in same] + [(None, Terms(all_of=[Prefix("s")])), (None, Terms(all_of=[Prefix("se")]))],
              vocab, df, corpus.n_docs)
    assert tt.n_cons == 6 and tt.n_union == 2 and tt.unions == (Prefix("sell"), Prefix("s"))
    assert tt.ops[3].tolist() == [len(vocab)] * 4 + [len(vocab) + 1] * 2
    # a PhraseOf / NearOf of plain slots IS the plain item, also when a slot is a class of one token
    tt = pack([(None, Terms(all_of=[PhraseOf(Prefix("sellers"), OneOf("w00", Q.UNKNOWN))])), (None, Terms(all_of=[Phrase("sellers", "w00")])),
               (None, Terms(all_of=[NearOf("w01", Prefix("selx"), distance=5)])), (None, Terms(all_of=[Near("w01", "selx", distance=5)]))],
              vocab, df, corpus.n_docs)
    assert (tt.n_phr, tt.n_near, tt.n_union, tt.n_cspan) == (1, 1, 0, 0) and tt.ops[3].tolist() == [60, 60, 61, 61]
    assert tt.n_cons == 4  # (the Terms differ; their lists do not)


def test_pack_keeps_its_invariants_after_each_edit_round():
    """The host model alone: after an add, a remove and a replace the same expressions packed against the NEW vocabulary and
    document frequencies keep every invariant over the edited documents."""
    from legal_rag_amd.bm25_model import BM25Okapi
    words = Q.world()[1]
    model = BM25Okapi(words)
    kept = Q.live_terms()
    seen, sel = {tuple(model.vocab())}, [sorted(w for w in model.vocab() if w.startswith("sel"))]
    for op, after in Q.edit_rounds(words):
        Q.apply_edit(model, op)
        vocab, df = model.vocab(), model._doc_frequencies()
        assert model.corpus_size == len(after) and set(vocab) == set().union(*map(set, after))
        ev = Q.Evaluator(after)
        ok = [t for t in kept if not Q.refused(t, vocab, df, len(after))]
        assert all(Q.overlapping_pair(t, list(vocab)) for t in kept if t not in ok) and len(ok) >= len(kept) - 5
        tt, _, _ = check_pack([(None, t) for t in ok], ev, vocab, df, len(after))
        assert min(tt.n_phr, tt.n_near, tt.n_union, tt.n_cspan) >= 10
        seen.add(tuple(vocab))
        sel.append(sorted(w for w in vocab if w.startswith("sel")))
    assert len(seen) == 4                                  # every round renumbers the vocabulary
    assert len(sel[0]) < len(sel[1]) > len(sel[2]) and sel[2] != sel[0]  # Prefix("sel") names other tokens each time


def test_shrink_finds_the_smallest_failing_expression():
    big = Terms(all_of=[("w00", NearOf(Prefix("sel"), OneOf("w01", "w02"), "w03", distance=5)), Phrase("w04", "w05")],
                any_of=[Near("w06", "w07", "w08", distance=2)], none_of=["w09"])
    has = lambda t: any(isinstance(m, NearOf) and Prefix("sel") in m.members for _, g in t.groups() for m in g)  # noqa: E731
    small = Q.shrink(big, has)
    assert has(small) and len(small.groups()) == 1 and len(small.groups()[0][1]) == 1 and len(small.groups()[0][1][0]) == 2
    least = Q.shrink(big, lambda t: True).groups()
    assert len(least) == 1 and len(least[0][1]) == 1 and isinstance(least[0][1][0], str)

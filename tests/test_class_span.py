"""PhraseOf / NearOf on the host: the certificates of tests/class_span_cases.py (each builder proves its own case against
`within`), the classes themselves (construction errors, hashing, pickling), `within` against a brute force over position
tuples, the certificate that the device's first-unfilled-slot tally equals the bipartite matching on equal-or-disjoint
slot families — and the written-out counter-example where it does not — `Terms` with the new members, `pack()` (the fold to
the plain Phrase / Near, equal items stored once, the numbering behind the unions, the bounds, a union registered only by a
span, the overlap ValueError, a table without a class span unchanged) and the plan arithmetic (amdr_class_spans_plan)."""
import dataclasses
import pickle
from itertools import permutations

import numpy as np
import pytest

import class_span_cases as CC
from legal_rag_amd.retrieval.terms import (Near, NearOf, OneOf, Phrase, PhraseOf, Prefix, TermTable, Terms, fills, pack)

VOCAB_TOKENS = ["sell", "seller", "seller's", "selling", "sells", "buyer", "buy", "buys", "buying", "purchaser", "goods",
                "good", "security", "secured", "interest", "interests", "accept", "accepts", "a", "b", "c", "d"]
VOCAB = {w: i for i, w in enumerate(VOCAB_TOKENS)}
DF = {w: 3 + 2 * i for i, w in enumerate(VOCAB_TOKENS)}
N_DOCS = 100
FIELDS = ["ops", "qscope", "n_cons", "n_groups", "n_base", "driver_lens", "cand_max", "rows_cap", "phr_ops", "phrases",
          "phr_cand_max", "phr_rows_cap", "span_ops", "nears", "near_cand_max", "near_rows_cap"]


# ---- the certificates --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", CC.SIZES)
def test_edge_corpus_certificates(m):
    CC.edge_certificates(m)


@pytest.mark.parametrize("count", CC.DRIVER_COUNTS)
def test_driver_corpus_certificates(count):
    CC.driver_certificates(count)


def test_batches_keep_the_overlap_rule_and_operands_number_classes_behind_cls_first():
    corpus, _ = CC.edge_corpus(2)
    for count in (1, 2, 65):
        items = CC.batch(corpus, CC.edge_items(2), count)
        assert len(items) == count
        for kind, slots, _n in items:
            if kind == CC.UNORDERED:
                sets = [set(s) if isinstance(s, tuple) else {s} for s in slots]
                assert all(a == b or not a & b for a in sets for b in sets)
    items = CC.batch(corpus, CC.edge_items(2), 65)
    (ptr, slots, kind, dist), (c_ptr, c_terms) = CC.operands(items, corpus.n_terms, cls_first=3)
    classes = CC.classes_of(items)
    assert ptr[-1] == slots.size and kind.size == dist.size == 65 and c_ptr[-1] == c_terms.size == sum(map(len, classes))
    assert slots[slots != CC.UNKNOWN].max() == corpus.n_terms + 3 + len(classes) - 1 and len(set(classes)) == len(classes)
    assert CC.UNKNOWN in slots and CC.UNKNOWN >= corpus.n_terms + 3 + len(classes)  # past the vocabulary AND the classes
    assert all(np.all(np.diff(c_terms[c_ptr[c]:c_ptr[c + 1]]) > 0) for c in range(len(classes)))


# ---- the classes -------------------------------------------------------------------------------------------------------
def test_phrase_of_and_near_of_are_frozen_hashable_picklable_and_validated():
    p = PhraseOf(Prefix("secur"), "interest")
    n = NearOf(Prefix("buy"), OneOf("seller", Prefix("sells")), distance=5)
    assert p == PhraseOf(Prefix("secur"), "interest") and hash(p) == hash(PhraseOf(Prefix("secur"), "interest"))
    assert p != PhraseOf("interest", Prefix("secur")) and p != Phrase("secur", "interest") and len(p) == 2 and len(n) == 2
    assert n == NearOf(Prefix("buy"), OneOf("seller", Prefix("sells")), distance=5)
    assert n != NearOf(Prefix("buy"), OneOf("seller", Prefix("sells")), distance=5, ordered=True)
    assert n != NearOf(Prefix("buy"), OneOf("seller", Prefix("sells")), distance=4) and n != Near("buy", "seller", distance=5)
    assert len({p, PhraseOf(Prefix("secur"), "interest"), n, NearOf(*n.members, distance=5)}) == 2
    assert repr(p) == "PhraseOf(Prefix('secur'), 'interest')"
    assert repr(n) == "NearOf(Prefix('buy'), OneOf('seller', Prefix('sells')), distance=5)"
    assert repr(NearOf("a", "b", distance=2, ordered=True)) == "NearOf('a', 'b', distance=2, ordered=True)"
    for x in (p, n, NearOf("a", Prefix("b"), distance=255, ordered=True)):
        back = pickle.loads(pickle.dumps(x))
        assert back == x and hash(back) == hash(x) and type(back) is type(x)
        with pytest.raises(AttributeError, match="frozen"):
            x.members = ()
        with pytest.raises(AttributeError, match="frozen"):
            del x.members
    for bad in (Phrase("a", "b"), Near("a", "b", distance=2), p, n, 3, None, ("a", "b")):
        with pytest.raises(TypeError, match="a member is a str, a Prefix or a OneOf"):
            PhraseOf("a", bad)
        with pytest.raises(TypeError, match="a member is a str, a Prefix or a OneOf"):
            NearOf(bad, "a", distance=2)
    for k in (0, 1, 17):
        with pytest.raises(ValueError, match="PhraseOf: 2 to 16 members"):
            PhraseOf(*["a"] * k)
    for k in (0, 1, 9):
        with pytest.raises(ValueError, match="NearOf: 2 to 8 members"):
            NearOf(*["a"] * k, distance=2)
    assert len(PhraseOf(*["a"] * 16)) == 16 and len(NearOf(*["a"] * 8, distance=1)) == 8
    for d in (0, 256, -1):
        with pytest.raises(ValueError, match="a distance of 1 to 255"):
            NearOf("a", "b", distance=d)
    for d in (2.0, "2", True, None):
        with pytest.raises(TypeError, match="distance is an int"):
            NearOf("a", "b", distance=d)
    with pytest.raises(TypeError):
        NearOf("a", "b")  # the distance is required
    assert NearOf("a", "b", distance=np.int64(3)).distance == 3


def test_terms_take_both_wherever_a_phrase_or_a_near_stands():
    p, n = PhraseOf(Prefix("secur"), "interest"), NearOf(Prefix("buy"), Prefix("sell"), distance=5)
    t = Terms(all_of=[p, (n, "goods")], any_of=n, none_of=[(p, Prefix("x"))])
    assert t.all_of == ((p,), (n, "goods")) and t.any_of == ((n,),) and t.none_of == ((p, Prefix("x")),)
    assert t.has_class_span and not t.has_phrase and not t.has_near and t.has_union
    assert not Terms(all_of=[Phrase("a", "b"), Prefix("x")]).has_class_span and not Terms().has_class_span
    assert hash(t) == hash(Terms(all_of=[p, (n, "goods")], any_of=n, none_of=[(p, Prefix("x"))]))
    one = Terms(all_of=[n])
    doc = "the buyer paid and the sellers shipped goods".split()
    assert one.matches(doc) and not one.matches(list(reversed(doc))[:2]) and one.matches(tuple(doc))
    for bad in (set(doc), frozenset(doc), dict.fromkeys(doc)):
        with pytest.raises(TypeError, match="token sequence"):
            one.matches(bad)
    assert Terms(all_of=[p], none_of=[n]).matches("a secured interest".split())
    assert not Terms(all_of=[p], none_of=[n]).matches("a secured interest buys sells".split())


# ---- within ------------------------------------------------------------------------------------------------------------
def brute(members, tokens, n, kind) -> bool:
    """The definitions spelt out on position tuples: every assignment of the members, in order, to distinct positions."""
    M = len(members)
    for pos in permutations(range(len(tokens)), M):
        if not all(fills(m, tokens[q]) for m, q in zip(members, pos)):
            continue
        if kind == "phrase" and all(pos[j] == pos[0] + j for j in range(M)):
            return True
        if kind == "ordered" and all(pos[j] < pos[j + 1] for j in range(M - 1)) and pos[-1] - pos[0] <= n:
            return True
        if kind == "unordered" and max(pos) - min(pos) <= n:
            return True
    return False


def test_within_equals_a_brute_force_over_position_tuples():
    rng = np.random.default_rng(11)
    alphabet = ["a", "b", "ab", "abc", "b2", "c", "x"]
    pool = ["a", "b", "c", Prefix("a"), Prefix("ab"), Prefix("b"), OneOf("a", "c"), OneOf("b", Prefix("ab")), OneOf("x"), "nowhere"]
    seen = {(k, w): 0 for k in ("phrase", "ordered", "unordered") for w in (False, True)}
    for _ in range(1500):
        M = int(rng.integers(2, 5))
        members = [pool[int(i)] for i in rng.integers(0, len(pool), size=M)]
        tokens = [alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=int(rng.integers(0, 7)))]
        n = int(rng.integers(1, 5))
        for kind, obj in (("phrase", PhraseOf(*members)), ("ordered", NearOf(*members, distance=n, ordered=True)),
                          ("unordered", NearOf(*members, distance=n))):
            want = brute(members, tokens, n, kind)
            assert obj.within(tokens) == want == obj.within(tuple(tokens)), (obj, tokens)
            seen[(kind, want)] += 1
    assert all(v > 50 for v in seen.values()), seen
    # the degenerate forms name what the plain classes name
    for _ in range(300):
        tokens = [alphabet[int(i)] for i in rng.integers(0, 4, size=int(rng.integers(0, 8)))]
        ws = [alphabet[int(i)] for i in rng.integers(0, 4, size=int(rng.integers(2, 4)))]
        n = int(rng.integers(1, 4))
        assert PhraseOf(*ws).within(tokens) == Phrase(*ws).within(tokens)
        for o in (False, True):
            assert NearOf(*ws, distance=n, ordered=o).within(tokens) == Near(*ws, distance=n, ordered=o).within(tokens), (ws, tokens, n, o)
    assert NearOf("a", "b", distance=1, ordered=True).within(["x", "a", "b"]) and PhraseOf("a", "b").within(["x", "a", "b"])


def tally(sets, tokens, n) -> bool:
    """The device's unordered rule (class_span_rule.hpp cs_lane_hit): from every anchor, a token fills the FIRST unfilled
    slot it may fill; an anchor that fills none does nothing."""
    full = (1 << len(sets)) - 1
    for s in range(len(tokens)):
        filled = 0
        for q in range(s, min(len(tokens), s + n + 1)):
            mask = sum(1 << j for j, ids in enumerate(sets) if tokens[q] in ids)
            free = mask & ~filled & full
            filled |= free & -free
            if filled == 0:
                break
            if filled == full:
                return True
    return False


def test_the_tally_is_the_matching_on_equal_or_disjoint_slots_and_not_beyond():
    rng = np.random.default_rng(12)
    groups = [("a", "b"), ("c",), ("d", "e", "f"), ("g",)]  # pairwise disjoint; a slot is one of them, repeats allowed
    alphabet = list("abcdefgx")
    hits = 0
    for _ in range(3000):
        M = int(rng.integers(2, 9))
        sets = [groups[int(i)] for i in rng.integers(0, len(groups), size=M)]
        tokens = [alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=int(rng.integers(0, 14)))]
        n = int(rng.integers(1, 12))
        want = NearOf(*[OneOf(*s) for s in sets], distance=n).within(tokens)
        assert tally(sets, tokens, n) == want, (sets, tokens, n)
        hits += want
    assert 300 < hits < 2700
    # the written-out counter-example: slots {a, b}, {a} on the tokens a b.  The matching b -> slot 0, a -> slot 1 exists;
    # the tally gives a to slot 0 and finds nothing for slot 1
    assert NearOf(OneOf("a", "b"), "a", distance=1).within(["a", "b"]) and not tally([("a", "b"), ("a",)], ["a", "b"], 1)
    assert tally([("a",), ("a", "b")], ["a", "b"], 1)  # (the other order happens to work: the rule cannot rest on luck)


# ---- pack ----------------------------------------------------------------------------------------------------------------
def same_fields(a, b):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, tuple) and x and isinstance(x[0], np.ndarray):
            assert all(np.array_equal(p, q) and p.dtype == q.dtype for p, q in zip(x, y)), f.name
        elif isinstance(x, np.ndarray):
            assert np.array_equal(x, y) and x.dtype == y.dtype, f.name
        else:
            assert x == y, f.name


def test_items_of_plain_slots_fold_to_the_plain_phrase_and_near():
    plain = [(None, Terms(all_of=[Phrase("a", "b")], none_of=[Near("c", "d", distance=4)])),
             (None, Terms(any_of=[Near("good", "sells", distance=2, ordered=True), Phrase("a", "nowhere")]))]
    # a one-token Prefix, a one-member OneOf and a OneOf of one KNOWN token are plain ids; an unknown str keeps its name
    folded = [(None, Terms(all_of=[PhraseOf("a", OneOf("b"))], none_of=[NearOf(Prefix("c"), OneOf("d", "nowhere"), distance=4)])),
              (None, Terms(any_of=[NearOf(Prefix("good"), Prefix("sells"), distance=2, ordered=True), PhraseOf("a", "nowhere")]))]
    vocab = dict(VOCAB)
    del vocab["goods"]  # (Prefix("good") then names one token)
    df = {w: DF[w] for w in vocab}
    vocab = {w: i for i, w in enumerate(vocab)}
    a, b = pack(plain, vocab, df, N_DOCS), pack(folded, vocab, df, N_DOCS)
    same_fields(a, b)
    assert b.n_cspan == 0 and b.n_union == 0 and b.cspans == () and b.cspan_rows_cap == 0 and b.cspan_cand_max == 0
    assert [x.tolist() for x in b.cspan_ops] == [[0], [], [], []]
    assert b.phrases == (Phrase("a", "b"), Phrase("a", "nowhere")) and b.nears[1] == Near("good", "sells", distance=2, ordered=True)
    # the plain form and the folded one in ONE batch share a slot
    both = pack(plain + folded, vocab, df, N_DOCS)
    assert (both.n_phr, both.n_near, both.n_cspan) == (2, 2, 0) and both.qscope.tolist() == [0, 1, 2, 3]
    assert both.ops[3].tolist()[:4] == both.ops[3].tolist()[4:]


def test_class_spans_are_stored_once_behind_the_unions_with_the_smallest_slot_bound():
    V = len(VOCAB)
    sell, buy = Prefix("sell"), Prefix("buy")
    n1 = NearOf(buy, sell, distance=5)
    n1_again = NearOf(OneOf("buy", "buyer", "buying", "buys"), OneOf(Prefix("sell")), distance=5)  # equal after resolution
    p1 = PhraseOf(Prefix("secur"), "interest")
    o1 = NearOf("accept", OneOf("buyer", "purchaser"), distance=3, ordered=True)
    ph, nr = Phrase("a", "b"), Near("c", "d", distance=4)
    pairs = [(None, Terms(all_of=[n1], none_of=[sell])), (None, Terms(all_of=[(p1, ph, nr)])), (None, Terms(any_of=[n1_again, o1])),
             (None, Terms(all_of=[NearOf(buy, sell, distance=5, ordered=True)])), (None, Terms(all_of=[PhraseOf(Prefix("zz"), sell)]))]
    tt = pack(pairs, VOCAB, DF, N_DOCS)
    ids = lambda stem: sorted(VOCAB[w] for w in VOCAB if w.startswith(stem))  # noqa: E731
    # unions in first-seen order: buy!, sell! (registered by the span BEFORE the top-level sell! that shares it), secur!, the OneOf
    assert tt.unions == (buy, sell, Prefix("secur"), OneOf("buyer", "purchaser")) and tt.n_union == 4
    assert tt.union_ops[1].tolist() == ids("buy") + ids("sell") + ids("secur") + sorted([VOCAB["buyer"], VOCAB["purchaser"]])
    assert (tt.n_phr, tt.n_near, tt.n_cspan) == (1, 1, 5)
    U = V + 2
    C = U + 4
    assert tt.cspans == (n1, p1, o1, NearOf(buy, sell, distance=5, ordered=True), PhraseOf(Prefix("zz"), sell))
    assert tt.ops[3].tolist() == [C + 0, U + 1, C + 1, V + 0, V + 1, C + 0, C + 2, C + 3, C + 4]
    assert [tt.list_item(i) for i in (0, 1, 2, 5, 6, 10)] == [ph, nr, buy, OneOf("buyer", "purchaser"), n1, tt.cspans[4]]
    ptr, slots, kind, dist = tt.cspan_ops
    assert ptr.dtype == np.int64 and slots.dtype == kind.dtype == dist.dtype == np.int32
    assert ptr.tolist() == [0, 2, 4, 6, 8, 10] and kind.tolist() == [1, 0, 2, 2, 0] and dist.tolist() == [5, 0, 3, 5, 0]
    assert slots.tolist() == [U + 0, U + 1, U + 2, VOCAB["interest"], VOCAB["accept"], U + 3, U + 0, U + 1, -1, U + 1]
    ub = lambda ws: min(N_DOCS, sum(DF[w] for w in ws))  # noqa: E731
    b_buy, b_sell = ub([w for w in VOCAB if w.startswith("buy")]), ub([w for w in VOCAB if w.startswith("sell")])
    bounds = [min(b_buy, b_sell), min(ub(["security", "secured"]), DF["interest"]), min(DF["accept"], ub(["buyer", "purchaser"])),
              min(b_buy, b_sell), 0]
    assert tt.cspan_cand_max == max(bounds) and tt.cspan_rows_cap == sum(bounds)
    assert tt.driver_lens.tolist() == [bounds[0], min(bounds[1], DF["a"], DF["c"]), N_DOCS, bounds[3], 0]
    assert tt.union_rows_cap == b_buy + b_sell + ub(["security", "secured"]) + ub(["buyer", "purchaser"])
    # a union registered ONLY by a span
    only = pack([(None, Terms(all_of=[PhraseOf("a", Prefix("sell"))]))], VOCAB, DF, N_DOCS)
    assert only.n_union == 1 and only.unions == (Prefix("sell"),) and only.n_cspan == 1
    assert only.cspan_ops[1].tolist() == [VOCAB["a"], V] and only.ops[3].tolist() == [V + 1]
    assert only.cand_max == min(DF["a"], b_sell) == only.cspan_cand_max


def test_overlapping_unequal_slots_of_an_unordered_near_of_are_refused_by_name():
    for bad in (NearOf("seller", Prefix("sell"), distance=3), NearOf(Prefix("sell"), "x", OneOf("sells", "buyer"), distance=3),
                NearOf(Prefix("sell"), Prefix("seller"), distance=9)):
        with pytest.raises(ValueError, match=r"NearOf\(.*\): members \d and \d name overlapping, unequal token sets"):
            pack([(None, Terms(all_of=[bad]))], VOCAB, DF, N_DOCS)
    with pytest.raises(ValueError, match=r"NearOf\('seller', Prefix\('sell'\), distance=3\)"):
        pack([(None, Terms(none_of=[("a", NearOf("seller", Prefix("sell"), distance=3))]))], VOCAB, DF, N_DOCS)
    # equal slots, disjoint slots, the ordered form and the phrase are taken
    ok = [NearOf(Prefix("sell"), Prefix("sell"), distance=3), NearOf(Prefix("sell"), OneOf(*[w for w in VOCAB if w.startswith("sell")]), distance=3),
          NearOf(Prefix("sell"), Prefix("buy"), "a", distance=3), NearOf("seller", Prefix("sell"), distance=3, ordered=True),
          PhraseOf("seller", Prefix("sell")), NearOf(Prefix("sell"), Prefix("nowhere"), distance=3)]
    tt = pack([(None, Terms(all_of=[x])) for x in ok], VOCAB, DF, N_DOCS)
    assert tt.n_cspan == 5 and tt.cspans[0] == ok[0]  # (the first two are equal after resolution)


def test_a_table_without_a_class_span_is_what_it_was():
    assert [f.name for f in dataclasses.fields(TermTable)] == FIELDS  # the class-span attributes are no dataclass fields
    assert not {"cspan_ops", "cspans", "cspan_cand_max", "cspan_rows_cap", "n_cspan"} & set(FIELDS)
    pairs = [(None, Terms(all_of=[Phrase("a", "b"), Prefix("sell")])), (None, Terms(all_of=["c"], none_of=[Near("b", "a", distance=3)]))]
    tt = pack(pairs, VOCAB, DF, N_DOCS)
    assert (tt.n_cspan, tt.cspans, tt.cspan_cand_max, tt.cspan_rows_cap) == (0, (), 0, 0)
    assert "cspans" not in tt.__dict__ and "cspan_ops" not in tt.__dict__  # the class-level defaults, untouched
    # a class span beside them changes no field of the constraints it does not stand in
    more = pack(pairs + [(None, Terms(all_of=[NearOf(Prefix("buy"), "a", distance=2)]))], VOCAB, DF, N_DOCS)
    for name in ("phr_ops", "span_ops"):
        assert all(np.array_equal(x, y) for x, y in zip(getattr(tt, name), getattr(more, name))), name
    for name in ("phrases", "nears", "phr_cand_max", "phr_rows_cap", "near_cand_max", "near_rows_cap"):
        assert getattr(tt, name) == getattr(more, name), name
    assert more.ops[3].tolist() == tt.ops[3].tolist() + [len(VOCAB) + 2 + 2] and more.unions == (Prefix("sell"), Prefix("buy"))


# ---- the plan --------------------------------------------------------------------------------------------------------------
def test_plan_arithmetic_and_null_handles():
    from legal_rag_amd import _native
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for n in (1, 2, 65, 4096):
        for cand_max in (0, 1, 255, 256, 257, 3 * 256 + 1, 1_000_000):
            cells = n * max(1, -(-cand_max // _native.PHRASE_TILE))
            assert _native.class_spans_plan(n, cand_max) == up(8 * cells) + up(8 * (cells + 1)) + up(1024 * cells), (n, cand_max)
    assert _native.class_spans_plan(0, 100) >= 0
    assert _native.class_spans_plan(2**24 - 1, 256) > 0
    for bad in ((-1, 10), (1, -1), (2**24, 256), (2**23, 257), (2**31, 1)):  # cells x 256 threads >= 2^32
        with pytest.raises(_native.NativeError):
            _native.class_spans_plan(*bad)
    lib = _native.load()  # a null handle is refused before any device is touched
    assert lib.amdr_class_spans_device(None, None, None, None, None, 1, None, None, 0, 0, 0, 0, 0, None, None, None, None, 0, None) == -1
    assert b"null handle" in lib.amdr_last_error()
    assert lib.amdr_class_spans(None, None, None, None, None, 1, None, None, 0, 0, 0, None, None, None) == -1
    assert b"null handle" in lib.amdr_last_error()

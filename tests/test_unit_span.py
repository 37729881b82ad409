"""The same-sentence and same-paragraph connectors on the CPU (no GPU): the rule that makes the break flags
(retrieval/units.py break_flags) on written-out texts, `Within` (retrieval/terms.py) — its constructor, hashing, pickling,
`Within.within` and `Terms.matches` against the brute-force evaluator of tests/unit_span_cases.py on every document —
`pack()`'s invariants, the certificates of the generated cases, and three wrong models that must each disagree with the
evaluator, or the cases would show nothing."""
import dataclasses
import pickle

import numpy as np
import pytest

import unit_span_cases as UC
from legal_rag_amd import text
from legal_rag_amd.retrieval.terms import Fuzzy, Near, NearOf, OneOf, Phrase, Prefix, TermTable, Terms, Wildcard, Within, pack
from legal_rag_amd.retrieval.units import break_flags, break_positions, unit_ranges

VOCAB_TOKENS = ["sell", "seller", "seller's", "selling", "sells", "buyer", "buy", "buys", "buying", "purchaser", "goods",
                "good", "security", "secured", "interest", "interests", "accept", "accepts", "a", "b", "c", "d"]
VOCAB = {w: i for i, w in enumerate(VOCAB_TOKENS)}
DF = {w: 3 + 2 * i for i, w in enumerate(VOCAB_TOKENS)}
N_DOCS = 100
FIELDS = ["ops", "qscope", "n_cons", "n_groups", "n_base", "driver_lens", "cand_max", "rows_cap", "phr_ops", "phrases",
          "phr_cand_max", "phr_rows_cap", "span_ops", "nears", "near_cand_max", "near_rows_cap"]


@pytest.fixture(scope="module")
def cases():
    corpus, at = UC.make_corpus()
    return corpus, at, UC.batch(corpus, UC.N_ITEMS)


# ---- the rule that makes the flags -----------------------------------------------------------------------------------------
def flags_en(s):
    toks = text.tokenize_en(s)
    fl, mapped = break_flags(s, toks, True)
    return toks, fl.tolist(), mapped


def test_break_flags_on_written_out_texts():
    # the UCC form: a section heading, subsections on lines of their own
    s = "§ 2-210. Delegation of Performance.\n(1) A party may perform his duty through a delegate. No delegation relieves.\n(2) Unless agreed."
    toks, fl, mapped = flags_en(s)
    assert mapped and len(fl) == len(toks)
    assert toks == ["2", "210", "delegation", "of", "performance", "1", "a", "party", "may", "perform", "his", "duty", "through", "a",
                    "delegate", "no", "delegation", "relieves", "2", "unless", "agreed"]
    #            2  210 delegation of performance (1) a  party may perform his duty through a delegate no delegation relieves (2) unless agreed
    assert fl == [0, 0, 1,         0, 0,          3,  0, 0,    0,  0,      0,  0,   0,      0, 0,       1, 0,         0,       3,  0,     0]
    # the first token's byte stays 0 (the rule forces it); "§ 2-210. " breaks: accepted; "\n(1)" opens a paragraph
    assert unit_ranges(fl, 2) == [(0, 5), (5, 18), (18, 21)] and unit_ranges(fl, 1) == [(0, 2), (2, 5), (5, 15), (15, 18), (18, 21)]
    # a closing quote behind the full stop is absorbed: the break lies behind it
    toks, fl, _ = flags_en('He said "no." Then he left. (See above.) Fine')
    assert [t for t, f in zip(toks, fl) if f] == ["then", "see", "fine"] and all(f == 1 for f in fl if f)
    assert break_positions('a." b')[0] == [3]
    # no whitespace behind the point: no break; "U.S. " breaks (accepted)
    toks, fl, _ = flags_en("Interest of 2.5 percent accrues. In the U.S. it does")
    assert [t for t, f in zip(toks, fl) if f] == ["in", "it"]
    # the end of the text is a break position, with no token behind it
    assert break_positions("end.")[0] == [4] and flags_en("end.")[1] == [0]
    # a Han sentence: the full stop breaks without whitespace; a segmenter's own "。" token closes its unit
    han = "买方应当付款。卖方应当交货！是吗？是"
    toks = ["买方", "应当", "付款", "。", "卖方", "应当", "交货", "！", "是", "吗", "？", "是"]
    fl, mapped = break_flags(han, toks, False)
    assert mapped and fl.tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1]
    fl, _ = break_flags(han, [t for t in toks if t not in "。！？"], False)
    assert fl.tolist() == [0, 0, 0, 1, 0, 0, 1, 0, 1]
    fl, _ = break_flags("他说：“不行。”然后走了", ["他", "说", "不行", "然后", "走了"], False)
    assert fl.tolist() == [0, 0, 0, 1, 0]  # the closing mark is absorbed
    # "\r\n" counts once, and a "\n" token of the stream closes its paragraph
    toks, fl, _ = flags_en("first line\r\nsecond line\n\nthird")
    assert [(t, f) for t, f in zip(toks, fl) if f] == [("second", 3), ("third", 3)]
    assert break_positions("a\r\nb")[1] == [3]
    fl, _ = break_flags("甲\n乙", ["甲", "\n", "乙"], False)
    assert fl.tolist() == [0, 0, 3]
    # lower-casing changes the length: the tokens cannot be mapped back — all zero, unmapped
    s = "İstanbul rules. Second sentence"
    assert len(s.lower()) != len(s)
    toks, fl, mapped = flags_en(s)
    assert not mapped and fl == [0] * len(toks) and len(toks) >= 3
    assert break_flags("", [], True)[0].size == 0 and break_flags("", [], True)[1]


# ---- the class ---------------------------------------------------------------------------------------------------------------
def test_within_is_frozen_hashable_picklable_and_validated():
    w = Within("buyer", Prefix("sell"), unit="paragraph", ordered=True)
    assert w == Within("buyer", Prefix("sell"), unit="paragraph", ordered=True) and hash(w) == hash(pickle.loads(pickle.dumps(w)))
    assert pickle.loads(pickle.dumps(w)) == w and len(w) == 2 and w.kind == 3
    assert repr(w) == "Within('buyer', Prefix('sell'), unit='paragraph', ordered=True)"
    assert repr(Within("a", "b")) == "Within('a', 'b', unit='sentence')" and Within("a", "b").kind == 0
    assert len({w, Within("buyer", Prefix("sell"), unit="paragraph"), Within("buyer", Prefix("sell"), ordered=True),
                Within(Prefix("sell"), "buyer", unit="paragraph", ordered=True)}) == 4
    assert w != NearOf("buyer", Prefix("sell"), distance=3, ordered=True)
    with pytest.raises(AttributeError):
        w.unit = "sentence"
    with pytest.raises(AttributeError):
        del w.members
    for bad in ((), ("a",), tuple("abcdefghi")):
        with pytest.raises(ValueError, match="2 to 8 members"):
            Within(*bad)
    Within(*"abcdefgh")
    with pytest.raises(ValueError, match="sentence.*paragraph"):
        Within("a", "b", unit="line")
    with pytest.raises(TypeError):
        Within("a", "b", unit=1)
    for bad in (Phrase("a", "b"), Near("a", "b", distance=2), Within("a", "b"), 3, None):
        with pytest.raises(TypeError):
            Within("a", bad)
    Within(OneOf("a", Prefix("b")), Wildcard("s?ll"), Fuzzy("goods"))
    # wherever a Near stands: an entry of every field, a member of a tuple group
    t = Terms(all_of=[w, ("a", w)], any_of=[w], none_of=[(w, "b")])
    assert t.has_within and not t.has_near and not Terms(all_of=["a"]).has_within and hash(t) == hash(pickle.loads(pickle.dumps(t)))
    assert t.all_of == ((w,), ("a", w))
    assert Terms(all_of=[Within("a", OneOf(Wildcard("s?ll"), "b"), Fuzzy("goods"))]).patterns() == [Wildcard("s?ll"), Fuzzy("goods")]
    with pytest.raises(TypeError, match="break flags"):
        t.matches(["a", "b"])
    with pytest.raises(TypeError, match="token sequence"):
        Terms(all_of=[Within("a", "b")]).matches({"a", "b"}, breaks=[0, 0])
    with pytest.raises(ValueError):
        Within("a", "b").within(["a", "b"], [0])
    assert Terms(all_of=["a"]).matches({"a"}) and Terms(all_of=["a"]).matches(["a"], breaks=[0])  # the argument is optional


def as_object(item):
    def member(s):
        if isinstance(s, tuple):
            return Prefix("k") if s == UC.ALL_K else OneOf(*[UC.word(t) for t in s])
        return UC.word(s)
    kind, slots = item
    return Within(*[member(s) for s in slots], unit="paragraph" if kind & UC.PARAGRAPH else "sentence", ordered=bool(kind & UC.ORDERED))


def test_within_and_terms_matches_agree_with_the_evaluator_on_every_document(cases):
    corpus, _, items = cases
    words = [[UC.word(t) for t in seq] for seq in corpus.docs]
    for item in items:
        obj = as_object(item)
        got = [d for d in range(corpus.n_docs) if obj.within(words[d], corpus.breaks[d])]
        assert got == UC.item_list(corpus, item).tolist(), item
    # Terms.matches: a Within beside a plain token, in none_of, in a tuple group
    named = UC.named_items()
    a_b, g_g = as_object(named["a b /s"]), as_object(named["g g /p"])
    A_B, G_G = (set(UC.item_list(corpus, named[k]).tolist()) for k in ("a b /s", "g g /p"))
    for t, want in ((Terms(all_of=[a_b]), lambda d: d in A_B),
                    (Terms(none_of=[a_b], all_of=[UC.word(UC.A)]), lambda d: d not in A_B and UC.A in corpus.docs[d]),
                    (Terms(any_of=[(g_g, UC.word(UC.F)), a_b]), lambda d: d in A_B or (d in G_G and UC.F in corpus.docs[d]))):
        for d in range(corpus.n_docs):
            assert t.matches(words[d], corpus.breaks[d]) == want(d), (t, d)


# ---- pack() ------------------------------------------------------------------------------------------------------------------
def test_withins_are_stored_once_behind_the_class_spans_with_the_smallest_slot_bound():
    V = len(VOCAB)
    sell, buy = Prefix("sell"), Prefix("buy")
    w1 = Within(buy, sell)
    w1_again = Within(OneOf("buy", "buyer", "buying", "buys"), OneOf(Prefix("sell")))  # equal after resolution
    w2 = Within("a", "b", unit="paragraph", ordered=True)                           # plain members: still a unit item
    w3 = Within("a", "b", unit="paragraph")
    w4 = Within("goods", "goods")
    w5 = Within(Prefix("zz"), "a")
    cs = NearOf(buy, "a", distance=4)
    ph, nr = Phrase("a", "b"), Near("c", "d", distance=4)
    pairs = [(None, Terms(all_of=[w1], none_of=[sell])), (None, Terms(all_of=[(w2, ph, nr)])), (None, Terms(any_of=[w1_again, w3, cs])),
             (None, Terms(all_of=[w4], none_of=[(w5, "c")])), (None, Terms(all_of=[w1]))]
    tt = pack(pairs, VOCAB, DF, N_DOCS)
    assert tt.units == (w1, w2, w3, w4, w5) and tt.n_unit == 5 and tt.unions == (buy, sell) and tt.cspans == (cs,)
    assert (tt.n_phr, tt.n_near, tt.n_union, tt.n_cspan) == (1, 1, 2, 1) and tt.qscope.tolist() == [0, 1, 2, 3, 4] and tt.n_cons == 5
    U = V + 2
    C = U + 2
    W = C + 1
    assert tt.ops[3].tolist() == [W + 0, U + 1, W + 1, V + 0, V + 1, W + 0, W + 2, C + 0, W + 3, W + 4, VOCAB["c"], W + 0]
    assert [tt.list_item(i) for i in range(2 + 2 + 1 + 5)] == [ph, nr, buy, sell, cs, w1, w2, w3, w4, w5]
    ptr, slots, kind = tt.unit_ops
    assert ptr.dtype == np.int64 and slots.dtype == kind.dtype == np.int32 and len(tt.unit_ops) == 3
    assert ptr.tolist() == [0, 2, 4, 6, 8, 10] and kind.tolist() == [0, 3, 2, 0, 0]
    assert slots.tolist() == [U + 0, U + 1, VOCAB["a"], VOCAB["b"], VOCAB["a"], VOCAB["b"], VOCAB["goods"], VOCAB["goods"], -1, VOCAB["a"]]
    ub = lambda ws: min(N_DOCS, sum(DF[w] for w in ws))  # noqa: E731
    b_buy, b_sell = ub([w for w in VOCAB if w.startswith("buy")]), ub([w for w in VOCAB if w.startswith("sell")])
    bounds = [min(b_buy, b_sell), min(DF["a"], DF["b"]), min(DF["a"], DF["b"]), DF["goods"], 0]
    assert tt.unit_cand_max == max(bounds) and tt.unit_rows_cap == sum(bounds)
    assert tt.driver_lens.tolist() == [bounds[0], min(bounds[1], DF["a"], DF["c"]), N_DOCS, bounds[3], bounds[0]]
    # a union registered ONLY by a Within; its sorted vocabulary may be handed in
    only = pack([(None, Terms(all_of=[Within("a", sell, unit="paragraph")]))], VOCAB, DF, N_DOCS, sorted_vocab=sorted(VOCAB))
    assert only.n_union == 1 and only.unions == (sell,) and only.n_unit == 1 and only.n_cspan == 0
    assert only.unit_ops[1].tolist() == [VOCAB["a"], V] and only.ops[3].tolist() == [V + 1] and only.unit_ops[2].tolist() == [2]
    assert only.cand_max == min(DF["a"], b_sell) == only.unit_cand_max
    # a pattern among the members takes its expansion
    fz = Fuzzy("sels")
    pat = pack([(None, Terms(all_of=[Within(fz, "a")]))], VOCAB, DF, N_DOCS, expansions={fz: [("sell", 1), ("sells", 1)]})
    assert pat.unions == (fz,) and pat.union_ops[1].tolist() == sorted([VOCAB["sell"], VOCAB["sells"]]) and pat.n_unit == 1
    with pytest.raises(ValueError, match="expansion"):
        pack([(None, Terms(all_of=[Within(fz, "a")]))], VOCAB, DF, N_DOCS)


def test_overlapping_unequal_members_of_an_unordered_within_are_refused_by_name():
    for bad in (Within("seller", Prefix("sell")), Within(Prefix("sell"), "x", OneOf("sells", "buyer"), unit="paragraph"),
                Within(Prefix("sell"), Prefix("seller"))):
        with pytest.raises(ValueError, match=r"Within\(.*\): members \d and \d name overlapping, unequal token sets"):
            pack([(None, Terms(all_of=[bad]))], VOCAB, DF, N_DOCS)
    ok = [Within(Prefix("sell"), Prefix("sell")), Within(Prefix("sell"), OneOf(*[w for w in VOCAB if w.startswith("sell")])),
          Within(Prefix("sell"), Prefix("buy"), "a"), Within("seller", Prefix("sell"), ordered=True), Within(Prefix("sell"), Prefix("nowhere"))]
    tt = pack([(None, Terms(all_of=[x])) for x in ok], VOCAB, DF, N_DOCS)
    assert tt.n_unit == 4 and tt.units[0] == ok[0]  # (the first two are equal after resolution: one id, one group)
    assert tt.unit_ops[1][:2].tolist() == [len(VOCAB), len(VOCAB)]


def test_a_table_without_a_within_is_what_it_was():
    assert [f.name for f in dataclasses.fields(TermTable)] == FIELDS  # the unit attributes are no dataclass fields
    pairs = [(None, Terms(all_of=[Phrase("a", "b"), Prefix("sell")])), (None, Terms(all_of=["c"], none_of=[Near("b", "a", distance=3)])),
             (None, Terms(all_of=[NearOf(Prefix("buy"), "a", distance=2)]))]
    tt = pack(pairs, VOCAB, DF, N_DOCS)
    assert (tt.n_unit, tt.units, tt.unit_cand_max, tt.unit_rows_cap) == (0, (), 0, 0)
    assert not {"units", "unit_ops", "unit_cand_max", "unit_rows_cap"} & set(tt.__dict__)  # the class-level defaults, untouched
    more = pack(pairs + [(None, Terms(all_of=[Within(Prefix("buy"), "a")]))], VOCAB, DF, N_DOCS)
    for name in ("phr_ops", "span_ops", "union_ops", "cspan_ops"):
        assert all(np.array_equal(x, y) for x, y in zip(getattr(tt, name), getattr(more, name))), name
    for name in ("phrases", "nears", "unions", "cspans", "phr_cand_max", "phr_rows_cap", "near_cand_max", "near_rows_cap", "union_rows_cap",
                 "cspan_cand_max", "cspan_rows_cap"):
        assert getattr(tt, name) == getattr(more, name), name
    assert more.ops[3].tolist() == tt.ops[3].tolist() + [len(VOCAB) + 2 + 2 + 1] and more.driver_lens[:3].tolist() == tt.driver_lens.tolist()


def test_highlight_marks_the_members_of_a_within_wherever_they_stand():
    from legal_rag_amd.retrieval.highlight import slot_table
    idf = {w: 1.0 + i for i, w in enumerate(VOCAB_TOKENS)}
    st = slot_table([], Terms(all_of=[Within("buyer", Prefix("sell"))]), VOCAB, idf, sorted(VOCAB))
    assert st.labels == ["buyer", "sell!"] and st.loose == 0b11 and not st.seqs
    assert st.terms[VOCAB["buyer"]] == 0 and all(st.terms[VOCAB[w]] == 1 for w in VOCAB if w.startswith("sell"))


# ---- the cases show something --------------------------------------------------------------------------------------------------
def test_certificates_of_the_generated_cases(cases):
    corpus, at, items = cases
    UC.certificates(corpus, at)
    assert corpus.n_docs <= 4000 and set(corpus.flags().tolist()) == {0, 1, 3}
    lens = {len(s) for s in corpus.docs}
    assert {1, 63, 64, 65, 128, 129} <= lens
    empty = sum(UC.item_list(corpus, it).size == 0 for it in items)
    full = sum(len(UC.conjunction(corpus, it)) > 0 and len(UC.conjunction(corpus, it)) == UC.item_list(corpus, it).size for it in items)
    assert empty * 4 <= len(items) and full * 4 <= len(items), (empty, full, len(items))
    for it in items:  # a list is a subset of the conjunction, a sentence list of the paragraph list, an ordered one of the unordered
        got = set(UC.item_list(corpus, it).tolist())
        assert got <= UC.conjunction(corpus, it)
        assert got <= set(UC.item_list(corpus, (it[0] | UC.PARAGRAPH, it[1])).tolist())
    for name in ("a b", "g g"):
        s_, p_, o_ = (set(UC.item_list(corpus, UC.named_items()[f"{name} {k}"]).tolist()) for k in ("/s", "/p", "+s"))
        assert o_ <= s_ < p_
    # the slots of every unordered item are pairwise disjoint or the same slot
    for kind, slots in items:
        if not kind & UC.ORDERED:
            sets = [set(s) if isinstance(s, tuple) else {s} for s in slots]
            assert all(a == b or not a & b for a in sets for b in sets)
    assert any(len(it[1]) == 8 for it in items) and {it[0] for it in items} == {0, 1, 2, 3}


def test_three_wrong_models_each_disagree_with_the_evaluator(cases):
    corpus, _, items = cases
    right = [UC.item_list(corpus, it).tolist() for it in items]
    assert sum(UC.no_breaks(corpus, it) != r for it, r in zip(items, right)) >= 5
    assert sum(UC.no_carry(corpus, it) != r for it, r in zip(items, right)) >= 5
    assert sum(UC.sentence_for_paragraph(corpus, it) != r for it, r in zip(items, right) if it[0] & UC.PARAGRAPH) >= 5


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def test_plan_arithmetic_and_null_handles():
    from legal_rag_amd import _native
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for n in (1, 2, 65, 4096):
        for cand_max in (0, 1, 255, 256, 257, 3 * 256 + 1, 1_000_000):
            cells = n * max(1, -(-cand_max // _native.PHRASE_TILE))
            assert _native.unit_spans_plan(n, cand_max) == up(8 * cells) + up(8 * (cells + 1)) + up(1024 * cells), (n, cand_max)
    assert _native.unit_spans_plan(0, 100) >= 0
    for bad in ((-1, 10), (1, -1), (2**24, 256), (2**31, 1)):
        with pytest.raises(_native.NativeError):
            _native.unit_spans_plan(*bad)
    lib = _native.load()  # a null handle is refused before any device is touched
    assert lib.amdr_unit_spans_device(None, None, None, None, 1, None, None, 0, 0, 0, 0, 0, None, None, None, None, 0, None) == -1
    assert b"null handle" in lib.amdr_last_error()
    assert lib.amdr_unit_spans(None, None, None, None, 1, None, None, 0, 0, 0, None, None, None) == -1
    assert b"null handle" in lib.amdr_last_error()
    for call in (lambda: lib.amdr_bm25_set_breaks(None, None, 0), lambda: lib.amdr_bm25_breaks_info(None, None),
                 lambda: lib.amdr_bm25_read_breaks(None, None)):
        assert call() == -1 and b"null" in lib.amdr_last_error()

"""Wildcard and Fuzzy on the host (no GPU): the classes, the plain evaluator of tests/vocab_match_cases.py on written-out
cases, terms.pack and highlight.slot_table with `expansions`, the ordering of suggest, and the arithmetic and refusals of
amdr_vocab_match_plan."""
import pickle

import numpy as np
import pytest

import vocab_match_cases as VC
from legal_rag_amd.retrieval.terms import (PREFIX_MAX_TERMS, Fuzzy, Near, NearOf, OneOf, Phrase, PhraseOf, Prefix, Terms, Wildcard,
                                           fills, pack)


def test_the_classes_validate_hash_pickle_and_print():
    w, f = Wildcard("s?ll*"), Fuzzy("warrenty")
    assert w == Wildcard("s?ll*") and hash(w) == hash(Wildcard("s?ll*")) and w != Wildcard("s?ll") and w != Prefix("s?ll*")
    assert f == Fuzzy("warrenty", edits=1) and hash(f) == hash(Fuzzy("warrenty", 1)) and f != Fuzzy("warrenty", edits=2)
    assert repr(w) == "Wildcard('s?ll*')" and repr(f) == "Fuzzy('warrenty', edits=1)"
    assert pickle.loads(pickle.dumps(w)) == w and pickle.loads(pickle.dumps(Fuzzy("lesee", edits=2))) == Fuzzy("lesee", edits=2)
    assert len({w, Wildcard("s?ll*"), f, Fuzzy("warrenty")}) == 2
    for obj in (w, f):
        with pytest.raises(AttributeError):
            obj.pattern = "x"
        with pytest.raises(AttributeError):
            del obj.edits
    for bad in ("", "sell", "?", "*", "?*?", "a" * 64 + "*"):
        with pytest.raises(ValueError):
            Wildcard(bad)
    assert Wildcard("a" * 63 + "*").pattern.endswith("*") and Wildcard("?a")
    with pytest.raises(ValueError, match="plain token"):
        Wildcard("sell")
    with pytest.raises(TypeError):
        Wildcard(3)
    for tok, e in (("", 1), ("a", 1), ("ab", 2), ("a" * 65, 1), ("abc", 0), ("abc", 3)):
        with pytest.raises(ValueError):
            Fuzzy(tok, edits=e)
    assert Fuzzy("ab", edits=1).edits == 1 and Fuzzy("a" * 64, edits=2).edits == 2
    for e in (True, 1.0, "1"):
        with pytest.raises(TypeError):
            Fuzzy("abc", edits=e)
    with pytest.raises(TypeError):
        Fuzzy(None)
    assert Wildcard("a?*").native_pattern() == (0, 0, [ord("a"), VC.ANY_ONE, VC.ANY_RUN])
    assert Fuzzy("中ab", edits=2).native_pattern() == (1, 2, [0x4E2D, ord("a"), ord("b")])


def test_the_plain_evaluator_on_written_out_cases():
    assert VC.osa("recieve", "receive") == 1 and VC.levenshtein("recieve", "receive") == 2
    assert VC.osa("recieve", "relieve") == 1 and VC.osa("ca", "abc") == 3 and VC.osa("", "ab") == 2
    assert VC.osa("warrenty", "warranty") == 1 and VC.osa("lesee", "lessee") == 1 and VC.osa("judgement", "judgment") == 1
    VC.edit_cases(), VC.wild_certificates(), VC.unicode_certificates(), VC.length_cases()
    for n in VC.SIZES:
        VC.sized_vocab(n)
    for m in (3, 4, 5):
        VC.cap_vocab(m)
    ids, dist, n_match = VC.evaluate(["seller", "sell", "", "sill", "tell"], [("w", "s?ll*"), ("f", "sell", 1), ("f", "sell", 2)], 2)
    assert n_match.tolist() == [3, 3, 4] and ids.tolist() == [[0, 1], [1, 3], [0, 1]] and dist.tolist() == [[0, 0], [0, 1], [2, 0]]


def test_within_fills_and_matches_follow_the_evaluator():
    toks = VC.WILD_VOCAB + VC.UNI_VOCAB + [t for _, t, _ in VC.edit_cases()] + VC.length_cases()[1]
    for p in VC.WILD_PATTERNS:
        w = Wildcard(p)
        for t in toks:
            assert w.fits(t) == fills(w, t) == VC.fits(("w", p), t)[0], (p, t)
    for word, e in ((VC.WORD, 1), (VC.WORD, 2), ("aaaaaa", 2), ("中文", 1), ("cafe", 1), ("éa", 1)):
        f = Fuzzy(word, edits=e)
        for t in toks:
            assert f.fits(t) == fills(f, t) == VC.fits(("f", word, e), t)[0], (word, e, t)
    doc = ["the", "seller", "gave", "a", "warranty", "to", "the", "lessee"]
    assert Wildcard("s?ll*").within(doc) and Wildcard("*ee").within(set(doc)) and not Wildcard("b?y*").within(doc)
    assert Fuzzy("warrenty").within(doc) and not Fuzzy("warrenty").within(["warrant"]) and not Wildcard("a*").within([""])
    assert Terms(all_of=[Fuzzy("warrenty"), (Wildcard("s?ll*"), "gave")], none_of=[Wildcard("b?y*")]).matches(doc)
    assert Terms(all_of=[Fuzzy("warrenty")]).matches(set(doc)) and not Terms(none_of=[Fuzzy("lesee")]).matches(doc)
    assert Terms(any_of=[OneOf("buyer", Fuzzy("lesee"))]).matches(doc)
    assert Terms(all_of=[PhraseOf(Fuzzy("warrenty"), "to")]).matches(doc) and not Terms(all_of=[PhraseOf(Fuzzy("warrenty"), "the")]).matches(doc)
    assert Terms(all_of=[NearOf(Wildcard("s?ll*"), Wildcard("*ee"), distance=6)]).matches(doc)
    assert not Terms(all_of=[NearOf(Wildcard("s?ll*"), Wildcard("*ee"), distance=5)]).matches(doc)
    t = Terms(all_of=[OneOf("x", Fuzzy("lesee")), PhraseOf(Wildcard("s?ll*"), "goods")], none_of=[Fuzzy("lesee")])
    assert t.has_pattern and t.patterns() == [Fuzzy("lesee"), Wildcard("s?ll*")] and not Terms(all_of=[Prefix("sell")]).has_pattern
    assert pickle.loads(pickle.dumps(t)) == t and hash(pickle.loads(pickle.dumps(t))) == hash(t)
    for span in (Phrase, lambda *m: Near(*m, distance=3)):
        with pytest.raises(TypeError):
            span(Wildcard("s?ll*"), "goods")
    with pytest.raises(TypeError):
        OneOf(PhraseOf("a", "b"))


VOCAB = {w: i for i, w in enumerate(["sell", "seller", "sells", "goods", "buyer", "sill", "lessee", "lessor", "warranty"])}
DF = {"sell": 5, "seller": 7, "sells": 2, "goods": 9, "buyer": 6, "sill": 1, "lessee": 4, "lessor": 3, "warranty": 8}


def _table_fields(tt):
    return ([a.tolist() for a in tt.ops], tt.qscope.tolist(), tt.n_cons, tt.n_groups, tt.n_base, tt.driver_lens.tolist(), tt.cand_max,
            tt.rows_cap, [a.tolist() for a in tt.phr_ops], tt.phrases, [a.tolist() for a in tt.span_ops], tt.nears,
            [a.tolist() for a in tt.union_ops], tt.unions, tt.union_rows_cap, [a.tolist() for a in tt.cspan_ops], tt.cspans,
            tt.cspan_cand_max, tt.cspan_rows_cap)


def test_pack_resolves_a_pattern_as_a_prefix_from_its_expansion():
    w, f, none, one = Wildcard("se*"), Fuzzy("sell"), Wildcard("zz*"), Fuzzy("warrenty")
    exp = {w: (("sell", 0), ("seller", 0), ("sells", 0)), f: (("sell", 0), ("sells", 1), ("sill", 1)), none: (), one: (("warranty", 1),)}
    # equal expansions share one union with the OneOf of their tokens and with the Prefix
    tt = pack([(None, Terms(all_of=[w])), (None, Terms(all_of=[OneOf("sell", "seller", "sells")])), (None, Terms(all_of=[Prefix("sell")]))],
              VOCAB, DF, 20, expansions=exp)
    assert tt.n_union == 1 and tt.unions == (w,) and tt.union_ops[1].tolist() == [0, 1, 2] and tt.n_cons == 3
    assert [int(tt.ops[3][i]) for i in range(3)] == [len(VOCAB)] * 3 and tt.union_rows_cap == 14
    # bare tokens are taken as well
    assert _table_fields(pack([(None, Terms(all_of=[w]))], VOCAB, DF, 20, expansions={w: ["sell", "seller", "sells"]})) == \
        _table_fields(pack([(None, Terms(all_of=[w]))], VOCAB, DF, 20, expansions=exp))
    # 0 / 1 / many matches: -1, the plain term, a union
    tt = pack([(None, Terms(all_of=[none], any_of=[one, f]))], VOCAB, DF, 20, expansions=exp)
    assert tt.ops[3].tolist() == [-1, VOCAB["warranty"], len(VOCAB)] and tt.union_ops[1].tolist() == [0, 2, 5] and tt.cand_max == 0
    assert _table_fields(pack([(None, Terms(any_of=[one]))], VOCAB, DF, 20, expansions=exp)) == \
        _table_fields(pack([(None, Terms(any_of=["warranty"]))], VOCAB, DF, 20))
    # inside a OneOf, a PhraseOf and a NearOf
    tt = pack([(None, Terms(all_of=[OneOf("buyer", f)]))], VOCAB, DF, 20, expansions=exp)
    assert tt.union_ops[1].tolist() == [0, 2, 4, 5]
    a = pack([(None, Terms(all_of=[PhraseOf(w, "goods"), NearOf(f, one, distance=3)]))], VOCAB, DF, 20, expansions=exp)
    b = pack([(None, Terms(all_of=[PhraseOf(Prefix("sell"), "goods"), NearOf(OneOf("sell", "sells", "sill"), "warranty", distance=3)]))],
             VOCAB, DF, 20)
    fa, fb = _table_fields(a), _table_fields(b)
    assert a.n_cspan == 2 and fa[:12] == fb[:12] and fa[12] == fb[12] and fa[14:16] == fb[14:16] and fa[17:] == fb[17:]
    # a PhraseOf of patterns that each name one token IS the plain phrase
    assert _table_fields(pack([(None, Terms(all_of=[PhraseOf(one, "goods")]))], VOCAB, DF, 20, expansions=exp)) == \
        _table_fields(pack([(None, Terms(all_of=[Phrase("warranty", "goods")]))], VOCAB, DF, 20))
    # the unordered NearOf keeps its overlap error
    with pytest.raises(ValueError, match="overlapping"):
        pack([(None, Terms(all_of=[NearOf(w, f, distance=3)]))], VOCAB, DF, 20, expansions=exp)
    # a missing entry, and no mapping at all
    for e in ({w: exp[w]}, None, {}):
        with pytest.raises(ValueError, match="no expansion"):
            pack([(None, Terms(all_of=[w, f]))], VOCAB, DF, 20, expansions=e)
    # the cap
    big = {f"t{i}": i for i in range(PREFIX_MAX_TERMS + 1)}
    wide = Wildcard("t*")
    with pytest.raises(ValueError, match=r"Wildcard\('t\*'\) names 4097 vocabulary tokens"):
        pack([(None, Terms(all_of=[wide]))], big, {}, 10, expansions={wide: tuple((t, 0) for t in big)})
    assert pack([(None, Terms(all_of=[wide]))], big, {}, 10, expansions={wide: tuple((t, 0) for t in list(big)[:-1])}).n_union == 1


def test_a_table_without_a_pattern_is_unchanged_field_for_field():
    pairs = [(None, Terms(all_of=[Prefix("sell"), ("goods", OneOf("buyer", "lessee"))], none_of=[Phrase("sells", "goods")])),
             (None, Terms(any_of=[Near("buyer", "seller", distance=4), PhraseOf(Prefix("less"), "goods")]))]
    base = _table_fields(pack(pairs, VOCAB, DF, 20))
    assert _table_fields(pack(pairs, VOCAB, DF, 20, expansions=None)) == base
    assert _table_fields(pack(pairs, VOCAB, DF, 20, None, None, {Wildcard("zz*"): (("sell", 0),)})) == base
    from legal_rag_amd.retrieval.highlight import slot_table
    idf = {w: float(i + 1) for w, i in VOCAB.items()}
    plain = slot_table(["seller", "goods"], pairs[0][1], VOCAB, idf, sorted(VOCAB))
    assert slot_table(["seller", "goods"], pairs[0][1], VOCAB, idf, sorted(VOCAB), expansions={Fuzzy("sell"): ()}) == plain


def test_the_slot_table_takes_a_pattern_as_the_oneof_of_its_tokens():
    from legal_rag_amd.retrieval.highlight import slot_table
    idf = {w: float(i + 1) for w, i in VOCAB.items()}
    f, w, none = Fuzzy("sell"), Wildcard("less*"), Wildcard("zz*")
    exp = {f: (("sell", 0), ("sells", 1), ("sill", 1)), w: (("lessee", 0), ("lessor", 0)), none: ()}
    got = slot_table(["goods"], Terms(all_of=[f, PhraseOf(w, "goods")], any_of=[none]), VOCAB, idf, sorted(VOCAB), expansions=exp)
    want = slot_table(["goods"], Terms(all_of=[OneOf("sell", "sells", "sill"), PhraseOf(OneOf("lessee", "lessor"), "goods")]), VOCAB, idf,
                      sorted(VOCAB))
    assert (got.terms, got.weights, got.loose, got.seqs) == (want.terms, want.weights, want.loose, want.seqs)
    assert got.labels[:2] == ["sell~1", "less*"] and got.missing == ["zz*"]
    with pytest.raises(ValueError, match="no expansion"):
        slot_table([], Terms(all_of=[f]), VOCAB, idf, sorted(VOCAB))


def test_suggest_orders_by_distance_then_document_frequency_then_token():
    from legal_rag_amd.retrieval.vocab_match import Suggestion, order_suggestions
    df = {"sell": 5, "sells": 2, "sill": 2, "seal": 9, "tell": 2, "sel": 0}
    got = order_suggestions([("tell", 1), ("sill", 1), ("seal", 2), ("sell", 0), ("sells", 1), ("sel", 1), ("cell", 1)], df, 6)
    assert got == (Suggestion("sell", 0, 5), Suggestion("sells", 1, 2), Suggestion("sill", 1, 2), Suggestion("tell", 1, 2),
                   Suggestion("cell", 1, 0), Suggestion("sel", 1, 0))
    assert order_suggestions([("b", 1), ("a", 1)], {}, 1) == (Suggestion("a", 1, 0),) and order_suggestions([], df, 5) == ()
    with pytest.raises(AttributeError):
        got[0].token = "x"


def test_the_plan_is_two_int64_and_a_bitmap_per_cell_and_refuses_what_the_call_refuses():
    from legal_rag_amd import _native
    assert (_native.VOCAB_TILE_TERMS, _native.VOCAB_MAX_PATTERN, _native.VOCAB_MAX_ITEMS) == (VC.T, VC.MAX_LEN, VC.MAX_CAP)
    assert (_native.VOCAB_ANY_ONE, _native.VOCAB_ANY_RUN) == (VC.ANY_ONE, VC.ANY_RUN)
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731

    def want(n_terms, n_pat):
        cells = n_pat * max(1, -(-n_terms // VC.T))
        return up(cells * 8) + up((cells + 1) * 8) + up(cells * VC.T // 8) if cells else 0
    for n_terms in (0, 1, VC.T - 1, VC.T, VC.T + 1, 3 * VC.T + 7, 10 ** 6):
        for n_pat in (0, 1, 2, 65, 1168):
            assert _native.vocab_match_plan(n_terms, n_pat) == want(n_terms, n_pat), (n_terms, n_pat)
    assert _native.vocab_match_plan(64, 70_000) == want(64, 70_000) and _native.vocab_match_plan(64, 2 ** 24 - 1) > 0
    for n_terms, n_pat in ((-1, 1), (1, -1), (64, 2 ** 24), (2 * VC.T, 2 ** 23), (2 ** 31, 1)):
        with pytest.raises(_native.NativeError):
            _native.vocab_match_plan(n_terms, n_pat)
    import re
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    header = (root / "include" / "amdretrieval.h").read_text()
    rule = (root / "legal-rag_amd" / "csrc" / "vocab_match_rule.hpp").read_text()
    for name, const, val in (("AMDR_VOCAB_TILE_TERMS", "kVmTile", VC.T), ("AMDR_VOCAB_MAX_PATTERN", "kVmMaxLen", VC.MAX_LEN),
                             ("AMDR_VOCAB_MAX_ITEMS", "kVmMaxCap", VC.MAX_CAP)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == val
        assert int(re.search(rf"constexpr int {const} = (\d+);", rule).group(1)) == val
    # the twin refuses before it touches a device: a null handle
    import ctypes as C
    assert _native.load().amdr_vocab_match(None, None, None, None, None, C.c_int64(0), C.c_int64(0), C.c_int32(1), None, None, None) == -1
    assert np.uint32(VC.ANY_ONE) > 0x10FFFF

"""The host side of highlighting (legal-rag_amd/retrieval/highlight.py), without a GPU: the result types, the slot-table
packer — priority of the `terms` slots, the 32-slot cut, unknown tokens, a term in two slots, loose and phrase-only slots
— the operand arrays, and the character-span mapper, including a text whose lower-casing changes its length."""
import numpy as np
import pytest

from legal_rag_amd.retrieval import highlight as H
from legal_rag_amd.retrieval.terms import Near, NearOf, OneOf, Phrase, PhraseOf, Prefix, Terms

WORDS = ["buyer", "goods", "interest", "interests", "party", "secured", "security", "seller", "sells", "the"] + \
        [f"w{i:02d}" for i in range(40)]
VOCAB = {w: i for i, w in enumerate(WORDS)}
IDF = {w: 1.0 + 0.01 * i for i, w in enumerate(WORDS)}  # the later the word, the heavier
SORTED = sorted(WORDS)


def table(question, terms=None):
    return H.slot_table(question, terms, VOCAB, IDF, SORTED)


def test_highlight_spec_is_frozen_and_validated():
    h = H.Highlight()
    assert (h.window, h.marks, h.question) == (48, 32, True)
    with pytest.raises(Exception):
        h.window = 3
    for bad in (dict(window=0), dict(window=4097), dict(marks=-1), dict(marks=65), dict(window=2.5), dict(window=True),
                dict(question=1)):
        with pytest.raises(ValueError):
            H.Highlight(**bad)
    assert H.Highlight(window=4096, marks=0, question=False).marks == 0


def test_plain_question_tokens_are_loose_slots_in_question_order():
    t = table(["the", "seller", "the", "goods", "unknownword"])
    assert t.labels == ["the", "seller", "goods"] and t.loose == 0b111 and t.seqs == []
    assert t.terms == {VOCAB["goods"]: 2, VOCAB["seller"]: 1, VOCAB["the"]: 0}
    assert list(t.terms) == sorted(t.terms) and t.missing == ["unknownword"]
    assert t.weights == [IDF["the"], IDF["seller"], IDF["goods"]]


def test_terms_slots_come_first_and_none_of_is_never_marked():
    terms = Terms(all_of=[Phrase("security", "interest")], any_of=[Prefix("sell"), OneOf("buyer", "party")], none_of=["goods"])
    t = table(["goods", "interest"], terms)
    assert t.labels == ["security", "interest", "sell!", "(buyer party)", "goods"]
    assert t.seqs == [[0, 1]]
    # the phrase's members are loose only if something else makes them so: "interest" is a question token, "security" not
    assert t.loose == 0b11110
    assert t.terms[VOCAB["seller"]] == 2 and t.terms[VOCAB["sells"]] == 2 and t.terms[VOCAB["buyer"]] == 3
    assert t.weights[2] == max(IDF["seller"], IDF["sells"]) and t.weights[3] == max(IDF["buyer"], IDF["party"])  # a class: the greatest
    assert table([], Terms(none_of=["goods"])).labels == []


def test_near_members_are_loose_and_a_phraseof_is_a_sequence_over_classes():
    terms = Terms(all_of=[Near("buyer", "seller", distance=5), PhraseOf(Prefix("secur"), OneOf("interest", "interests")),
                          NearOf(Prefix("sell"), "goods", distance=3)])
    t = table([], terms)
    assert t.labels == ["buyer", "seller", "secur!", "(interest interests)", "sell!", "goods"]
    assert t.seqs == [[2, 3]] and t.loose == 0b110011
    # a term in two slots goes to the lower one: "seller" is slot 1 (the plain token) and a member of sell! (slot 4)
    assert t.terms[VOCAB["seller"]] == 1 and t.terms[VOCAB["sells"]] == 4
    assert t.terms[VOCAB["secured"]] == 2 and t.terms[VOCAB["security"]] == 2 and t.terms[VOCAB["interests"]] == 3


def test_unknown_tokens_get_no_slot_and_an_unknown_member_drops_the_phrase():
    terms = Terms(all_of=[Phrase("security", "nosuch"), Prefix("zz"), OneOf("nosuch", "buyer")])
    t = table(["nope", "buyer"], terms)
    assert t.labels == ["(nosuch buyer)", "buyer"] and t.seqs == [] and t.loose == 0b11
    assert t.missing == ["nosuch", "zz!", "nope"]
    assert t.terms == {VOCAB["buyer"]: 0}  # the lower slot


def test_the_32_slot_cut_keeps_terms_first_then_the_heaviest_question_tokens():
    terms = Terms(any_of=[f"w{i:02d}" for i in range(30)])
    question = ["the", "buyer", "w39", "goods", "w38"]  # weights: the 1.09, buyer 1.00, w39 1.49, goods 1.01, w38 1.48
    t = table(question, terms)
    assert len(t.labels) == 32 and t.labels[:30] == [f"w{i:02d}" for i in range(30)]
    assert t.labels[30:] == ["w39", "w38"]  # the two heaviest, in question order
    assert t.missing == ["the", "buyer", "goods"]
    assert t.loose == 0xFFFFFFFF
    many = table([], Terms(any_of=[f"w{i:02d}" for i in range(40)] + [Phrase("w35", "w01")]))
    assert many.labels == [f"w{i:02d}" for i in range(32)] and many.seqs == []  # a sequence with a cut member goes
    tie = H.slot_table(["a", "b", "c"], Terms(any_of=[f"w{i:02d}" for i in range(31)]), {**VOCAB, "a": 50, "b": 51, "c": 52},
                       {**IDF, "a": 9.0, "b": 9.0, "c": 9.0}, SORTED)
    assert tie.labels[31] == "a"  # ties to the earliest


def test_pack_tables_lays_the_batch_out_as_the_kernel_reads_it():
    a = table(["goods"], Terms(all_of=[Phrase("security", "interest")]))
    b = table([], None)
    c = table(["buyer", "seller"], Terms(all_of=[Phrase("the", "buyer", "the")]))
    mk_ptr, mk_terms, mk_slot, w, loose, sq_ptr, sq_off, sq_slots = H.pack_tables([a, b, c])
    assert mk_ptr.tolist() == [0, 3, 3, 6] and mk_ptr.dtype == np.int64 and mk_terms.dtype == np.int32
    for q in range(3):
        seg = mk_terms[mk_ptr[q]:mk_ptr[q + 1]]
        assert np.all(np.diff(seg) > 0)
    assert w.shape == (3, 32) and w.dtype == np.float64 and loose.dtype == np.uint32 and loose.tolist() == [0b100, 0, 0b110]
    assert sq_ptr.tolist() == [0, 1, 1, 2] and sq_off.tolist() == [0, 2, 5] and sq_slots.tolist() == [0, 1, 0, 1, 0]


def test_char_spans_find_each_token_in_order():
    text = "The Seller's goods; the SELLER sells."
    toks = ["the", "seller's", "goods", "the", "seller", "sells"]
    spans = H.char_spans(text, toks, lowered=True)
    assert [text[a:b].lower() for a, b in spans] == toks
    assert spans[3] == (20, 23) and spans[4] == (24, 30)  # the second "the", not the first again
    assert H.char_spans(text, ["the", "buyer"], lowered=True) is None  # a token that is not there
    assert H.char_spans(text, ["goods", "the", "the", "the"], lowered=True) is None  # not in order
    assert H.char_spans("Seller", ["seller"], lowered=False) is None  # the tokeniser that does not lower-case saw "Seller"
    assert H.char_spans("", [], lowered=True) == []


def test_a_text_whose_lower_casing_changes_its_length_gives_none_fields():
    text = "İstanbul seller"  # "İ".lower() is two code points
    assert len(text.lower()) != len(text)
    assert H.char_spans(text, ["i", "stanbul", "seller"], lowered=True) is None
    t = table(["seller"])
    hl = H.build(t, H.Highlight(window=4, marks=4), [2, 3, 1, 1], 1.07, [1, 1], [[2, 0], [-1, -1], [-1, -1], [-1, -1]], 0, text,
                 ["i", "stanbul", "seller"], True, 3)
    assert hl.window_chars is None and hl.snippet is None
    assert hl.marks == [H.Mark(2, 0, "seller", None, None)]  # the token fields still stand
    assert hl.window_tokens == (0, 3) and hl.found == ["seller"] and hl.n_marks_in_chunk == 1 and not hl.truncated
    d = hl.as_dict()
    assert d["marks"][0] == {"token": 2, "slot": 0, "label": "seller", "char_start": None, "char_end": None}
    assert d["window_chars"] is None and d["snippet"] is None and d["window_tokens"] == [0, 3]


def test_build_centres_the_marks_and_slices_the_snippet():
    words = [f"x{i}" for i in range(20)]
    words[10], words[11] = "security", "interest"
    text = " ".join(w.upper() if i % 2 else w for i, w in enumerate(words))
    t = H.slot_table([], Terms(all_of=[Phrase("security", "interest")]), {"security": 0, "interest": 1}, [2.0, 3.0], [])
    marks = [[10, 0], [11, 1]] + [[-1, -1]] * 2
    hl = H.build(t, H.Highlight(window=6, marks=4), [10, 16, 2, 2], 5.0, [3, 3], marks, 0, text, words, True, 20)
    assert hl.window_tokens == (8, 14)  # the two marks in the middle of six tokens
    assert hl.snippet == text[hl.window_chars[0]:hl.window_chars[1]] and hl.snippet.lower().split() == words[8:14]
    assert [text[m.char_start:m.char_end].lower() for m in hl.marks] == ["security", "interest"]
    assert [m.label for m in hl.marks] == ["security", "interest"] and hl.score == 5.0 and hl.missing == []
    # at the start of the chunk the window is clamped, not shifted out of it; a token count that differs from the index's
    hl = H.build(t, H.Highlight(window=6, marks=4), [1, 7, 1, 1], 2.0, [1, 1], [[1, 0]] + [[-1, -1]] * 3, 0, text, words, True, 20)
    assert hl.window_tokens == (0, 6) and hl.missing == ["interest"]
    hl = H.build(t, H.Highlight(window=6, marks=4), [1, 7, 1, 1], 2.0, [1, 1], [[1, 0]] + [[-1, -1]] * 3, 0, text, words, True, 21)
    assert hl.snippet is None and hl.marks[0].char_start is None and hl.marks[0].token == 1
    # no mark: the head of the chunk
    hl = H.build(t, H.Highlight(window=6, marks=4), [0, 6, 0, 0], 0.0, [0, 0], [[-1, -1]] * 4, 0, text, words, True, 20)
    assert hl.window_tokens == (0, 6) and hl.marks == [] and hl.found == [] and hl.snippet.lower().split() == words[:6]

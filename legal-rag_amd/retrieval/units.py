"""Sentences and paragraphs of a chunk text as BREAK FLAGS beside its tokens: what `Within` (retrieval/terms.py) is
resolved from on the GPU (amdr_bm25_set_breaks, amdr_unit_spans; csrc/unit_span.hip).

No reference counterpart: legalrag's BM25 channel scores bags of words.  The English index drops punctuation when it cuts a
text (text.tokenize_en) and nothing resident says where a sentence or a subsection begins, so the flags are made here, from
the text and the character spans of its tokens (highlight.char_spans), one byte per token:
  bit 0 (1)  the token begins a sentence;
  bit 1 (2)  the token begins a paragraph — and then a sentence too, so a byte is 0, 1 or 3.
The first token of a document begins both whatever its byte says (the kernel forces it; this module leaves it 0).

This is the specification, a rule and not a parser.  The BREAK POSITIONS of a text are
  sentence   the position behind '.', '?' or '!' — once the closing marks  " ' ) ] ” ’ 」 』 ）  directly behind it have been
             absorbed — when whitespace or the end of the text follows; and the position behind '。', '！' or '？', again
             behind absorbed closing marks, unconditionally;
  paragraph  the position behind each '\\n' ("\\r\\n" counts once: only the '\\n' breaks).  A paragraph break is a sentence
             break too.
Token i > 0 gets the flag when a break position e satisfies start[i - 1] < e <= start[i].  A segmenter's own '。' or '\\n'
token, which is in the stream, therefore closes its unit and the next token opens the next one.  "U.S. " and "§ 1-101. "
break: accepted.  "2.5" does not (no whitespace follows the point).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from .highlight import char_spans

SENTENCE, PARAGRAPH = 1, 2  # the bits (unit_span_rule.hpp UsBreak)
_CLOSERS = "\"')]”’」』）"
_ENDS_SPACED = ".?!"
_ENDS_ALWAYS = "。！？"


def break_positions(text: str) -> Tuple[List[int], List[int]]:
    """(sentence break positions, paragraph break positions) of a text, each ascending; a paragraph break is listed among
    the sentence breaks as well."""
    sent: List[int] = []
    para: List[int] = []
    n = len(text)
    for i, ch in enumerate(text):
        if ch == "\n":
            para.append(i + 1)
            sent.append(i + 1)
        elif ch in _ENDS_SPACED or ch in _ENDS_ALWAYS:
            j = i + 1
            while j < n and text[j] in _CLOSERS:
                j += 1
            if ch in _ENDS_ALWAYS or j == n or text[j].isspace():
                sent.append(j)
    sent.sort()
    return sent, para


def break_flags(text: str, tokens: Sequence[str], lowered: bool) -> Tuple[np.ndarray, bool]:
    """(flags u8 [len(tokens)], mapped) of one document: `tokens` is the text cut by the index's document-side tokeniser,
    `lowered` whether that tokeniser saw the lower-cased text (highlight.char_spans).  When the tokens cannot be mapped back
    to the text (char_spans returns None: lower-casing changed its length, or a token is not found in order) the flags are
    all zero and mapped is False: the document is one sentence and one paragraph, and a Within holds there what the
    conjunction holds — never a false negative."""
    flags = np.zeros(len(tokens), dtype=np.uint8)
    if len(tokens) == 0:
        return flags, True
    spans = char_spans(text, tokens, lowered)
    if spans is None:
        return flags, False
    start = np.fromiter((s for s, _ in spans), dtype=np.int64, count=len(spans))
    sent, para = break_positions(text)
    for positions, value in ((sent, SENTENCE), (para, SENTENCE | PARAGRAPH)):
        if positions:
            below = np.searchsorted(np.asarray(positions, dtype=np.int64), start, side="right")  # breaks e <= start[i]
            flags[1:][below[1:] > below[:-1]] |= value
    return flags, True


def unit_ranges(flags: Sequence[int], bit: int) -> List[Tuple[int, int]]:
    """The [begin, end) token ranges of one document's units: a unit begins at token 0 and at every token whose flag has
    `bit` (SENTENCE or PARAGRAPH)."""
    n = len(flags)
    cuts = [0] + [i for i in range(1, n) if int(flags[i]) & bit] + [n]
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]

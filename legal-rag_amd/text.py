"""Tokenisers of the BM25 channel (host side).

Index side, English: lower-cased regex words (legalrag/retrieval/builders/
bm25_builder.py:18-19,39-41).  Index side, Chinese, and EVERY query regardless
of language: `jieba.cut` (bm25_builder.py:43, bm25_retriever.py:73) — note the
reference does NOT lower-case queries, so capitalised English query words never
match the lower-cased English index; that behaviour is kept.

jieba (`jieba>=0.42.1`, requirements.txt) is absent from the build container.
If it is importable it is used.  Otherwise `jieba_cut` restates jieba 0.42.1's
default mode (cut_all=False, HMM=True) for text WITHOUT Han characters, which
needs no dictionary beyond a handful of ASCII entries (restated from the
published algorithm: jieba/__init__.py `cut`/`__cut_DAG`, finalseg `cut`):
  1. split on runs of [\\u4E00-\\u9FD5a-zA-Z0-9+#&._%-]; between such blocks,
     whitespace (\\r\\n or one \\s char) is emitted as a token and every other
     character as its own token;
  2. inside a block made of single-character DAG steps the whole buffer goes
     through finalseg.cut: runs matching [a-zA-Z0-9]+(?:\\.\\d+)?%? are one token
     each, and each maximal run of the remaining characters is one token.
Han runs cannot be segmented without dict.txt.  That case is never silent:
  * default: `jieba_cut` raises `ZhTokenizerUnavailable` when the text holds Han
    characters and neither jieba nor a registered tokenizer is available;
  * `register_tokenizer(fn, name)` plugs in an exact segmenter (a caller that
    has jieba elsewhere, or any jieba-compatible callable);
  * pre-tokenised entry points (`build_bm25_index(..., tokens=)`,
    `BM25Retriever.search(..., tokens=)`) bypass tokenisation altogether;
  * explicit opt-in to the inexact one-character-per-token stand-in:
    `cfg.retrieval.zh_tokenizer = "char"` (or LEGALRAG_ZH_TOKENIZER=char, or
    `mode="char"`): a WARNING is logged once, the index records tokenizer id
    "char" and every consumer reports `zh_exact: False`;
  * explicit opt-in to a dictionary segmenter over the CALLER's dictionary file (jieba's dict.txt format):
    `cfg.retrieval.zh_tokenizer = "dict"` with `cfg.retrieval.zh_dict_file` — `dict_cut` below, jieba's default
    cut (prefix dictionary, word graph, maximum-log-probability route) without its HMM: a run of characters the
    dictionary does not cover comes out one Han character per token.  The index records tokenizer id "dict" and
    every consumer reports `zh_exact: False`.
`dict_cut` and `jieba_cut_restated` are the executable specification of the native tokenisers
(csrc/tokenize_rule.hpp: host and device) in the modes "dict" and "char".
"""
from __future__ import annotations

import logging
import math
import os
import re
from typing import Callable, Dict, Iterable, List, Optional, Union

logger = logging.getLogger(__name__)

try:  # pragma: no cover - not installed in the build container
    import jieba as _jieba
    HAVE_JIEBA = True
except Exception:  # noqa: BLE001
    _jieba = None
    HAVE_JIEBA = False


class ZhTokenizerUnavailable(RuntimeError):
    """Han text needs jieba's dictionary segmentation and none is available."""


_custom_cut: Optional[Callable[[str], List[str]]] = None
_custom_name: Optional[str] = None
_warned_char = False
_warned_dict = False


def register_tokenizer(fn: Optional[Callable[[str], List[str]]], name: str = "custom") -> None:
    """Use `fn(sentence) -> tokens` wherever the reference calls jieba.cut (None removes it)."""
    global _custom_cut, _custom_name
    _custom_cut, _custom_name = fn, (name if fn is not None else None)


def zh_exact() -> bool:
    """True when Han text is segmented by jieba (or a registered exact tokenizer)."""
    return HAVE_JIEBA or _custom_cut is not None


def tokenizer_id(mode: Optional[str] = None) -> str:
    """Id recorded in bm25.pkl next to the index: which segmenter produced its tokens."""
    if _custom_cut is not None:
        return str(_custom_name)
    if HAVE_JIEBA:
        return "jieba"
    m = resolve_mode(mode)
    return m if m in ("char", "dict") else "jieba-restated-ascii"


def resolve_mode(mode: Optional[str]) -> str:
    m = (mode or os.environ.get("LEGALRAG_ZH_TOKENIZER") or "jieba").strip().lower()
    return m if m in ("char", "dict") else "jieba"


def cfg_mode(cfg) -> Optional[str]:
    """`cfg.retrieval.zh_tokenizer` if the (duck-typed) config has it."""
    return getattr(getattr(cfg, "retrieval", None), "zh_tokenizer", None)


def cfg_dict_file(cfg) -> Optional[str]:
    """`cfg.retrieval.zh_dict_file` if the (duck-typed) config has it."""
    return getattr(getattr(cfg, "retrieval", None), "zh_dict_file", None)


_EN_INDEX_RE = re.compile(r"[A-Za-z0-9]+(?:'[A-Za-z0-9]+)?")
_RE_BLOCK = re.compile(r"([一-鿕a-zA-Z0-9+#&\._%\-]+)", re.U)
_RE_SKIP = re.compile(r"(\r\n|\s)", re.U)
_RE_HAN = re.compile(r"([一-鿕]+)", re.U)
_RE_HAN_ANY = re.compile(r"[一-鿕]", re.U)  # contains_han's test without the group and the run (batch callers)
_RE_ENG = re.compile(r"([a-zA-Z0-9]+(?:\.\d+)?%?)", re.U)
# ASCII multi-character entries of jieba's dict.txt [from memory — verify]
_ASCII_DICT_WORDS = ("AT&T", "C++", "c++", "C#", "c#")


def tokenize_en(text: str) -> List[str]:
    return _EN_INDEX_RE.findall(text.lower())


def _finalseg_cut(buf: str) -> List[str]:
    out: List[str] = []
    for blk in _RE_HAN.split(buf):
        if not blk:
            continue
        if _RE_HAN.match(blk):
            out.extend(list(blk))  # no dictionary / HMM tables: one char per token (inexact)
        else:
            out.extend(x for x in _RE_ENG.split(blk) if x)
    return out


_ASCII_DICT_MARKS = frozenset("&+#")  # every entry of _ASCII_DICT_WORDS holds one of these


def _cut_block(blk: str) -> List[str]:
    if _ASCII_DICT_MARKS.isdisjoint(blk):  # no dictionary word can start anywhere in the block
        return [blk] if len(blk) == 1 else _finalseg_cut(blk)
    out: List[str] = []
    buf = ""
    i = 0
    n = len(blk)

    def flush():
        nonlocal buf
        if buf:
            if len(buf) == 1:
                out.append(buf)
            else:
                out.extend(_finalseg_cut(buf))
            buf = ""

    while i < n:
        hit = next((w for w in _ASCII_DICT_WORDS if blk.startswith(w, i)), None)
        if hit:
            flush()
            out.append(hit)
            i += len(hit)
        else:
            buf += blk[i]
            i += 1
    flush()
    return out


def jieba_cut_restated(sentence: str) -> List[str]:
    out: List[str] = []
    for blk in _RE_BLOCK.split(sentence):
        if not blk:
            continue
        if _RE_BLOCK.match(blk):
            out.extend(_cut_block(blk))
        else:
            for x in _RE_SKIP.split(blk):
                if _RE_SKIP.match(x):
                    out.append(x)
                else:
                    out.extend(list(x))
    return out


def contains_han(sentence: str) -> bool:
    return _RE_HAN.search(sentence) is not None


# ---- the dictionary segmenter ("dict" mode) ---------------------------------------------------------------------------
# jieba 0.42.1's default cut restated from the published algorithm (jieba/__init__.py: gen_pfdict, get_DAG, calc,
# __cut_DAG) [from memory — verify], minus the HMM: what __cut_DAG hands to finalseg.cut goes through _finalseg_cut
# above (one Han character per token).  The hard-coded _ASCII_DICT_WORDS are NOT consulted here: only the caller's
# dictionary is (jieba's own dict.txt holds them).
class HanDict:
    """A prefix dictionary: `lfreq` maps every word AND every proper prefix of a word to its frequency (0 for a key
    that is only a prefix), `total` is the sum of the frequencies of all lines.  Per key with freq > 0,
    logw[key] = log(freq) - log(total); logw_unknown = 0.0 - log(total).  Native code receives these doubles as they
    are and never takes a logarithm, so its route is this module's bit for bit."""

    def __init__(self, lfreq: Dict[str, int], total: int):
        if total <= 0:
            raise ValueError("Han dictionary: the total frequency must be > 0")
        self.lfreq = dict(lfreq)
        self.total = int(total)
        logtotal = math.log(self.total)
        self.logw = {w: math.log(f) - logtotal for w, f in self.lfreq.items() if f > 0}
        self.logw_unknown = 0.0 - logtotal

    def native_tables(self):
        """(keys, logw f64 [n], is_word u8 [n], logw_unknown) for _native.Tokenizer(han=): every key of lfreq, its
        logw (logw_unknown for a frequency-0 key) and the flag freq > 0."""
        import numpy as np
        keys = list(self.lfreq)
        logw = np.fromiter((self.logw.get(k, self.logw_unknown) for k in keys), dtype=np.float64, count=len(keys))
        word = np.fromiter((self.lfreq[k] > 0 for k in keys), dtype=np.uint8, count=len(keys))
        return keys, logw, word, self.logw_unknown


def load_han_dict(path_or_lines: Union[str, os.PathLike, Iterable[str]]) -> HanDict:
    """Parse `word freq [tag]` lines (jieba's dict.txt format; a path, or the lines themselves)."""
    if isinstance(path_or_lines, (str, os.PathLike)):
        with open(path_or_lines, "r", encoding="utf-8") as f:
            lines = f.read().splitlines()
    else:
        lines = list(path_or_lines)
    lfreq: Dict[str, int] = {}
    total = 0
    for lineno, line in enumerate(lines, 1):
        parts = line.split()
        if not parts:
            continue
        if len(parts) < 2 or not parts[1].isascii() or not parts[1].isdigit():
            raise ValueError(f"Han dictionary line {lineno}: expected 'word freq [tag]', got {line!r}")
        word, freq = parts[0], int(parts[1])
        lfreq[word] = freq
        total += freq
        for ch in range(1, len(word)):
            if word[:ch] not in lfreq:
                lfreq[word[:ch]] = 0
    return HanDict(lfreq, total)


def _dict_cut_block(blk: str, d: HanDict, stats: Optional[dict]) -> List[str]:
    n = len(blk)
    lfreq, logw, unknown = d.lfreq, d.logw, d.logw_unknown
    dag: List[List[int]] = []
    for k in range(n):
        ends = []
        i = k
        while i < n and blk[k:i + 1] in lfreq:
            if lfreq[blk[k:i + 1]] > 0:
                ends.append(i)
            i += 1
        dag.append(ends or [k])
    route: List[tuple] = [(0.0, 0)] * (n + 1)
    for idx in range(n - 1, -1, -1):
        cands = [(logw.get(blk[idx:x + 1], unknown) + route[x + 1][0], x) for x in dag[idx]]
        route[idx] = max(cands)
        if stats is not None and sum(1 for c in cands if c[0] == route[idx][0]) > 1:
            stats["ties"] = stats.get("ties", 0) + 1
    out: List[str] = []
    buf = ""

    def flush():
        nonlocal buf
        if not buf:
            return
        if len(buf) == 1:
            out.append(buf)
        elif lfreq.get(buf, 0) > 0:  # the buffer of single steps is itself a word: every character on its own
            out.extend(buf)
            if stats is not None:
                stats["bufword"] = stats.get("bufword", 0) + 1
        else:
            out.extend(_finalseg_cut(buf))
            if stats is not None:
                stats["finalseg"] = stats.get("finalseg", 0) + 1
        buf = ""

    x = 0
    while x < n:
        y = route[x][1] + 1
        if y - x == 1:
            buf += blk[x]
        else:
            flush()
            out.append(blk[x:y])
            if stats is not None:
                stats["words"] = stats.get("words", 0) + 1
        x = y
    flush()
    return out


def dict_cut(sentence: str, d: HanDict, stats: Optional[dict] = None) -> List[str]:
    """jieba's default cut over the caller's dictionary, without the HMM (the module docstring).  `stats`, when
    given, counts `ties` (positions where two candidates of the route had the same value), `bufword` (a buffer of
    single steps that is itself a word), `finalseg` (a buffer handed to _finalseg_cut) and `words` (steps longer than
    one character)."""
    out: List[str] = []
    for blk in _RE_BLOCK.split(sentence):
        if not blk:
            continue
        if _RE_BLOCK.match(blk):
            out.extend(_dict_cut_block(blk, d, stats))
        else:
            for x in _RE_SKIP.split(blk):
                if _RE_SKIP.match(x):
                    out.append(x)
                else:
                    out.extend(list(x))
    return out


def han_cut(sentence: str, mode: str, d: Optional[HanDict] = None) -> List[str]:
    """What the native tokenisers emit in `mode` ("char" | "dict"): text without Han characters by the exact
    restatement whatever the mode, Han text one character per token ("char") or by dict_cut ("dict")."""
    if mode == "dict" and contains_han(sentence):
        if d is None:
            raise ValueError("zh_tokenizer='dict' needs a dictionary (cfg.retrieval.zh_dict_file)")
        return dict_cut(sentence, d)
    return jieba_cut_restated(sentence)


def require_dict(mode: Optional[str], dict_file: Optional[str]) -> None:
    """ValueError when `mode` resolves to "dict", no exact segmenter takes precedence and there is no dictionary."""
    if resolve_mode(mode) == "dict" and not zh_exact():
        han_dict_for(dict_file)


_han_dicts: Dict[tuple, HanDict] = {}


def han_dict_for(path: Optional[str]) -> HanDict:
    """The dictionary of `path`, parsed once per (path, mtime)."""
    if not path:
        raise ValueError("zh_tokenizer='dict' needs cfg.retrieval.zh_dict_file (a dictionary in jieba's dict.txt format)")
    key = (str(path), os.stat(path).st_mtime)
    d = _han_dicts.get(key)
    if d is None:
        _han_dicts.clear()
        d = _han_dicts[key] = load_han_dict(path)
    return d


def jieba_cut(sentence: str, mode: Optional[str] = None, dict_file: Optional[str] = None) -> List[str]:
    """`list(jieba.cut(sentence))`: a registered tokenizer, else the wheel, else — for text
    without Han characters only — the exact restatement.  Han text without a segmenter raises
    ZhTokenizerUnavailable unless a stand-in was chosen explicitly (`mode` / LEGALRAG_ZH_TOKENIZER):
    "char", one character per token, or "dict", dict_cut over the dictionary at `dict_file`
    (ValueError without one); that choice is logged once."""
    global _warned_char, _warned_dict
    if _custom_cut is not None:
        return list(_custom_cut(sentence))
    if HAVE_JIEBA:
        return list(_jieba.cut(sentence))
    if not contains_han(sentence):
        return jieba_cut_restated(sentence)
    if resolve_mode(mode) == "dict":
        d = han_dict_for(dict_file)
        if not _warned_dict:
            _warned_dict = True
            logger.warning("[BM25] jieba is not importable: Han text is segmented over %s without jieba's HMM "
                           "(zh_tokenizer='dict'). zh BM25 results differ from the reference; zh_exact=False", dict_file)
        return dict_cut(sentence, d)
    if resolve_mode(mode) != "char":
        raise ZhTokenizerUnavailable(
            "text contains Han characters but jieba is not importable: BM25 tokens would differ from the "
            "reference (bm25_builder.py:43, bm25_retriever.py:73). Install jieba, call "
            "legal_rag_amd.text.register_tokenizer(fn), pass pre-tokenised input (tokens=...), or opt in to the "
            "inexact one-character-per-token stand-in with cfg.retrieval.zh_tokenizer='char' / "
            "LEGALRAG_ZH_TOKENIZER=char, or to the dictionary segmenter with zh_tokenizer='dict' and zh_dict_file")
    if not _warned_char:
        _warned_char = True
        logger.warning("[BM25] jieba is not importable: Han text is tokenised one character per token "
                       "(zh_tokenizer='char'). zh BM25 results differ from the reference; zh_exact=False")
    return jieba_cut_restated(sentence)


_RE_ZH = re.compile(r"[一-鿿]")
_RE_LATIN = re.compile(r"[A-Za-z]")


def detect_lang(text: str) -> str:
    """legalrag/utils/lang.py:9-15."""
    if not text:
        return "zh"
    return "en" if len(_RE_LATIN.findall(text)) > len(_RE_ZH.findall(text)) else "zh"

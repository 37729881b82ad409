"""Inputs for the Han modes of the BM25 query tokenisers (csrc/tokenize_rule.hpp: "char" and "dict"), whose executable
specification is legal-rag_amd/text.py (jieba_cut_restated, dict_cut).

What the dictionary route does depends on the DICTIONARY as much as on the text: random text over a random dictionary
almost never has two candidates of exactly the same fp64 value, and almost never leaves a buffer of single steps that is
itself a word.  The dictionaries built here make both common:
  * a word and its reverse carry the same frequency, so a text that can be cut "XY | Z" or "X | YZ" has two routes whose
    values are the same two doubles added in the other order — and often the same double;
  * four of the eight Han characters are very frequent as single characters, so the route prefers "X", "Y" to a rare
    word "XY" and the buffer "XY" is then found to be a word (emitted per character, not through finalseg).

Not a test module (no test_ prefix): tests/test_han_tokenizer.py runs these on the CPU against the specification,
tests/test_han_rule_host.py feeds them to the sanitised host program, tests/test_han_tokenizer_gpu.py compares the
device with the host on them.
"""
from __future__ import annotations

import json
from collections import Counter
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"

# ---------------------------------------------------------------------------------------------------------------------
# the known answers (worked by hand from the rule; total frequency 9246)
KNOWN_DICT_LINES = ["合同 5", "合同法 3", "法律 6", "同法 5", "人民 4", "民法 4", "人 4096", "民 4096", "C++ 2", "ab 1",
                    "a 512", "b 512", "条款 0"]
KNOWN_TOTAL = 9246
KNOWN_DICT_ANSWERS = [
    ("合同法律", ["合同", "法律"]),
    ("合同法", ["合同法"]),
    ("人民法", ["人", "民法"]),
    ("人民", ["人", "民"]),  # the route prefers the frequent single characters; the buffer 人民 is a word: per character
    ("第3.5%条 C++法律", ["第", "3.5%", "条", " ", "C++", "法律"]),
    ("ab合同", ["a", "b", "合同"]),
    ("abc", ["abc"]),
    ("条款", ["条", "款"]),  # a frequency-0 key is a prefix, not a word
    ("合同\r\n法律，律", ["合同", "\r\n", "法律", "，", "律"]),
    ("x合y同", ["x", "合", "y", "同"]),
]
KNOWN_CHAR_ANSWERS = [("第3.5%条 C++法律", ["第", "3.5%", "条", " ", "C++", "法", "律"])]

LONG_HAN_RUN = "合同法律人民" * 166 + "合同法律"  # 1000 Han characters = 3000 bytes, one block


def adversary_texts():
    """The edge cases of the rule, for the known-answer dictionary (and any other)."""
    out = ["", "合", LONG_HAN_RUN]
    assert len(LONG_HAN_RUN.encode()) == 3000
    out += [f"合同{m}法律" for m in "+#&._%-"] + [f"{m}合同" for m in "+#&._%-"] + [f"法律{m}" for m in "+#&._%-"]
    out += ["合同\r\n法律", "合同　法律", "合同\x85法律", "合同 法律", "合同\r法律\n\n人民", "人民 \t 民法"]
    out += ["合é同", "é合同", "合同é", "合\U0001F600同", "\U0001F600合同", "合同\U0001F600", "aé合\U0001F600b同"]
    out += ["鿕鿖", "鿖鿕", "合鿕同", "合鿖同", "一䷿一", "一合同鿕"]
    out += ["合同", "合同法", "合同法律", "同法律", "合同合同法"]           # a word that is a proper prefix of another
    out += ["条款", "条", "条款条款", "条款法律", "条合同"]                 # a key of frequency 0 (a prefix only)
    out += ["人合同法", "x 合同法", "x，合同法", "法律合同法", "3.5%合同法"]  # the longest word at the end of a block / text
    out += ["C++法律", "法律C++", "c#合同", "AT&T人民", "a+b合", "ab", "abab合同ab", "3.5%", "v1.2.3条", "第12条第3.5%款"]
    out += ["人民人民人民", "民人民人", "合 同 法", "，，合同。。", "合同。法律？人民！", "\r\n", "\n\r", " "]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the fuzz: 8 Han characters, a dictionary of about 48 keys over them with exact ties built in
FUZZ_HAN = list("合同法律人民条款")
FUZZ_EXTRA = list("aB3.%+#&") + [" ", "\r", "\n", "，", "　", "é", "\U0001F600", "-", "_"]
FUZZ_SEED = 20


def fuzz_dict_lines(seed: int = FUZZ_SEED):
    """Four single Han characters at frequency 4096; words of 2-4 characters at frequencies from {1, 4, 64}, each word's
    reverse entered with the SAME frequency (exact fp64 ties between the two cuts of an overlap)."""
    rng = np.random.default_rng(seed)
    lines = [f"{c} 4096" for c in FUZZ_HAN[:4]]
    words = {}
    while len(words) < 28:
        n = int(rng.integers(2, 5))
        alphabet = FUZZ_HAN if rng.random() < 0.85 else FUZZ_HAN + list("aB3")
        w = "".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=n))
        if w in words or w[::-1] in words:
            continue
        f = int((1, 4, 64)[int(rng.integers(0, 3))])
        words[w] = f
        if w[::-1] != w:
            words[w[::-1]] = f
    return lines + [f"{w} {f}" for w, f in words.items()]


def fuzz_texts(seed: int = FUZZ_SEED, count: int = 2000):
    """`count` strings of 0-40 code points: half over the 8 Han characters only, half over those and FUZZ_EXTRA."""
    rng = np.random.default_rng(seed + 1)
    out = []
    for i in range(count):
        alphabet = FUZZ_HAN if i % 2 == 0 else FUZZ_HAN + FUZZ_EXTRA
        out.append("".join(alphabet[int(j)] for j in rng.integers(0, len(alphabet), size=int(rng.integers(0, 41)))))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the fixture corpus
def law_zh_texts():
    path = GOLDEN / "corpus" / "law_zh.jsonl"
    return [json.loads(line)["text"] for line in path.read_text(encoding="utf-8").splitlines() if line.strip()]


def law_zh_sentences(texts, count: int, seed: int = 3):
    """`count` sentences of the corpus (split at 。；：), drawn with a fixed seed: Han queries of a few dozen characters."""
    import re
    sents = [s for t in texts for s in re.split(r"(?<=[。；：])", t) if 4 <= len(s) <= 120]
    rng = np.random.default_rng(seed)
    return [sents[int(i)] for i in rng.integers(0, len(sents), size=count)]


def ngram_dict_lines(texts, top: int = 400):
    """A dictionary made of the corpus itself: its `top` most frequent 2-4-character Han n-grams with their counts."""
    import re
    counts = Counter()
    for t in texts:
        for run in re.findall("[一-鿕]+", t):
            for n in (2, 3, 4):
                counts.update(run[i:i + n] for i in range(len(run) - n + 1))
    return [f"{w} {c}" for w, c in sorted(counts.items(), key=lambda kv: (-kv[1], kv[0]))[:top]]


def pack(texts):
    """(blob bytes, offsets i64 [n + 1]) of the texts back to back."""
    enc = [t.encode("utf-8") for t in texts]
    offs = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum([len(e) for e in enc], out=offs[1:])
    return b"".join(enc), offs

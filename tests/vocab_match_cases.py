"""The plain evaluator of the vocabulary patterns and the case families of the tests of amdr_vocab_match (pure Python and
numpy; nothing of the package's rule is used here: the wildcard is a translation to `re.fullmatch`, the distance a
full-matrix optimal string alignment).  Every edge case carries a certificate that it has the answer it was built for."""
import re

import numpy as np

T = 8192        # AMDR_VOCAB_TILE_TERMS
MAX_LEN = 64    # AMDR_VOCAB_MAX_PATTERN
MAX_CAP = 4096  # AMDR_VOCAB_MAX_ITEMS
ANY_ONE, ANY_RUN = 0x110000, 0x110001
WILDCARD, FUZZY = 0, 1


# ---- the plain evaluator ------------------------------------------------------------------------------------------------------
def osa(a: str, b: str) -> int:
    """The optimal-string-alignment distance over code points, full matrix."""
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        D[i][0] = i
    for j in range(len(b) + 1):
        D[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
            if i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                D[i][j] = min(D[i][j], D[i - 2][j - 2] + 1)
    return D[len(a)][len(b)]


def levenshtein(a: str, b: str) -> int:
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[len(b)]


def wildcard_regex(pattern: str):
    return re.compile("".join(".*" if c == "*" else "." if c == "?" else re.escape(c) for c in pattern), re.S)


def fits(pattern, token: str):
    """(whether `token` fits the pattern, its distance): pattern is ("w", text) or ("f", text, edits).  The empty token
    fits nothing."""
    if not token:
        return False, 0
    if pattern[0] == "w":
        return wildcard_regex(pattern[1]).fullmatch(token) is not None, 0
    d = osa(pattern[1], token)
    return d <= pattern[2], d


def evaluate(vocab, patterns, item_cap):
    """(ids i32 [n, cap], dist u8 [n, cap], n_match i64 [n]) as amdr_vocab_match promises them, by the plain evaluator."""
    n = len(patterns)
    ids = np.full((n, item_cap), -1, np.int32)
    dist = np.full((n, item_cap), 255, np.uint8)
    n_match = np.zeros(n, np.int64)
    for p, pat in enumerate(patterns):
        regex = wildcard_regex(pat[1]) if pat[0] == "w" else None
        k = 0
        for t, tok in enumerate(vocab):
            if not tok:
                continue
            if regex is not None:
                hit, d = regex.fullmatch(tok) is not None, 0
            elif abs(len(tok) - len(pat[1])) > pat[2]:  # (the distance is at least the difference of the lengths)
                continue
            else:
                d = osa(pat[1], tok)
                hit = d <= pat[2]
            if hit:
                if k < item_cap:
                    ids[p, k], dist[p, k] = t, d
                k += 1
        n_match[p] = k
    return ids, dist, n_match


def native_pattern(pat):
    """(kind, arg, code points) of an evaluator pattern."""
    if pat[0] == "w":
        return WILDCARD, 0, [ANY_ONE if c == "?" else ANY_RUN if c == "*" else ord(c) for c in pat[1]]
    return FUZZY, pat[2], [ord(c) for c in pat[1]]


def pack(patterns):
    """(pat_cp u32, pat_ptr i64, pat_kind i32, pat_arg i32) of evaluator patterns."""
    nat = [native_pattern(p) for p in patterns]
    ptr = np.zeros(len(nat) + 1, np.int64)
    np.cumsum([len(x[2]) for x in nat], out=ptr[1:])
    return (np.asarray([c for x in nat for c in x[2]], np.uint32), ptr, np.asarray([x[0] for x in nat], np.int32),
            np.asarray([x[1] for x in nat], np.int32))


# ---- vocabularies --------------------------------------------------------------------------------------------------------------
def filler(n, seed=0):
    """n distinct tokens over {x, y, z, w} of 9 to 12 characters: none within two edits of a probe word below (certified
    by the callers that rely on it)."""
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < n:
        tok = "".join("xyzw"[i] for i in rng.integers(0, 4, size=int(rng.integers(9, 13))))
        if tok not in seen:
            seen.add(tok)
            out.append(tok)
    return out


def sized_vocab(n):
    """A vocabulary of n tokens with the probe word "zebra" at the ids 0, T - 1, T and n - 1 that exist and a near miss
    ("zebar", one transposition) beside each where there is room.  Certificate: the filler holds no 'e', 'b', 'r' or 'a',
    so only the planted tokens lie within two edits of the probe."""
    vocab = filler(n, seed=n)
    at = sorted({i for i in (0, T - 1, T, n - 1) if 0 <= i < n})
    for i in at:
        vocab[i] = "zebra"
    for i in at:
        if i + 1 < n and i + 1 not in at:
            vocab[i + 1] = "zebar"
    assert all(osa("zebra", t) > 2 for i, t in enumerate(vocab) if t not in ("zebra", "zebar"))
    return vocab, at


SIZES = (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7)


# ---- Fuzzy edits: each kind at the first, a middle and the last position ----------------------------------------------------------
WORD = "warranty"


def edit_cases():
    """[(name, token, expected distance from WORD)] with the certificate asserted."""
    w = WORD
    mid = len(w) // 2
    out = []
    for name, at in (("first", 0), ("middle", mid), ("last", len(w) - 1)):
        out.append((f"insertion-{name}", w[:at] + "q" + w[at:], 1))
        out.append((f"deletion-{name}", w[:at] + w[at + 1:], 1))
        out.append((f"substitution-{name}", w[:at] + "q" + w[at + 1:], 1))
    out.append(("insertion-behind", w + "q", 1))
    for name, at in (("first", 0), ("middle", mid), ("last", len(w) - 2)):
        assert w[at] != w[at + 1]
        out.append((f"transposition-{name}", w[:at] + w[at + 1] + w[at] + w[at + 2:], 1))
    out += [("identity", w, 0), ("two-substitutions", "q" + w[1:-1] + "q", 2), ("three-substitutions", "q" + w[1:3] + "q" + w[4:-1] + "q", 3),
            # a transposition BESIDE a substitution: two edits; and "ca" -> "abc", where unrestricted Damerau says 2
            ("transposition+substitution", w[1] + w[0] + "q" + w[3:], 2),
            ("two-transpositions", w[1] + w[0] + w[2:-2] + w[-1] + w[-2], 2)]
    for name, tok, d in out:
        assert osa(w, tok) == d, (name, tok, osa(w, tok), d)
    assert osa("ca", "abc") == 3 and osa("recieve", "receive") == 1 and levenshtein("recieve", "receive") == 2
    return out


# ---- token lengths around a pattern of m code points -----------------------------------------------------------------------------
def length_cases(m=6, e=2):
    """Tokens of 0, 1, m - e - 1, m - e, m, m + e, m + e + 1 and 300 characters against the pattern "a" * m: a token of n
    characters 'a' is at distance |n - m| exactly."""
    pat = "a" * m
    toks = ["", "a", "a" * (m - e - 1), "a" * (m - e), "a" * m, "a" * (m + e), "a" * (m + e + 1), "a" * 300]
    for t in toks:
        assert osa(pat, t) == abs(len(t) - m)
    return pat, toks


# ---- Wildcard forms --------------------------------------------------------------------------------------------------------------
WILD_VOCAB = ["a", "aa", "aba", "ab", "abab", "ababc", "abxababc", "xabyabz", "sell", "seller", "sill", "sll", "lessee",
              "assignee", "ee", "e", "wom\U00020000n", "woman", "women", "womn", "a?", "?", "", "in\nment", "inment"]
WILD_PATTERNS = ["s?ll", "a??", "*ee", "s?ll*", "se*r", "in*ment", "**ee", "a*a", "*ab*ab?", "wom?n", "?e", "a?", "*a*", "s*l*l*", "?*e"]


def wild_certificates():
    ev = lambda p, t: fits(("w", p), t)[0]  # noqa: E731
    assert ev("a*a", "aa") and not ev("a*a", "a")
    assert ev("*ab*ab?", "abxababc") and ev("*ab*ab?", "ababc") and not ev("*ab*ab?", "abab")
    assert ev("wom?n", "wom\U00020000n") and not ev("wom?n", "womn")
    assert ev("a?", "a?") and ev("?e", "ee") and not ev("?e", "e") and not ev("*ee", "")
    assert ev("in*ment", "in\nment") and ev("**ee", "ee") and not ev("**ee", "e")


# ---- code points, not bytes --------------------------------------------------------------------------------------------------------
UNI_VOCAB = ["中文", "国文", "中", "cafe", "café", "caf", "a\U00020000c", "abc", "a中c", "ac", "é", "e", "\U00020000\U00020001"]
UNI_PATTERNS = [("f", "中文", 1), ("f", "cafe", 1), ("f", "café", 1), ("w", "a?c"), ("f", "\U00020000\U00020001", 1), ("w", "*文"),
                ("f", "éa", 1), ("w", "caf?")]


def unicode_certificates():
    assert osa("中文", "国文") == 1 and osa("cafe", "café") == 1 and len("café".encode()) != len("cafe".encode())
    assert fits(("w", "a?c"), "a\U00020000c")[0] and len("\U00020000".encode()) == 4
    assert osa("éa", "é") == 1 and osa("éa", "e") == 2  # (bytes would say é -> e is two edits more)


# ---- truncation ---------------------------------------------------------------------------------------------------------------------
def cap_vocab(matches, n=T + 50):
    """A vocabulary of n tokens of which exactly `matches` fit Wildcard("quo*") and lie within one edit of "quorum",
    spread over both tiles.  Certificate: counted by the plain evaluator."""
    vocab = filler(n, seed=matches)
    spots = [3, 500, T - 1, T, T + 7, T + 8, T + 49, 9, 10, 11, 12][:matches]
    for j, i in enumerate(sorted(spots)):
        vocab[i] = "quorum" if j % 2 == 0 else "quorums" if j % 4 == 1 else "quorun"
    assert sum(fits(("w", "quo*"), t)[0] for t in vocab) == matches
    assert sum(fits(("f", "quorum", 1), t)[0] for t in vocab) == matches
    return vocab


# ---- garbage for the device form -------------------------------------------------------------------------------------------------
def garbage_patterns():
    """(pat_cp, pat_ptr, pat_kind, pat_arg, the indices that are VALID) — every other pattern breaks one promise of the
    rule and names nothing: a kind out of range, edits 0 and 3, a reserved value in a Fuzzy, a Wildcard without a literal,
    a value that is no code point, a Wildcard with an argument, and spans that are negative, reversed, too long or
    beyond cp_total."""
    abc = [ord(c) for c in "abc"]
    cp = abc + abc + abc + abc + [ord("a"), ANY_ONE, ord("c")] + [ANY_ONE, ANY_ONE, ANY_RUN] + [ord("a"), 0x110002] + abc + abc
    ptr = [0, 3, 6, 9, 12, 15, 18, 20, 23, 26]
    kind = [2, -1, FUZZY, FUZZY, FUZZY, WILDCARD, WILDCARD, WILDCARD, FUZZY]
    arg = [0, 0, 0, 3, 1, 0, 0, 1, 1]
    return (np.asarray(cp, np.uint32), np.asarray(ptr, np.int64), np.asarray(kind, np.int32), np.asarray(arg, np.int32), [8])


def garbage_spans(cp_total):
    """pat_ptr arrays of four Fuzzy patterns whose spans break the promise: each names nothing."""
    return np.asarray([-5, 6, 3, 3 + 70, cp_total + 1000], np.int64)

"""Mixed constraint expressions end to end: Terms -> pack() -> HybridEngine.term_scopes -> the scope table, against a plain
evaluator.  A seeded word corpus of stem families, a seeded grammar over all seven member kinds (token, Phrase, Near, Prefix,
OneOf, PhraseOf, NearOf) in all three fields, alone and in tuple groups, and the reference: `holds` — one member on one
document's words, written from the docstrings of retrieval/terms.py, brute force over every window — plus set algebra over
the documents.  It shares nothing with Terms.matches, the `within` methods, pack() or the rule headers: no posting list, no
driver, no term id, no bound.  Plain Python and numpy; only retrieval.terms (the classes, pack for the generator's refusal)
and retrieval.scope are imported.

The CPU test (tests/test_query_fuzz.py) asserts the certificates below — what the corpus holds, that the batches reach every
resolver with lists on both sides of a candidate tile, and that each of six deliberately WRONG evaluators changes the
expected table of several constraints, so a resolver with that mistake could not pass — and pack()'s invariants against the
evaluator; the GPU test (tests/test_query_fuzz_gpu.py) compares the device tables with `expected_table`.
"""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from legal_rag_amd.retrieval.scope import Scope
from legal_rag_amd.retrieval.terms import Near, NearOf, OneOf, Phrase, PhraseOf, Prefix, Terms, pack
from phrase_cases import SeqCorpus

TILE = 256  # candidates per block of the span resolvers (kPhTile)

# ---- the corpus ----------------------------------------------------------------------------------------------------------
FAMILIES = (("sel", "sell", "seller", "sellers", "selling", "selx"), ("buy", "buyer", "buyers", "buying"),
            ("good", "goods", "goodwill"), ("sec", "secur", "secure", "secured", "security"),
            ("int", "inter", "interest", "interests"), ("con", "cont", "contra", "contract", "contracts"))
PLAIN = tuple(f"w{i:02d}" for i in range(33))
VOCAB = tuple(w for fam in FAMILIES for w in fam) + PLAIN  # token -> term id: its place here
UNKNOWN = "zzz"                                            # in no document
NO_STEM = "qq"                                             # no token starts with it
STEMS = ("s", "se", "sel", "sell", "seller", "sellers", "selx", "b", "buy", "buyer", "go", "good", "goods", "sec", "secur",
         "secure", "int", "inter", "interest", "con", "cont", "contra", "contract", "w", "w0", "w1", "w3", "w32", NO_STEM)
LENGTHS = (0, 1, 2, 5, 20, 63, 64, 65, 130, 300)           # 63 / 64 / 65: the lane stride of the span walk
LENGTH_P = (0.03, 0.04, 0.05, 0.08, 0.25, 0.12, 0.12, 0.12, 0.12, 0.07)
DISTANCES = (1, 2, 5, 30, 255)
N_DOCS = 900
NEW_TOKENS = ("sells", "sellable", "buyout", "goodness", "securities", "contractor", "w99")  # what the edits bring in


def make_words(seed: int = 2024, n_docs: int = N_DOCS) -> List[List[str]]:
    """The documents as words: Zipf-like token frequencies over a seeded permutation of the vocabulary (family members land
    on common and on rare ranks alike), lengths from LENGTHS."""
    rng = np.random.default_rng(seed)
    rank = rng.permutation(len(VOCAB))
    p = 1.0 / (1.0 + rank)
    p /= p.sum()
    lens = rng.choice(LENGTHS, size=n_docs, p=LENGTH_P)
    return [[VOCAB[t] for t in rng.choice(len(VOCAB), size=int(n), p=p)] for n in lens]


_WORLD: Dict[str, object] = {}


def world():
    """(SeqCorpus, its documents as words, {token: term id}, {token: document frequency}) of the base corpus, built once."""
    if "base" not in _WORLD:
        words = make_words()
        vocab = {w: t for t, w in enumerate(VOCAB)}
        corpus = SeqCorpus("fuzz", len(VOCAB), [[vocab[w] for w in d] for d in words])
        df = {w: int(x) for w, x in zip(VOCAB, corpus.df())}
        _WORLD["base"] = (corpus, words, vocab, df)
    return _WORLD["base"]


def corpus_certificates() -> None:
    corpus, words, vocab, df = world()
    assert corpus.n_docs == N_DOCS and len(VOCAB) == 60 and len(set(VOCAB)) == 60 and len(FAMILIES) == 6
    assert {len(d) for d in words} == set(LENGTHS)                      # every length, the empty document among them
    assert max(df.values()) > 2 * TILE + 1 and 0 < min(df.values()) < TILE  # three candidate tiles | less than one
    assert sum(1 for x in df.values() if x > 2 * TILE + 1) >= 3 and sum(1 for x in df.values() if x < TILE) >= 10
    assert UNKNOWN not in vocab and not any(w.startswith(NO_STEM) for w in VOCAB)
    named = {s: [w for w in VOCAB if w.startswith(s)] for s in STEMS}
    assert named[NO_STEM] == [] and named["sellers"] == ["sellers"] and named["selx"] == ["selx"]  # none | exactly one
    assert set(named["seller"]) < set(named["sell"]) < set(named["sel"]) < set(named["se"])  # nested
    assert named["se"] == named["s"]  # two stems, one set of tokens: one union
    assert set(named["sec"]) & set(named["se"]) and not set(named["sec"]) & set(named["sel"])  # overlapping | disjoint
    assert len(named["w"]) == len(PLAIN) and not any(t in vocab or any(w.startswith(t) for w in VOCAB) for t in NEW_TOKENS[:-1])


# ---- the reference -------------------------------------------------------------------------------------------------------
WRONG = ("distance", "unordered", "prefix", "none_of", "cross", "somewhere")  # the deliberately wrong evaluators


def fills(slot, token: str, wrong: Optional[str] = None) -> bool:
    """Whether `token` fills `slot` (a str, a Prefix or a OneOf).  wrong == "prefix": a Prefix read as the exact token."""
    if isinstance(slot, str):
        return token == slot
    if isinstance(slot, Prefix):
        return token == slot.stem if wrong == "prefix" else token.startswith(slot.stem)
    return any(fills(m, token, wrong) for m in slot.members)


def slots_of(member) -> tuple:
    return member.tokens if isinstance(member, (Phrase, Near)) else member.members


def holds(member, words: Sequence[str], tail: Sequence[str] = (), wrong: Optional[str] = None, fillers=None) -> bool:
    """Whether the document `words` holds `member`, by the docstrings of terms.py, brute force over every start position and
    every window.  `tail`: tokens behind the document that a window may run into — () for the rule, the next document's
    words for the wrong evaluator "cross".  wrong: None or one of WRONG ("none_of" is a mistake of `expected_rows`).
    fillers: per slot the set of tokens that fill it, if the caller knows them already (a pure function of slot and wrong)."""
    if isinstance(member, (str, Prefix, OneOf)):
        return any(fills(member, t, wrong) for t in words)
    seq, own = list(words) + list(tail), len(words)
    slots = slots_of(member)
    M = len(slots)
    if fillers is None:
        have = set(seq)
        fillers = [{t for t in have if fills(s, t, wrong)} for s in slots]
    fl = [[t in f for t in seq] for f in fillers]  # fl[j][q]: the token at position q fills slot j
    if not all(any(x) for x in fl):
        return False  # (a slot that no token of the document fills is filled in no window of it)
    if isinstance(member, (Phrase, PhraseOf)):
        return any(all(fl[j][p + j] for j in range(M)) for p in range(min(own, len(seq) - M + 1)))
    n = member.distance + (1 if wrong == "distance" else 0)
    ordered = member.ordered and wrong != "unordered"
    for s in range(own):
        e = min(s + n + 1, len(seq))  # the run of at most n + 1 tokens from s
        if ordered:  # p0 = s; every later member at its earliest position behind the one before
            if not fl[0][s]:
                continue
            j = 1
            for q in range(s + 1, e):
                if fl[j][q]:
                    j += 1
                    if j == M:
                        return True
        elif wrong == "somewhere" and isinstance(member, NearOf):
            if all(any(fl[j][s:e]) for j in range(M)):
                return True
        elif isinstance(member, Near):  # every distinct token at least as many times as the Near names it
            if all(sum(fl[j][s:e]) >= slots.count(slots[j]) for j in range(M)):
                return True
        else:  # the members on DISTINCT positions: every assignment, the member with the fewest positions first
            may = sorted(([q for q in range(s, e) if fl[j][q]] for j in range(M)), key=len)

            def place(j: int, used: frozenset) -> bool:
                return j == M or any(q not in used and place(j + 1, used | {q}) for q in may[j])
            if may[0] and place(0, frozenset()):
                return True
    return False


def _touched(member, wrong: str) -> bool:
    """Whether the wrong evaluator can differ from the right one on this member."""
    if wrong == "distance":
        return isinstance(member, (Near, NearOf))
    if wrong == "unordered":
        return isinstance(member, (Near, NearOf)) and member.ordered
    if wrong == "cross":
        return isinstance(member, (Phrase, Near, PhraseOf, NearOf))
    if wrong == "somewhere":
        return isinstance(member, NearOf) and not member.ordered
    if wrong == "prefix":
        inner = lambda m: isinstance(m, Prefix) or (isinstance(m, OneOf) and any(isinstance(x, Prefix) for x in m.members))  # noqa: E731
        return inner(member) or (isinstance(member, (PhraseOf, NearOf)) and any(inner(m) for m in member.members))
    return False


class Evaluator:
    """The documents that hold a member, each distinct member evaluated once (a batch repeats members; a Terms is then set
    algebra over these).  wrong: one of WRONG; members the mistake cannot touch are taken from `right`."""

    def __init__(self, words: Sequence[Sequence[str]], wrong: Optional[str] = None, right: "Optional[Evaluator]" = None):
        self.words, self.wrong, self.right = words, wrong, right
        self.n_docs = len(words)
        self.sets = [frozenset(d) for d in words]
        self.tokens = frozenset().union(*self.sets)
        self.kept: Dict[object, np.ndarray] = {}

    def docs(self, member) -> np.ndarray:
        """bool [n_docs]"""
        got = self.kept.get(member)
        if got is not None:
            return got
        if self.right is not None and not _touched(member, self.wrong):
            got = self.right.docs(member)
        else:
            w = None if self.wrong == "none_of" else self.wrong
            if isinstance(member, (str, Prefix, OneOf)):
                f = frozenset(t for t in self.tokens if fills(member, t, w))
                got = np.fromiter((not f.isdisjoint(s) for s in self.sets), dtype=bool, count=self.n_docs)
            else:
                fillers = [frozenset(t for t in self.tokens if fills(s, t, w)) for s in slots_of(member)]
                got = np.zeros(self.n_docs, dtype=bool)
                for d, ws in enumerate(self.words):
                    tail, have = (), self.sets[d]
                    if w == "cross" and d + 1 < self.n_docs:
                        tail, have = self.words[d + 1], have | self.sets[d + 1]
                    if not any(f.isdisjoint(have) for f in fillers):  # (otherwise `holds` says no at once)
                        got[d] = holds(member, ws, tail, w, fillers)
        got.setflags(write=False)
        self.kept[member] = got
        return got

    def rows(self, member) -> np.ndarray:
        return np.flatnonzero(self.docs(member)).astype(np.int64)

    def terms_docs(self, terms: Terms) -> np.ndarray:
        sat = lambda g: np.logical_and.reduce([self.docs(m) for m in g])  # noqa: E731 - a group: every member
        out = np.ones(self.n_docs, dtype=bool)
        for g in terms.all_of or ():
            out &= sat(g)
        if terms.any_of is not None:
            out &= np.logical_or.reduce([sat(g) for g in terms.any_of])
        if self.wrong != "none_of":
            for g in terms.none_of or ():
                out &= ~sat(g)
        return out


def expected_rows(terms: Terms, base_rows=None, ev: Optional[Evaluator] = None) -> np.ndarray:
    """The ascending int64 rows of the constraint (base, terms); base_rows: the ascending rows of its Scope, or None; ev: the
    evaluator of the documents (the base corpus's when not given)."""
    ev = ev or base_evaluator()
    docs = ev.terms_docs(terms)
    if base_rows is not None:
        inside = np.zeros(ev.n_docs, dtype=bool)
        inside[np.asarray(base_rows, dtype=np.int64)] = True
        docs = docs & inside
    return np.flatnonzero(docs).astype(np.int64)


def expected_table(pairs: Sequence[Tuple[Optional[Scope], Terms]], ev: Evaluator, base_rows=None):
    """(scope_ptr i64, rows i64, qscope i32, per constraint its (scope, terms)): equal pairs are ONE constraint, numbered in
    the order they first appear; a Scope that restricts nothing is no Scope."""
    slot: Dict[object, int] = {}
    cons, lists = [], []
    qscope = np.empty(len(pairs), dtype=np.int32)
    for i, (scope, terms) in enumerate(pairs):
        if scope is not None and scope.unrestricted:
            scope = None
        if (scope, terms) not in slot:
            slot[(scope, terms)] = len(cons)
            cons.append((scope, terms))
            lists.append(expected_rows(terms, None if scope is None else base_rows(scope), ev))
        qscope[i] = slot[(scope, terms)]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    return ptr, (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)), qscope, cons


def explain(cons, ev: Evaluator, want_ptr, want_rows, got_ptr, got_rows) -> str:
    """The first constraint whose rows differ: its Terms, the first differing document and that document's words."""
    got_ptr, got_rows = np.asarray(got_ptr, dtype=np.int64), np.asarray(got_rows, dtype=np.int64)
    for c, (scope, terms) in enumerate(cons):
        want = want_rows[want_ptr[c]:want_ptr[c + 1]]
        got = got_rows[got_ptr[c]:got_ptr[c + 1]] if c + 1 < got_ptr.size else got_rows[:0]
        if not np.array_equal(want, got):
            odd = sorted(set(want.tolist()) ^ set(got.tolist()))
            d = odd[0] if odd else -1
            words = " ".join(ev.words[d]) if 0 <= d < ev.n_docs else "(rows repeated, out of order or out of range)"
            return (f"constraint {c}: {terms!r}{'' if scope is None else ' inside a base of %d rows' % len(scope.chunk_ids)}: "
                    f"{want.size} rows expected, {got.size} returned; document {d} is "
                    f"{'missing' if d in set(want.tolist()) else 'extra'}: {words}")
    return "scope_ptr differs" if not np.array_equal(want_ptr, got_ptr) else "equal"


# ---- the generator -------------------------------------------------------------------------------------------------------
KINDS = ("token", "Phrase", "Near", "Prefix", "OneOf", "PhraseOf", "NearOf")
KIND_P = (0.20, 0.13, 0.14, 0.12, 0.11, 0.15, 0.15)


class Grammar:
    """Draws members from the documents `words` (so that spans match somewhere) and from the vocabulary."""

    def __init__(self, words: Sequence[Sequence[str]]):
        self.words = words
        self.long = [d for d, ws in enumerate(words) if len(ws) >= 20]
        self.family = {w: fam for fam in FAMILIES for w in fam}

    def token(self, rng) -> str:
        r = rng.random()
        if r < 0.06:
            return UNKNOWN
        if r < 0.30:
            return VOCAB[int(rng.integers(len(VOCAB)))]
        ws = self.words[self.long[int(rng.integers(len(self.long)))]]
        return ws[int(rng.integers(len(ws)))]  # by frequency

    def window(self, rng, count: int, span: int) -> List[str]:
        """`count` tokens of one document in text order, the last at most `span` positions behind the first."""
        ws = self.words[self.long[int(rng.integers(len(self.long)))]]
        s = int(rng.integers(0, len(ws) - count + 1))
        room = min(span + 1, len(ws) - s)
        at = sorted(rng.choice(room, size=count, replace=False).tolist()) if room >= count else list(range(count))
        return [ws[s + q] for q in at]

    def prefix(self, rng, of: Optional[str] = None) -> Prefix:
        if of is not None and rng.random() < 0.8:  # a stem of the token itself
            return Prefix(of[:int(rng.integers(max(1, len(of) - 3), len(of) + 1))])
        return Prefix(STEMS[int(rng.integers(len(STEMS)))])

    def one_of(self, rng, of: Optional[str] = None) -> OneOf:
        n = int(rng.choice([1, 2, 3, 4], p=[0.15, 0.45, 0.25, 0.15]))
        members = [of] if of is not None else []
        while len(members) < n:
            members.append(self.prefix(rng) if rng.random() < 0.3 else self.token(rng))
        return OneOf(*[members[i] for i in rng.permutation(len(members))])

    def slot(self, rng, token: str, plain: bool):
        """A slot of a PhraseOf / NearOf that `token` fills (mostly)."""
        r = rng.random()
        if plain or r < 0.3:
            return token if r < 0.9 else OneOf(token)  # (a OneOf of one member is that member)
        if r < 0.65:
            return self.prefix(rng, token)
        return self.one_of(rng, token)

    def member(self, rng, kind: Optional[str] = None):
        kind = kind or KINDS[int(rng.choice(len(KINDS), p=KIND_P))]
        if kind == "token":
            return self.token(rng)
        if kind == "Prefix":
            return self.prefix(rng, self.token(rng) if rng.random() < 0.5 else None)
        if kind == "OneOf":
            return self.one_of(rng)
        dist = int(DISTANCES[int(rng.integers(len(DISTANCES)))])
        ordered = bool(rng.random() < 0.5)
        from_text = rng.random() < 0.75
        if kind == "Phrase":
            L = int(rng.choice([1, 2, 3, 4], p=[0.1, 0.55, 0.25, 0.1]))
            return Phrase(*(self.window(rng, L, L - 1) if from_text else [self.token(rng) for _ in range(L)]))
        if kind == "Near":
            M = int(rng.choice([2, 3, 4], p=[0.6, 0.3, 0.1]))
            toks = self.window(rng, M, dist) if from_text else [self.token(rng) for _ in range(M)]
            if rng.random() < 0.25:
                toks[int(rng.integers(1, M))] = toks[0]  # a repeated token: it must stand twice in the window
            if not ordered:
                toks = [toks[i] for i in rng.permutation(M)]
            return Near(*toks, distance=dist, ordered=ordered)
        plain = rng.random() < 0.12  # every slot plain: pack() folds the item into the plain Phrase / Near
        if kind == "PhraseOf":
            L = int(rng.choice([2, 3, 4], p=[0.6, 0.3, 0.1]))
            toks = self.window(rng, L, L - 1) if from_text else [self.token(rng) for _ in range(L)]
            return PhraseOf(*[self.slot(rng, t, plain) for t in toks])
        M = int(rng.choice([2, 3, 4], p=[0.6, 0.3, 0.1]))
        toks = self.window(rng, M, dist) if from_text else [self.token(rng) for _ in range(M)]
        slots = [self.slot(rng, t, plain) for t in toks]
        if rng.random() < 0.3:
            slots[int(rng.integers(1, M))] = slots[0]  # an equal slot: two distinct positions
        if not ordered:
            slots = [slots[i] for i in rng.permutation(M)]
        return NearOf(*slots, distance=dist, ordered=ordered)

    def entry(self, rng):
        if rng.random() < 0.7:
            return self.member(rng)
        return tuple(self.member(rng) for _ in range(int(rng.choice([2, 3], p=[0.7, 0.3]))))

    def terms(self, rng) -> Terms:
        while True:
            given = rng.random(3) < (0.6, 0.4, 0.35)
            if given.any():
                break
        field = lambda on: [self.entry(rng) for _ in range(int(rng.choice([1, 2], p=[0.65, 0.35])))] if on else None  # noqa: E731
        return Terms(all_of=field(given[0]), any_of=field(given[1]), none_of=field(given[2]))


def _grammar() -> Grammar:
    if "grammar" not in _WORLD:
        _WORLD["grammar"] = Grammar(world()[1])
    return _WORLD["grammar"]


def refused(terms: Terms, vocab, df, n_docs: int) -> bool:
    """Whether pack() refuses the expression by ValueError (an unordered NearOf with overlapping, unequal slots)."""
    try:
        pack([(None, terms)], vocab, df, n_docs)
    except ValueError:
        return True
    return False


def overlapping_pair(terms: Terms, tokens) -> bool:
    """Whether some unordered NearOf of `terms` has two slots whose sets of `tokens` (the vocabulary's) intersect without
    being equal — by filling every token into every slot."""
    for _, g in terms.groups():
        for m in g:
            if isinstance(m, NearOf) and not m.ordered:
                sets = [frozenset(t for t in tokens if fills(s, t)) for s in m.members]
                if any(a & b and a != b for i, a in enumerate(sets) for b in sets[:i]):
                    return True
    return False


def random_terms(rng) -> Terms:
    """One expression over the base corpus; may be one that pack() refuses (`random_batch` redraws those)."""
    return _grammar().terms(rng)


def random_batch(seed: int, count: int = 100):
    """(`count` expressions that pack() takes, the ones it refused on the way), seeded."""
    key = ("batch", seed, count)
    if key not in _WORLD:
        _, _, vocab, df = world()
        rng = np.random.default_rng(seed)
        kept, dropped = [], []
        while len(kept) < count:
            t = random_terms(rng)
            (dropped if refused(t, vocab, df, N_DOCS) else kept).append(t)
        _WORLD[key] = (kept, dropped)
    return _WORLD[key]


BATCH_SEEDS = (101, 202, 303)  # one GPU call each; together THE batch of the certificates


def base_evaluator() -> Evaluator:
    if "ev" not in _WORLD:
        _WORLD["ev"] = Evaluator(world()[1])
    return _WORLD["ev"]


def pack_base(pairs, base_rows=None):
    corpus, _, vocab, df = world()
    return pack(pairs, vocab, df, corpus.n_docs, base_rows=base_rows)


# ---- the sixteen step combinations ---------------------------------------------------------------------------------------
STEP_KINDS = ("phrase", "near", "union", "cspan")


def directed_tables():
    """[(name, the subset of STEP_KINDS that pack() must report, [Terms])]: one table per subset — the empty one is plain
    tokens only — plus "a class span whose union nothing else uses" beside the table whose union is also a term of its own.
    A class span WITHOUT a union has the stem no token starts with as its only class: its list is empty.  Tables alternate
    between large (every second one carries ten more members of each of its kinds) and small."""
    g = _grammar()
    rng = np.random.default_rng(16)
    df = world()[3]
    top = sorted(VOCAB, key=lambda w: -df[w])
    a, b, c, rare = top[0], top[1], top[2], top[-1]
    fixed = {"phrase": [Terms(all_of=[Phrase(a, b)]), Terms(all_of=[a], none_of=[Phrase(b, a)])],
             "near": [Terms(all_of=[Near(a, c, distance=5)]), Terms(any_of=[Near(c, c, b, distance=30, ordered=True), rare])],
             "union": [Terms(all_of=[Prefix("sel")]), Terms(all_of=[(OneOf("buyer", rare), a)], none_of=[Prefix("w0")])]}
    with_union = [Terms(all_of=[PhraseOf(Prefix("se"), a)]), Terms(all_of=[b], any_of=[NearOf(OneOf(a, b), Prefix("con"), distance=2)])]
    no_union = [Terms(any_of=[PhraseOf(a, Prefix(NO_STEM)), rare]), Terms(all_of=[a], none_of=[NearOf(Prefix(NO_STEM), b, distance=5)])]
    draw = {"phrase": "Phrase", "near": "Near", "union": "Prefix"}
    out = []
    for mask in range(16):
        subset = tuple(k for i, k in enumerate(STEP_KINDS) if mask >> i & 1)
        terms = [Terms(all_of=[a]), Terms(all_of=[(b, c)], none_of=[rare]), Terms(any_of=[rare, UNKNOWN])]
        for k in subset:
            terms += fixed[k] if k != "cspan" else (with_union if "union" in subset else no_union)
        if mask & 1 == 0:  # a large table
            for k in subset:
                if k in draw:
                    terms += [Terms(all_of=[m]) for m in _distinct(g, rng, draw[k], 10, k)]
        out.append(("+".join(subset) or "plain", subset, terms))
    out.append(("cspan whose union nothing else uses", ("union", "cspan"), [Terms(all_of=[a])] + with_union))
    order = sorted(range(len(out)), key=lambda i: len(out[i][2]))
    mixed = [order[i // 2] if i % 2 else order[-1 - i // 2] for i in range(len(order))]  # largest, smallest, 2nd largest ...
    return [out[i] for i in mixed]


def _distinct(g: Grammar, rng, kind: str, count: int, step: str):
    """`count` members of `kind` that stay in their step: a Phrase of two tokens or more, a Prefix of two tokens or more."""
    got = []
    while len(got) < count:
        m = g.member(rng, kind)
        if step == "phrase" and len(m) < 2:
            continue
        if step == "union" and sum(w.startswith(m.stem) for w in VOCAB) < 2:
            continue
        got.append(m)
    return got


def steps_of(tt) -> tuple:
    return tuple(k for k, n in zip(STEP_KINDS, (tt.n_phr, tt.n_near, tt.n_union, tt.n_cspan)) if n)


# ---- base scopes ---------------------------------------------------------------------------------------------------------
BASE_SIZES = (0, 1, TILE - 1, TILE, TILE + 1, N_DOCS)


def base_scopes():
    """One Scope per size of BASE_SIZES: a random ascending subset of the documents, as chunk ids."""
    rng = np.random.default_rng(77)
    return [Scope(chunk_ids=frozenset(int(x) for x in rng.choice(N_DOCS, size=m, replace=False))) for m in BASE_SIZES]


def rows_of_scope(scope: Scope) -> np.ndarray:
    return np.asarray(sorted(int(x) for x in scope.chunk_ids), dtype=np.int64)  # (a Scope keeps its ids as str)


def scoped_pairs():
    """(Scope, Terms) pairs: every base with Terms that have no MUST term (the base drives) and with Terms whose MUST list
    is shorter than the base (the list drives); the Terms come from the first batch, so equal scopes are shared."""
    ev = base_evaluator()
    batch = random_batch(BATCH_SEEDS[0])[0]
    no_must = [t for t in batch if t.all_of is None][:6]
    must = sorted((t for t in batch if t.all_of is not None and 0 < int(ev.terms_docs(Terms(all_of=t.all_of)).sum())),
                  key=lambda t: int(ev.terms_docs(Terms(all_of=t.all_of)).sum()))
    pairs = []
    for scope in base_scopes():
        pairs += [(scope, t) for t in no_must]
        pairs += [(scope, t) for t in must[:4] + must[-4:]]
    return pairs


def scoped_certificates() -> None:
    ev = base_evaluator()
    pairs = scoped_pairs()
    tt = pack_base(pairs, rows_of_scope)
    assert tt.n_base == len(BASE_SIZES)  # equal scopes are stored once; the one of no rows restricts too
    base_drives = list_drives = 0
    for scope, t in pairs:
        m = len(scope.chunk_ids)
        if t.all_of is None:
            base_drives += 1
        elif 0 < int(ev.terms_docs(Terms(all_of=t.all_of)).sum()) < m:
            list_drives += 1
    assert base_drives >= 30 and list_drives >= 8


# ---- the live index ------------------------------------------------------------------------------------------------------
def edit_rounds(words: Sequence[Sequence[str]]):
    """Three edits of the corpus `words`, each computed from the corpus the one before leaves:
      ("add", documents)            documents of every length that bring NEW_TOKENS into the stem families;
      ("remove", ids)               document 0 (the vocabulary's first-seen order moves), the last one, the document that
                                    holds the commonest token most often, every document that holds "selx" (the token
                                    leaves the vocabulary) and a random tenth;
      ("replace", ids, documents)   documents 0 and n - 1 among them; an empty and a 300-token document among the new ones,
                                    and "sellable" once more.
    Returns [(op, the corpus after it)]."""
    rng = np.random.default_rng(5)
    pool = list(VOCAB) + list(NEW_TOKENS)
    p = np.asarray([1.0] * len(VOCAB) + [4.0] * len(NEW_TOKENS))
    p /= p.sum()
    draw = lambda n: [pool[i] for i in rng.choice(len(pool), size=int(n), p=p)]  # noqa: E731
    out, cur = [], [list(d) for d in words]
    added = [draw(n) for n in list(LENGTHS) * 4]
    cur = cur + added
    out.append((("add", added), cur))
    counts: Dict[str, int] = {}
    for d in cur:
        for w in set(d):
            counts[w] = counts.get(w, 0) + 1
    commonest = max(counts, key=counts.get)
    ids = {0, len(cur) - 1, max(range(len(cur)), key=lambda d: cur[d].count(commonest))}
    ids |= {d for d, ws in enumerate(cur) if "selx" in ws}
    ids |= {int(x) for x in rng.choice(len(cur), size=len(cur) // 10, replace=False)}
    ids = sorted(ids)
    gone = set(ids)
    cur = [d for i, d in enumerate(cur) if i not in gone]
    out.append((("remove", ids), cur))
    ids = sorted({0, len(cur) - 1} | {int(x) for x in rng.choice(len(cur), size=30, replace=False)})
    docs = [draw(LENGTHS[i % len(LENGTHS)]) for i in range(len(ids))]
    docs[1] = docs[1] + ["sellable", "w99"]
    cur = list(cur)
    for i, d in zip(ids, docs):
        cur[i] = d
    out.append((("replace", ids, docs), cur))
    return out


def live_terms() -> List[Terms]:
    """The expressions of the live-index test: half a batch, so that a round's reference stays within a second or two."""
    return random_batch(BATCH_SEEDS[0])[0][:50]


def apply_edit(model, op, carry: bool = True) -> None:
    """The edit on a BM25Okapi (and on its resident index, if it has one)."""
    if op[0] == "add":
        model.add_documents(op[1], carry_tokens=carry)
    elif op[0] == "remove":
        model.remove_documents(op[1], carry_tokens=carry)
    else:
        model.replace_documents(op[1], op[2], carry_tokens=carry)


def edit_certificates(rounds) -> None:
    base = world()[1]
    (add, after_add), (rem, after_rem), (rep, after_rep) = rounds
    have = lambda docs: set().union(*map(set, docs))  # noqa: E731
    assert [r[0][0] for r in rounds] == ["add", "remove", "replace"]
    assert set(NEW_TOKENS) <= have(after_add) - have(base)              # Prefix("sell") names more tokens than before
    assert "selx" in have(after_add) and "selx" not in have(after_rem)  # ... and Prefix("sel") one fewer
    assert 0 in rem[1] and len(after_add) - 1 in rem[1] and len(after_rem) == len(after_add) - len(rem[1])
    df = {w: sum(w in d for d in map(set, after_add)) for w in have(after_add)}
    commonest = max(df, key=df.get)
    assert max(d.count(commonest) for d in after_add) == max(after_add[i].count(commonest) for i in rem[1]) > 20
    assert after_rem[0] != after_add[0] and 0 in rep[1] and len(after_rep) - 1 in rep[1]
    assert {len(d) for d in add[1]} == set(LENGTHS) and {0, 300} <= {len(d) for d in rep[2]}


# ---- shrinking a mismatch ------------------------------------------------------------------------------------------------
def _smaller_member(m):
    """Members with one token, slot or alternative fewer."""
    if isinstance(m, Phrase) and len(m) > 1:
        return [Phrase(*(m.tokens[:i] + m.tokens[i + 1:])) for i in range(len(m))]
    if isinstance(m, OneOf) and len(m) > 1:
        return [OneOf(*(m.members[:i] + m.members[i + 1:])) for i in range(len(m))]
    if isinstance(m, Near) and len(m) > 2:
        return [Near(*(m.tokens[:i] + m.tokens[i + 1:]), distance=m.distance, ordered=m.ordered) for i in range(len(m))]
    if isinstance(m, PhraseOf) and len(m) > 2:
        return [PhraseOf(*(m.members[:i] + m.members[i + 1:])) for i in range(len(m))]
    if isinstance(m, NearOf) and len(m) > 2:
        return [NearOf(*(m.members[:i] + m.members[i + 1:]), distance=m.distance, ordered=m.ordered) for i in range(len(m))]
    return []


def smaller(terms: Terms) -> List[Terms]:
    """Every Terms one step smaller: a field, an entry, a member of a group, or a part of a member dropped."""
    fields = {"all_of": terms.all_of, "any_of": terms.any_of, "none_of": terms.none_of}
    out = []
    for name, groups in fields.items():
        if groups is None:
            continue
        put = lambda new: out.append(Terms(**{**fields, name: new}))  # noqa: E731
        put(None)
        for i, g in enumerate(groups):
            if len(groups) > 1:
                put(groups[:i] + groups[i + 1:])
            for j, m in enumerate(g):
                if len(g) > 1:
                    put(groups[:i] + (g[:j] + g[j + 1:],) + groups[i + 1:])
                for m2 in _smaller_member(m):
                    put(groups[:i] + (g[:j] + (m2,) + g[j + 1:],) + groups[i + 1:])
    return [t for t in out if not t.unrestricted]


def shrink(terms: Terms, fails) -> Terms:
    """The smallest Terms reached from `terms` by `smaller` steps on which `fails(Terms) -> bool` still holds (greedy)."""
    while True:
        for t in smaller(terms):
            if fails(t):
                terms = t
                break
        else:
            return terms

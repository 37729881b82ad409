"""amdr_vocab_match on the GPU, both forms, byte for byte against the plain evaluator of tests/vocab_match_cases.py: the
vocabulary sizes around the tile with matches at the ids 0, T - 1, T and n - 1, pattern lengths 1, 63 and 64, token lengths
around a pattern's, every kind of edit at the first, a middle and the last position, the Wildcard forms, code points of 2, 3
and 4 bytes, 1 / 2 / 65 / 70 000 patterns, truncation at item_cap, garbage patterns in the device form, every refusal (after
which outputs and workspace are untouched), the call captured in a graph and replayed over rewritten patterns, and two
handles of different vocabularies in one process."""
import ctypes as C

import numpy as np
import pytest

import vocab_match_cases as VC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0x5a


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    assert _native.VOCAB_TILE_TERMS == VC.T
    return _native


def dev_arr(a, dtype, room=0):
    t = torch.zeros(max(int(np.size(a)), room, 1), dtype=dtype, device=DEV)
    if np.size(a):
        t[:np.size(a)].copy_(torch.from_numpy(np.ascontiguousarray(a).ravel().view(np.int32 if a.dtype == np.uint32 else a.dtype)))
    return t


class DeviceCall:
    """The operands of one amdr_vocab_match_device call on the device and its outputs and workspace, filled with SENT."""

    def __init__(self, nat, index, ops, cap, cp_room=0, n_room=0):
        self.nat, self.index, self.cap = nat, index, int(cap)
        cp, ptr, kind, arg = ops
        self.n = max(int(ptr.size) - 1, n_room)
        self.cp_total = max(int(cp.size), cp_room)
        self.cp = dev_arr(cp, torch.int32, cp_room)
        self.ptr = dev_arr(ptr, torch.int64, n_room + 1)
        self.kind, self.arg = dev_arr(kind, torch.int32, n_room), dev_arr(arg, torch.int32, n_room)
        rows = max(self.n * self.cap, 1)
        self.ids = torch.full((rows,), -0x5a5a5a5b, dtype=torch.int32, device=DEV)
        self.dist = torch.full((rows,), SENT, dtype=torch.uint8, device=DEV)
        self.n_match = torch.full((max(self.n, 1),), -77, dtype=torch.int64, device=DEV)
        self.work_bytes = nat.vocab_match_plan(index.n_terms, self.n)
        self.work = torch.full((self.work_bytes + 8,), SENT, dtype=torch.uint8, device=DEV)  # (dirty: nothing needs clearing)

    def write(self, ops):
        for t, a in zip((self.cp, self.ptr, self.kind, self.arg), ops):
            t[:a.size].copy_(torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a))

    def __call__(self):
        self.index.match_device(self.cp.data_ptr(), self.ptr.data_ptr(), self.kind.data_ptr(), self.arg.data_ptr(), self.n,
                                self.cp_total, self.cap, self.ids.data_ptr(), self.dist.data_ptr(), self.n_match.data_ptr(),
                                self.work.data_ptr(), self.work_bytes, torch.cuda.current_stream().cuda_stream)

    def fetch(self):
        torch.cuda.synchronize()
        n, cap = self.n, self.cap
        return (self.ids[:n * cap].cpu().numpy().reshape(n, cap), self.dist[:n * cap].cpu().numpy().reshape(n, cap),
                self.n_match[:n].cpu().numpy())

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.ids == -0x5a5a5a5b).all() and (self.dist == SENT).all() and (self.n_match == -77).all()
                    and (self.work == SENT).all())


def assert_equal(got, want, what):
    for name, g, w in zip(("ids", "dist", "n_match"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, g[:3], w[:3])


def both_forms(nat, vocab, patterns, cap, what, want=None):
    """The twin and the device form of one call against the evaluator; returns what the evaluator gave."""
    index = nat.VocabIndex(vocab, device=0)
    assert index.info() == (len(vocab), sum(len(t.encode()) for t in vocab))
    ops = VC.pack(patterns)
    want = VC.evaluate(vocab, patterns, cap) if want is None else want
    assert_equal(index.match(*ops, cap), want, (what, "twin"))
    call = DeviceCall(nat, index, ops, cap)
    call()
    assert_equal(call.fetch(), want, (what, "device"))
    return want


SIZE_PATTERNS = [("f", "zebra", 1), ("w", "z?b*"), ("f", "zbera", 1), ("f", "zebra", 2), ("w", "*ra"), ("f", "qqqqq", 2)]


@pytest.mark.parametrize("n", VC.SIZES)
def test_vocabulary_sizes_around_the_tile_with_matches_at_its_edges(nat, n):
    vocab, at = VC.sized_vocab(n)
    want = both_forms(nat, vocab, SIZE_PATTERNS, 8, n)
    # the certificate: the probe itself stands at the ids 0, T - 1, T and n - 1 that exist, a transposition beside each
    assert [int(i) for i, d in zip(want[0][0], want[1][0]) if d == 0] == at and want[2][5] == 0
    assert want[2][0] == len([t for t in vocab if t in ("zebra", "zebar")]) <= 8 and want[2][2] == len(at) == want[2][4]
    assert want[2][3] == want[2][0] and set(at) <= set(want[0][3].tolist()) and want[2][1] == want[2][0]


def test_pattern_lengths_token_lengths_and_every_kind_of_edit(nat):
    VC.edit_cases()
    edits = VC.edit_cases()
    vocab = [t for _, t, _ in edits] + VC.filler(40, seed=5)
    want = both_forms(nat, vocab, [("f", VC.WORD, 1), ("f", VC.WORD, 2)], 32, "edits")
    for p, e in ((0, 1), (1, 2)):
        hit = {int(i): int(d) for i, d in zip(want[0][p], want[1][p]) if i >= 0}
        assert hit == {i: d for i, (_, _, d) in enumerate(edits) if d <= e}  # distance exactly e is in, e + 1 is out
    pat, toks = VC.length_cases(6, 2)
    want = both_forms(nat, toks, [("f", pat, 2), ("f", pat, 1), ("w", "a*"), ("w", "aaaaa?"), ("w", "a?*")], 8, "token lengths")
    assert want[0][0].tolist()[:3] == [3, 4, 5] and want[2].tolist() == [3, 1, 7, 1, 6]
    a63, a64 = "a" * 62 + "b", "a" * 63 + "b"
    vocab = ["a", "b", a63, a64, a64 + "c", "a" * 64, "a" * 66, "c" * 63 + "b", "ab"]
    pats = [("f", "ab", 1), ("f", a63, 1), ("f", a64, 1), ("f", a64, 2), ("w", "a" * 63 + "?"), ("w", "a" * 62 + "*b"), ("w", "?" * 63 + "b"),
            ("w", "a*")]
    for p in pats:
        assert len(p[1]) in (2, 63, 64)
    want = both_forms(nat, vocab, pats, 8, "pattern lengths")
    assert want[2].tolist() == [3, 2, 4, 4, 2, 2, 2, 7]
    # a pattern of one code point: the twin takes it as the rule defines it (the classes of retrieval/terms.py ask for more)
    want = both_forms(nat, ["a", "b", "ab", "ba", "abc", ""], [("f", "a", 1), ("w", "a")], 8, "one code point")
    assert want[2].tolist() == [4, 1]


def test_wildcard_forms(nat):
    VC.wild_certificates()
    pats = [("w", p) for p in VC.WILD_PATTERNS]
    want = both_forms(nat, VC.WILD_VOCAB, pats, 32, "wildcards")
    names = {p: [VC.WILD_VOCAB[i] for i in row if i >= 0] for p, row in zip(VC.WILD_PATTERNS, want[0])}
    assert names["a*a"] == ["aa", "aba"] and names["*ab*ab?"] == ["ababc", "abxababc", "xabyabz"] and names["**ee"] == names["*ee"]
    assert names["wom?n"] == ["wom\U00020000n", "woman", "women"] and names["a?"] == ["aa", "ab", "a?"] and names["in*ment"] == ["in\nment", "inment"]


def test_code_points_not_bytes(nat):
    VC.unicode_certificates()
    want = both_forms(nat, VC.UNI_VOCAB, VC.UNI_PATTERNS, 16, "unicode")
    named = lambda p: {VC.UNI_VOCAB[i]: int(d) for i, d in zip(want[0][p], want[1][p]) if i >= 0}  # noqa: E731
    assert named(0) == {"中文": 0, "国文": 1, "中": 1} and named(1) == {"cafe": 0, "café": 1, "caf": 1}
    assert named(3) == {"a\U00020000c": 0, "abc": 0, "a中c": 0} and named(6) == {"é": 1}
    assert named(4) == {"\U00020000\U00020001": 0}


@pytest.mark.parametrize("n_pat", (1, 2, 65, 70_000))
def test_pattern_counts_up_to_a_grid_of_70_000_blocks(nat, n_pat):
    vocab, _ = VC.sized_vocab(64)
    vocab[10:14] = ["zebras", "ezbra", "cobra", "zeb"]
    distinct = [("f", "zebra", 1), ("w", "*bra*"), ("f", "cobra", 2), ("w", "z??"), ("f", "zeb", 1), ("w", "?e*"), ("f", "xyzzy", 1)]
    ids, dist, n_match = VC.evaluate(vocab, distinct, 4)
    pick = [(p * 5) % len(distinct) for p in range(n_pat)]
    want = (ids[pick], dist[pick], n_match[pick])
    both_forms(nat, vocab, [distinct[j] for j in pick], 4, n_pat, want)
    assert n_match.max() > 4 > n_match.min()  # (some rows are truncated, some padded)


@pytest.mark.parametrize("extra", (-1, 0, 1))
def test_truncation_keeps_the_true_count_the_first_ids_and_the_padding(nat, extra):
    cap = 4
    vocab = VC.cap_vocab(cap + extra)
    want = both_forms(nat, vocab, [("w", "quo*"), ("f", "quorum", 1), ("f", "nothing", 1)], cap, ("cap", extra))
    assert want[2].tolist() == [cap + extra, cap + extra, 0]
    kept = min(cap, cap + extra)
    assert (np.diff(want[0][0][:kept]) > 0).all() and (want[0][0][kept:] == -1).all() and (want[1][1][kept:] == 255).all()
    assert want[0][0][:kept].max() >= VC.T or extra < 0  # (the matches cross the tile edge)


def test_garbage_patterns_match_nothing_and_touch_nothing_else(nat):
    vocab = ["abc", "abd", "ab", "a?c", "xbc"] + VC.filler(VC.T + 3, seed=9)
    index = nat.VocabIndex(vocab, device=0)
    cp, ptr, kind, arg, valid = VC.garbage_patterns()
    cap = 4
    guard = 64
    call = DeviceCall(nat, index, (cp, ptr, kind, arg), cap)
    ids_all = torch.full((call.n * cap + 2 * guard,), 0x1234567, dtype=torch.int32, device=DEV)
    call.ids = ids_all[guard:guard + call.n * cap]
    call()
    ids, dist, n_match = call.fetch()
    want = VC.evaluate(vocab, [("f", "abc", 1)], cap)
    for p in range(call.n):
        if p in valid:
            assert (ids[p].tolist(), dist[p].tolist(), int(n_match[p])) == (want[0][0].tolist(), want[1][0].tolist(), int(want[2][0]))
            assert n_match[p] == 5 > cap
        else:
            assert n_match[p] == 0 and (ids[p] == -1).all() and (dist[p] == 255).all(), p
    assert (ids_all[:guard] == 0x1234567).all() and (ids_all[-guard:] == 0x1234567).all()
    # spans that are negative, reversed, too long or beyond cp_total
    four = (np.asarray([ord(c) for c in "abc"] * 30, np.uint32), VC.garbage_spans(90), np.ones(4, np.int32), np.ones(4, np.int32))
    call = DeviceCall(nat, index, four, cap)
    call()
    ids, dist, n_match = call.fetch()
    assert (n_match == 0).all() and (ids == -1).all() and (dist == 255).all()
    # the twin refuses each of them
    for p in range(len(kind)):
        if p not in valid:
            with pytest.raises(nat.NativeError):
                index.match(cp[ptr[p]:ptr[p + 1]], [0, ptr[p + 1] - ptr[p]], kind[p:p + 1], arg[p:p + 1], cap)
    with pytest.raises(nat.NativeError, match="pat_ptr"):
        index.match(four[0], four[1], four[2], four[3], cap)
    with pytest.raises(nat.NativeError, match="pat_ptr"):
        index.match(four[0], [0, 3, 6], [1, 1], [1, 1], cap)  # (pat_ptr does not end at cp_total)


def test_argument_errors_enqueue_nothing_and_leave_outputs_and_workspace_untouched(nat):
    vocab, _ = VC.sized_vocab(2 * VC.T)
    index = nat.VocabIndex(vocab, device=0)
    pats = [("f", "zebra", 1), ("w", "z*")]
    call = DeviceCall(nat, index, VC.pack(pats), 8)
    lib = nat.load()
    vp = lambda x: C.c_void_p(int(x) if x else 0)  # noqa: E731

    def raw(**over):
        a = dict(h=index._h, cp=call.cp.data_ptr(), ptr=call.ptr.data_ptr(), kind=call.kind.data_ptr(), arg=call.arg.data_ptr(),
                 n=call.n, cp_total=call.cp_total, cap=call.cap, ids=call.ids.data_ptr(), dist=call.dist.data_ptr(),
                 n_match=call.n_match.data_ptr(), work=call.work.data_ptr(), work_bytes=call.work_bytes)
        a.update(over)
        return lib.amdr_vocab_match_device(a["h"], vp(a["cp"]), vp(a["ptr"]), vp(a["kind"]), vp(a["arg"]), C.c_int64(a["n"]),
                                           C.c_int64(a["cp_total"]), C.c_int32(a["cap"]), vp(a["ids"]), vp(a["dist"]),
                                           vp(a["n_match"]), vp(a["work"]), C.c_int64(a["work_bytes"]),
                                           vp(torch.cuda.current_stream().cuda_stream))
    bad = [dict(h=None), dict(cp=0), dict(ptr=0), dict(kind=0), dict(arg=0), dict(ids=0), dict(dist=0), dict(n_match=0), dict(work=0),
           dict(n=-1), dict(cp_total=-1), dict(cap=0), dict(cap=-1), dict(cap=VC.MAX_CAP + 1), dict(work_bytes=-1), dict(work_bytes=0),
           dict(work_bytes=call.work_bytes - 1), dict(n=2 ** 24), dict(n=(2 ** 24 - 1) // 2 + 1)]
    for over in bad:
        assert raw(**over) == -1, over  # AMDR_EINVAL
        assert lib.amdr_last_error(), over
    assert call.untouched()
    assert raw() == 0  # the same arguments, unchanged, are a valid call
    assert_equal(call.fetch(), VC.evaluate(vocab, pats, 8), "after the refusals")
    # the twin: the sizes; create: offsets and UTF-8
    ops = VC.pack(pats)
    for cap in (0, VC.MAX_CAP + 1):
        with pytest.raises(nat.NativeError, match="item_cap"):
            index.match(*ops, cap)
    h = C.c_void_p()
    blob = "中a".encode()
    for offs in ([0, 1, 4], [1, 4], [0, 4, 3]):
        o = np.asarray(offs, np.int64)
        rc = lib.amdr_vocab_create(C.c_char_p(blob), o.ctypes.data_as(C.c_void_p), C.c_int64(o.size - 1), C.c_int32(0), C.byref(h))
        assert rc == -1 and not h.value, offs
    assert lib.amdr_vocab_create(C.c_char_p(b"\xc0\x80"), np.asarray([0, 2], np.int64).ctypes.data_as(C.c_void_p), C.c_int64(1), C.c_int32(0),
                                 C.byref(h)) == -1
    empty = nat.VocabIndex([], device=0)
    assert empty.info() == (0, 0) and empty.match(*VC.pack([("f", "abc", 1)]), 3)[2].tolist() == [0]
    assert index.match(*VC.pack([]), 3)[2].size == 0


def test_a_captured_call_replays_over_rewritten_patterns(nat):
    """One linear graph: the call's three launches.  Between the replays the patterns are rewritten in place (fewer code
    points than the arrays hold: the tail of pat_ptr repeats cp_total, empty patterns that name nothing)."""
    vocab, _ = VC.sized_vocab(VC.T + 9)
    vocab[20:24] = ["zebras", "cobra", "zeal", "zebu"]
    index = nat.VocabIndex(vocab, device=0)
    n_room, cp_room, cap = 4, 40, 6
    variants = [[("f", "zebra", 1), ("w", "z*"), ("f", "cobra", 2), ("w", "?e??")],
                [("w", "*bra"), ("f", "zeal", 1), ("w", "ze*"), ("f", "zebus", 2)],
                [("f", "zebu", 2), ("w", "co?ra")]]

    def ops_of(pats):
        cp, ptr, kind, arg = VC.pack(pats)
        full = lambda a, n, v: np.concatenate([a, np.full(n - a.size, v, a.dtype)])  # noqa: E731
        return (full(cp, cp_room, 0), full(ptr, n_room + 1, cp_room), full(kind, n_room, 7), full(arg, n_room, 0))

    def want_of(pats):
        ids, dist, n_match = VC.evaluate(vocab, pats, cap)
        k = n_room - len(pats)
        return (np.concatenate([ids, np.full((k, cap), -1, np.int32)]), np.concatenate([dist, np.full((k, cap), 255, np.uint8)]),
                np.concatenate([n_match, np.zeros(k, np.int64)]))
    call = DeviceCall(nat, index, ops_of(variants[0]), cap)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):  # an eager run first, outside the capture
        call()
    side.synchronize()
    assert_equal(call.fetch(), want_of(variants[0]), "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    g0 = nat.workspace_growths()
    for i in (1, 2):
        call.write(ops_of(variants[i]))
        graph.replay()
        got = call.fetch()
        assert nat.workspace_growths() == g0
        assert_equal(got, want_of(variants[i]), f"replay {i}")
        assert want_of(variants[i])[2].sum() > 0


def test_two_handles_of_different_vocabularies_in_one_process(nat):
    a, b = nat.VocabIndex(["seller", "sells", "buyer"], device=0), nat.VocabIndex(["buyer", "sell", "lessee", "seller"], device=0)
    ops = VC.pack([("f", "sell", 2), ("w", "*er")])
    for _ in range(2):
        assert a.match(*ops, 4)[0].tolist() == [[0, 1, -1, -1], [0, 2, -1, -1]]
        assert b.match(*ops, 4)[0].tolist() == [[1, 3, -1, -1], [0, 3, -1, -1]]
    a.close()
    assert b.match(*ops, 4)[2].tolist() == [2, 2]

"""The empty "_device" call of the list resolvers (csrc/list_step.hpp: the launch sequence's shortcut), the one behaviour of
their shared frame that the resolvers' own tests do not reach.  With no item a call enqueues no kernel: one that starts an
array (n_before = 0) writes list_ptr[0] = 0 and nothing else; one that continues an array (n_before > 0: the union step
and the class step) changes no byte of list_ptr, the documents or the status words.  Outputs and workspaces are filled
with a sentinel first, so a stray write shows."""
import numpy as np
import pytest
import torch

import phrase_cases as PC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = -77
WORK_BYTE = 0xB3
ROOM = 64  # elements of every output, bytes of every workspace: far more than an empty call may touch


@pytest.fixture(scope="module")
def index():
    from legal_rag_amd import _native
    _native.load()
    assert _native.device_count() >= 1, "no GPU visible"
    assert _native.device_name(0).startswith("gfx950"), _native.device_name(0)
    corpus, _ = PC.edge_corpus()
    tp, pd, pt, idf, dl, avgdl = corpus.postings()
    gi = _native.BM25Index(tp, pd, pt, idf, dl, avgdl)
    gi.set_tokens(*corpus.stream())
    return _native, corpus, gi


class Outputs:
    """list_ptr i64, rows (i32 documents or i64 scope rows), status i32 and a workspace, all sentinel."""

    def __init__(self, rows_dtype=torch.int32):
        self.list_ptr = torch.full((ROOM,), SENTINEL, dtype=torch.int64, device=DEV)
        self.rows = torch.full((ROOM,), SENTINEL, dtype=rows_dtype, device=DEV)
        self.status = torch.full((ROOM,), SENTINEL, dtype=torch.int32, device=DEV)
        self.work = torch.full((ROOM,), WORK_BYTE, dtype=torch.uint8, device=DEV)

    def host(self):
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy().copy() for t in (self.list_ptr, self.rows, self.status, self.work))


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def dummy(dtype):
    return torch.full((4,), SENTINEL, dtype=dtype, device=DEV)


def empty_calls(gi):
    """name -> (rows dtype, call(outputs)): each "_device" entry with no item, starting an array."""
    i64, i32 = dummy(torch.int64), dummy(torch.int32)
    a, b = i64.data_ptr(), i32.data_ptr()

    def tail(o):
        return o.list_ptr.data_ptr(), o.rows.data_ptr(), o.status.data_ptr(), o.work.data_ptr(), ROOM, stream_ptr()

    return (i64, i32), {
        "term_scope_device": (torch.int64, lambda o: gi.term_scope_device([a, b, a, b, a, a, b], 0, 0, 0, 0, ROOM, *tail(o))),
        "phrase_lists_device": (torch.int32, lambda o: gi.phrase_lists_device(a, b, 0, 0, ROOM, *tail(o))),
        "span_lists_device": (torch.int32, lambda o: gi.span_lists_device(a, b, b, b, 0, 0, ROOM, *tail(o))),
        "union_lists_device": (torch.int32, lambda o: gi.union_lists_device(a, b, 0, 0, ROOM, *tail(o))),
        "class_spans_device": (torch.int32, lambda o: gi.class_spans_device(a, b, b, b, 0, a, b, 0, 0, 0, 0, ROOM, *tail(o))),
    }


@pytest.mark.parametrize("name", ["term_scope_device", "phrase_lists_device", "span_lists_device", "union_lists_device",
                                  "class_spans_device"])
def test_empty_call_starts_an_empty_array(index, name):
    _, _, gi = index
    held, calls = empty_calls(gi)
    rows_dtype, call = calls[name]
    o = Outputs(rows_dtype)
    call(o)
    list_ptr, rows, status, work = o.host()
    assert list_ptr[0] == 0 and np.all(list_ptr[1:] == SENTINEL), list_ptr
    assert np.all(rows == SENTINEL) and np.all(status == SENTINEL) and np.all(work == WORK_BYTE)
    assert all(np.all(t.cpu().numpy() == SENTINEL) for t in held)  # (the operands are not written either)


def test_empty_call_behind_two_lists_changes_nothing(index):
    nat, corpus, gi = index
    phrases = [PC.AB, PC.ABC]
    p_ptr, p_terms = PC.operands(phrases)
    want_ptr, want_docs = PC.expected_lists(corpus, phrases)
    assert want_ptr[-1] > 0 and want_ptr[-1] <= ROOM  # two non-empty lists that fit
    cand_max = max(PC.driver_len(corpus, p) for p in phrases)
    ops = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in
           (p_ptr.astype(np.int64), p_terms.astype(np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32))]
    o = Outputs()
    s_bytes = nat.span_lists_plan(2, cand_max)
    s_work = torch.empty(max(s_bytes, 1), dtype=torch.uint8, device=DEV)
    gi.span_lists_device(*[t.data_ptr() for t in ops], 2, cand_max, ROOM, o.list_ptr.data_ptr(), o.rows.data_ptr(),
                         o.status.data_ptr(), s_work.data_ptr(), s_bytes, stream_ptr())
    before = o.host()
    assert np.array_equal(before[0][:3], want_ptr) and np.array_equal(before[1][:want_ptr[-1]], want_docs)
    assert not before[2][:2].any() and np.all(before[0][3:] == SENTINEL)
    i64, i32 = dummy(torch.int64), dummy(torch.int32)
    a, b = i64.data_ptr(), i32.data_ptr()
    tail = (o.list_ptr.data_ptr(), o.rows.data_ptr(), o.status.data_ptr() + 4 * 2, o.work.data_ptr(), ROOM, stream_ptr())
    for call in (lambda: gi.union_lists_device(a, b, 0, 2, ROOM, *tail),
                 lambda: gi.class_spans_device(a, b, b, b, 0, a, b, 0, 0, 2, 0, ROOM, *tail)):
        call()
        after = o.host()
        for x, y in zip(before, after):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))

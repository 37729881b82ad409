"""The carrying updates without a GPU: the new entry points are exported and refuse a null handle before they touch a
device, and cfg.retrieval.token_stream is validated like query_tokenizer."""
import ctypes as C

import pytest

NAMES = ("amdr_bm25_add_carry", "amdr_bm25_remove_carry", "amdr_bm25_replace_carry", "amdr_bm25_carry_kernel_ms")


def test_exports_hold_the_four_names_after_their_plain_counterparts():
    from legal_rag_amd import _native
    for name in NAMES:
        assert name in _native.EXPORTS, name
    s = _native.SIGNATURES
    # the plain call's arguments in the plain call's order, then the token arguments
    assert s["amdr_bm25_add_carry"] == s["amdr_bm25_add"] + "PP"
    assert s["amdr_bm25_remove_carry"] == s["amdr_bm25_remove"]
    assert s["amdr_bm25_replace_carry"] == s["amdr_bm25_replace"] + "PP"
    assert s["amdr_bm25_carry_kernel_ms"] == "PP"


def test_the_new_calls_refuse_a_null_handle():
    from legal_rag_amd import _native
    lib = _native.load()
    one64, one32, oned = (C.c_int64 * 2)(0, 0), (C.c_int32 * 2)(0, 0), (C.c_double * 2)(1.0, 1.0)
    p64, p32, pd = C.cast(one64, C.POINTER(C.c_int64)), C.cast(one32, C.POINTER(C.c_int32)), C.cast(oned, C.POINTER(C.c_double))
    rc = lib.amdr_bm25_add_carry(None, p64, p32, p32, pd, p32, C.c_int64(1), C.c_int64(1), C.c_double(1.0), p64, p32)
    assert rc == -1 and b"null handle" in lib.amdr_last_error()
    rc = lib.amdr_bm25_remove_carry(None, p64, C.c_int64(1), None, C.c_int64(1), pd, C.c_double(1.0))
    assert rc == -1 and b"null handle" in lib.amdr_last_error()
    rc = lib.amdr_bm25_replace_carry(None, p64, C.c_int64(1), p64, p32, p32, p32, None, C.c_int64(1), pd, C.c_double(1.0), p64, p32)
    assert rc == -1 and b"null handle" in lib.amdr_last_error()
    ms = C.c_double(0.0)
    assert lib.amdr_bm25_carry_kernel_ms(None, C.byref(ms)) == -1
    assert lib.amdr_bm25_carry_kernel_ms(None, None) == -1


def test_token_stream_mode_default_values_and_refusal():
    from types import SimpleNamespace

    from legal_rag_amd.config import TOKEN_STREAMS, RetrievalConfig, token_stream_mode
    assert TOKEN_STREAMS == ("rebuild", "carry")
    assert RetrievalConfig().token_stream == "rebuild" and token_stream_mode(RetrievalConfig()) == "rebuild"
    assert token_stream_mode(SimpleNamespace()) == "rebuild"                      # a duck-typed config without the field
    assert token_stream_mode(SimpleNamespace(retrieval=SimpleNamespace(token_stream=None))) == "rebuild"
    for value in TOKEN_STREAMS:
        assert token_stream_mode(RetrievalConfig(token_stream=value)) == value
        assert token_stream_mode(SimpleNamespace(retrieval=SimpleNamespace(token_stream=value))) == value
    for bad in ("Carry", "keep", "", 1):
        with pytest.raises(ValueError, match="retrieval.token_stream"):
            RetrievalConfig(token_stream=bad)
        with pytest.raises(ValueError, match="retrieval.token_stream"):
            token_stream_mode(SimpleNamespace(retrieval=SimpleNamespace(token_stream=bad)))

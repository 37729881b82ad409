"""Host side of the device query tokeniser (no GPU): the C ABI entries, the pinned-blob pack helper and the
`query_tokenizer` knob."""
import numpy as np
import pytest

NEW_EXPORTS = ("amdr_tokenizer_pack", "amdr_tokenizer_device_create", "amdr_tokenizer_device_reserve",
               "amdr_tokenizer_encode_device", "amdr_tokenizer_device_destroy")


def test_device_tokeniser_entries_are_declared_bound_and_exported():
    import ctypes

    from legal_rag_amd import _native
    from test_abi import header_prototypes
    protos = header_prototypes()
    lib = ctypes.CDLL(str(_native.lib_path()))
    for name in NEW_EXPORTS:
        assert name in _native.EXPORTS and name in protos, name
        assert _native.SIGNATURES[name] == protos[name], name
        assert hasattr(lib, name), name
    assert protos["amdr_tokenizer_encode_device"] == "PPPilPlPPP"


TEXTS = ["What is § 2-314?", "", "rate of 3.5% p.a.", "合同 buyer", "emoji \U0001F600 and 　 space", "x" * 1000,
         "a\0b", "é—ü", ""]


@pytest.mark.parametrize("pystrings", [True, False])
def test_pack_texts_is_the_joined_utf8_bytes_and_cumulative_lengths(pystrings, monkeypatch):
    from legal_rag_amd import _native
    if not pystrings:
        monkeypatch.setattr(_native, "_pystr", None)  # the per-text encode form of utf8_views
    rng = np.random.default_rng(3)
    alphabet = list("abcXYZ0159 +#&._%-\t\r\n") + ["§", "é", "　", "合", "\U0001F600", "\0"]
    fuzz = ["".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=int(rng.integers(0, 30)))) for _ in range(3000)]
    for texts in (TEXTS, fuzz, [], ["only"]):
        blob, offs = _native.pack_texts(texts)
        enc = [t.encode("utf-8") for t in texts]
        assert blob.tobytes() == b"".join(enc)
        assert offs.tolist() == [0] + np.cumsum([len(e) for e in enc], dtype=np.int64).tolist()


def test_utf8_views_flags_every_string_that_may_hold_han():
    from legal_rag_amd import _native, text
    texts = ["plain", "§ latin-1", "— dash (UCS-2)", "合同", "\U0001F600", None]
    _, lens, total, maybe_han, _ = _native.utf8_views(texts)
    assert total == sum(len((t or "").encode()) for t in texts) and lens.tolist()[-1] == 0
    assert maybe_han.tolist()[:2] == [False, False] and maybe_han[3]
    for t, m in zip(texts, maybe_han):
        assert m or not text.contains_han(t or "")  # never a false "no Han"


def test_pack_refuses_a_small_blob_and_copies_nothing():
    import ctypes
    from legal_rag_amd import _native
    ptrs, lens, total, _, keep = _native.utf8_views(["abc", "defg"])
    blob = np.full(8, 7, dtype=np.uint8)
    offs = np.full(3, -5, dtype=np.int64)
    with pytest.raises(_native.NativeError, match="blob too small"):
        _native.pack_utf8(ptrs, lens, blob.ctypes.data, total - 1, offs.ctypes.data)
    assert (blob == 7).all() and (offs == -5).all()
    _native.pack_utf8(ptrs, lens, blob.ctypes.data, total, offs.ctypes.data)
    assert blob[:total].tobytes() == b"abcdefg" and offs.tolist() == [0, 3, 7]
    del keep, ctypes


def test_query_tokenizer_defaults_to_host_and_rejects_unknown_values():
    from types import SimpleNamespace

    from legal_rag_amd.config import AppConfig, RetrievalConfig, query_tokenizer_mode
    assert RetrievalConfig().query_tokenizer == "host"
    assert query_tokenizer_mode(AppConfig()) == "host"
    assert query_tokenizer_mode(SimpleNamespace(retrieval=SimpleNamespace())) == "host"  # duck-typed, knob absent
    assert query_tokenizer_mode(RetrievalConfig(query_tokenizer="device")) == "device"
    with pytest.raises(ValueError, match="query_tokenizer"):
        RetrievalConfig(query_tokenizer="gpu")
    with pytest.raises(ValueError, match="query_tokenizer"):
        query_tokenizer_mode(SimpleNamespace(retrieval=SimpleNamespace(query_tokenizer="Device")))
    cfg = AppConfig()
    assert cfg.with_lang("en").retrieval.query_tokenizer == "host"

"""`cfg.retrieval.dense_image`: the knob of the resident fp16 image of the large dense scan (no GPU)."""
from types import SimpleNamespace

import pytest


def test_dense_image_mode_validation():
    from legal_rag_amd.config import AppConfig, RetrievalConfig, dense_image_mode
    assert dense_image_mode(AppConfig()) == "none"
    assert dense_image_mode(RetrievalConfig()) == "none"
    assert dense_image_mode(SimpleNamespace(retrieval=SimpleNamespace())) == "none"  # duck-typed, knob absent
    assert dense_image_mode(RetrievalConfig(dense_image="fp16")) == "fp16"
    assert dense_image_mode(SimpleNamespace(retrieval=SimpleNamespace(dense_image="fp16"))) == "fp16"
    for bad in ("FP16", "fp8", "half", "", 1, True):
        with pytest.raises(ValueError):
            RetrievalConfig(dense_image=bad)
        with pytest.raises(ValueError):
            dense_image_mode(SimpleNamespace(retrieval=SimpleNamespace(dense_image=bad)))
        with pytest.raises(ValueError):
            dense_image_mode(SimpleNamespace(dense_image=bad))


def test_widths_the_image_supports():
    from legal_rag_amd import _native
    assert [d for d in range(4, 1025, 4) if _native.dense_hi_supported(d)] == [128 * i for i in range(1, 9)]

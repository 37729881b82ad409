"""ctypes binding of libamdretrieval.so (include/amdretrieval.h).

There is NO CPU fallback: if the shared library is missing or a call fails the
error is raised to the caller.  The GIL is released for the duration of every
native call (ctypes.CDLL), so concurrent searches from the retrieval service's
thread pool overlap their host-side work.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from pathlib import Path
from typing import Optional, Sequence, Tuple

import numpy as np

LIB_NAME = "libamdretrieval.so"
MAX_K = 256
MMR_MAX_POOL = 64  # AMDR_MMR_MAX_POOL
MAX_DIM = 1024
MAXSIM_DIM = 128
MAXSIM_QLEN = 32
FUSE_NVALS = 9
FUSE_METHODS = {"rrf_norm_blend": 0, "rrf": 1, "wrrf": 2, "weighted_sum": 3}
FV = dict(score=0, rrf_norm=1, weighted_sum=2, dense_norm=3, bm25_norm=4, colbert_norm=5,
          contrib_dense=6, contrib_bm25=7, contrib_colbert=8)

# argument kinds of every export, in header order: P = pointer (host or device, or an opaque handle /
# handle out-parameter / hipStream_t passed as void*), i = int32_t, l = int64_t, d = double.
# tests/test_abi.py parses include/amdretrieval.h and checks this table against the prototypes, so a
# wrapper can no longer pass a Python int where the ABI wants 64 bits (or the reverse) unnoticed.
SIGNATURES = {
    "amdr_last_error": "", "amdr_version": "", "amdr_device_count": "P", "amdr_device_name": "iPi", "amdr_workspace_growths": "P",
    "amdr_dense_create": "PliiP", "amdr_dense_create_from_device": "PliiP", "amdr_dense_add": "PPl", "amdr_dense_remove": "PPl", "amdr_dense_remove_kernel_ms": "PP", "amdr_dense_replace": "PPPl", "amdr_dense_replace_kernel_ms": "PP",
    "amdr_dense_ntotal": "PP", "amdr_dense_dim": "PP", "amdr_dense_reserve": "Pii", "amdr_dense_search": "PPiiPP",
    "amdr_dense_search_device": "PPiiPPP", "amdr_dense_search_fuse_device": "PPiiPPPPiPPPPPPPP", "amdr_hybrid_small_device": "PPPPPiiiPPPPPPPPPPPP", "amdr_hybrid_batch_device": "PPPPPiiiPPPPPPPPPPPP", "amdr_dense_small_create": "PP", "amdr_dense_small_approx_device": "PPiPlPP", "amdr_dense_small_destroy": "P", "amdr_dense_two_pass_fallbacks": "PP", "amdr_dense_read_rows": "PllP", "amdr_dense_score_rows": "PPiPiP",
    "amdr_dense_plan_info": "PiiPi", "amdr_dense_workspace_plan": "liiiiiP", "amdr_dense_hi_counters": "PP", "amdr_dense_image_build": "P", "amdr_dense_image_drop": "P", "amdr_dense_image_info": "PP", "amdr_dense_profile_begin": "Pi", "amdr_dense_profile_end": "PPP", "amdr_dense_destroy": "P",
    "amdr_bm25_create": "PPPPPlldddiP", "amdr_bm25_ndocs": "PP", "amdr_bm25_add": "PPPPPPlld", "amdr_bm25_info": "PP", "amdr_bm25_add_kernel_ms": "PP", "amdr_bm25_remove": "PPlPlPd", "amdr_bm25_remove_kernel_ms": "PP", "amdr_bm25_replace": "PPlPPPPPlPd", "amdr_bm25_replace_kernel_ms": "PP", "amdr_bm25_add_carry": "PPPPPPlldPP", "amdr_bm25_remove_carry": "PPlPlPd", "amdr_bm25_replace_carry": "PPlPPPPPlPdPP", "amdr_bm25_carry_kernel_ms": "PP", "amdr_bm25_replaces": "PP", "amdr_bm25_read": "PPPPPPP", "amdr_bm25_set_tokens": "PPP", "amdr_bm25_tokens_info": "PP", "amdr_bm25_read_tokens": "PPP", "amdr_bm25_reserve": "Piil", "amdr_bm25_workspace_plan": "liiiiP", "amdr_bm25_plan_info": "PiiPi",
    "amdr_bm25_search": "PPPiiPP", "amdr_bm25_search_device": "PPPiiPPP", "amdr_bm25_scores": "PPPiP",
    "amdr_bm25_destroy": "P",
    "amdr_tokenizer_create": "PPlP", "amdr_tokenizer_encode": "PPPiPlPP", "amdr_tokenizer_encode_joined": "PPliPlPP", "amdr_tokenizer_encode_ptrs": "PPPiPlPP", "amdr_tokenizer_spans": "PlPPiP",
    "amdr_tokenizer_set_han": "PiPPPPld", "amdr_tokenizer_han_mode": "PP", "amdr_tokenizer_spans_han": "PPlPPiP",
    "amdr_tokenizer_destroy": "P",
    "amdr_tokenizer_pack": "PPiPlP", "amdr_tokenizer_device_create": "PiP", "amdr_tokenizer_device_reserve": "Pil",
    "amdr_tokenizer_encode_device": "PPPilPlPPP", "amdr_tokenizer_device_destroy": "P",
    "amdr_maxsim_create": "PPliiP", "amdr_maxsim_add": "PPPl", "amdr_maxsim_remove": "PPl", "amdr_maxsim_remove_kernel_ms": "PP", "amdr_maxsim_replace": "PPPPl", "amdr_maxsim_replace_kernel_ms": "PP", "amdr_maxsim_read": "PPP", "amdr_maxsim_info": "PP", "amdr_maxsim_stats": "PP", "amdr_maxsim_ndocs": "PP", "amdr_maxsim_plan_info": "PiPi", "amdr_maxsim_reserve": "Pii", "amdr_maxsim_workspace_plan": "liiiiiP",
    "amdr_maxsim_search": "PPiiiPP", "amdr_maxsim_search_device": "PPiiiPPP", "amdr_maxsim_scores": "PPiiP",
    "amdr_maxsim_destroy": "P",
    "amdr_fuse": "Pi" + "PPi" * 3 + "PPPP", "amdr_fuse_device": "Pi" + "PPiP" * 3 + "PPPP" + "iP",
    "amdr_rerank_blend": "iiPPPPPidP", "amdr_rerank_blend_device": "iiPPPPPidPiP",
    "amdr_fuse_compact_device": "iiiPPPPPPPPiP",
    "amdr_mmr_device": "PPiPllPiiidPPPPP", "amdr_mmr": "PPiPllPiiidPPPP",
    "amdr_merge_topk_f32_device": "PPiiiiPPiP", "amdr_merge_topk_f64_device": "PPiiiiPPiP",
    "amdr_shard_row_words": "PiP", "amdr_shard_pack_device": "PiilPiP", "amdr_shard_merge_device": "PiiPiiP",
    "amdr_graph_create": "P" * 11 + "illiiP", "amdr_graph_reserve": "Piii", "amdr_graph_walk": "PPPiiiP" + "P" * 7,
    "amdr_graph_search": "PPPPPiiiiP" + "P" * 7, "amdr_graph_search_device": "PPPPPPiiiiP" + "P" * 8,
    "amdr_graph_destroy": "P",
    "amdr_scope_create": "iP", "amdr_scope_reserve": "Piil", "amdr_scope_workspace_plan": "iiliilP", "amdr_scope_plan_info": "PiilPi",
    "amdr_scope_dense_search_device": "PPPPPPiliiPPP", "amdr_scope_bm25_search_device": "PPPPPPPiliiPPP",
    "amdr_scope_maxsim_search_device": "PPPiPPPiliiPPP", "amdr_scope_dense_search": "PPPPPPiiiPP",
    "amdr_scope_bm25_search": "PPPPPPPiiiPP", "amdr_scope_maxsim_search": "PPPiPPPiiiPP", "amdr_scope_destroy": "P",
    "amdr_hybrid_scope_device": "PPPPPP" + "PPPil" * 2 + "iii" + "PPP" + "PPiP" + "PPPP" + "PPPP" + "P",
    "amdr_hybrid_scope_plan": "iiiillPP",
    "amdr_term_scope_plan": "llP", "amdr_term_scope_device": "P" + "P" * 7 + "l" * 5 + "PPP" + "PlP",
    "amdr_term_scope": "P" + "P" * 7 + "l" * 5 + "PPP",
    "amdr_phrase_lists_plan": "llP", "amdr_phrase_lists_device": "PPP" + "lll" + "PPP" + "PlP", "amdr_phrase_lists": "PPP" + "lll" + "PPP",
    "amdr_term_scope_lists_device": "P" + "P" * 9 + "l" * 6 + "PPP" + "PlP", "amdr_term_scope_lists": "P" + "P" * 9 + "l" * 6 + "PPP",
    "amdr_span_lists_plan": "llP", "amdr_span_lists_device": "PPPPP" + "lll" + "PPP" + "PlP", "amdr_span_lists": "PPPPP" + "lll" + "PPP",
    "amdr_union_lists_plan": "llP", "amdr_union_lists_device": "PPP" + "lll" + "PPP" + "PlP", "amdr_union_lists": "PPP" + "ll" + "PPP",
    "amdr_class_spans_plan": "llP", "amdr_class_spans_device": "PPPPP" + "l" + "PP" + "lllll" + "PPP" + "PlP",
    "amdr_class_spans": "PPPPP" + "l" + "PP" + "lll" + "PPP",
    "amdr_bm25_set_breaks": "PPl", "amdr_bm25_breaks_info": "PP", "amdr_bm25_read_breaks": "PP",
    "amdr_unit_spans_plan": "llP", "amdr_unit_spans_device": "PPPP" + "l" + "PP" + "lllll" + "PPP" + "PlP",
    "amdr_unit_spans": "PPPP" + "l" + "PP" + "lll" + "PPP",
    "amdr_bm25_marks_device": "PPlll" + "P" * 8 + "ii" + "P" * 6, "amdr_bm25_marks": "PPlll" + "P" * 8 + "ii" + "P" * 5,
    "amdr_bm25_marks_kernel_ms": "PP",
    "amdr_facet_plan": "liPP", "amdr_facet_counts_device": "PPll" + "PliPi" + "PPPPP" + "PlP",
    "amdr_facet_counts": "P" + "PPll" + "PliPi" + "PPPPP",
    "amdr_vocab_create": "PPliP", "amdr_vocab_destroy": "P", "amdr_vocab_info": "PP", "amdr_vocab_match_plan": "llP",
    "amdr_vocab_match_device": "PPPPP" + "lli" + "PPP" + "PlP", "amdr_vocab_match": "PPPPP" + "lli" + "PPP",
}
EXPORTS = tuple(SIGNATURES)  # every symbol include/amdretrieval.h declares (checked by tests/test_abi.py)
_KIND = {"P": C.c_void_p, "i": C.c_int32, "l": C.c_int64, "d": C.c_double}


class NativeError(RuntimeError):
    """A libamdretrieval call returned a non-zero status."""


class FuseParams(C.Structure):
    _fields_ = [("method", C.c_int32), ("rrf_k", C.c_int32), ("alpha", C.c_double), ("w_dense", C.c_double),
                ("w_bm25", C.c_double), ("w_colbert", C.c_double), ("min_final_score", C.c_double)]


class ShardChan(C.Structure):
    """amdr_shard_chan_t: one channel of the shard exchange (device pointers)."""
    _fields_ = [("scores", C.c_void_p), ("ids", C.c_void_p), ("k", C.c_int32), ("f64", C.c_int32)]


class GraphParams(C.Structure):
    """amdr_graph_params_t: per-call parameters of the graph channel (table pointers: host for walk / search, device
    for search_device)."""
    _fields_ = [("limit", C.c_int32), ("default_depth", C.c_int32), ("lang", C.c_int32), ("pad0", C.c_int32),
                ("min_conf", C.c_double), ("rel_max_depth", C.c_void_p), ("rel_allowed", C.c_void_p),
                ("rel_weight", C.c_void_p), ("decay", C.c_void_p)]


GRAPH_MAX_LIMIT = 4096
GRAPH_MAX_SEEDS = 1024


_lib: Optional[C.CDLL] = None


_pystr = False


def _pystrings():
    """The CPython helper next to the library (lib/_amdr_pystrings.so: UTF-8 views of a list of str without copies), or
    None when it was not built — the tokeniser then takes the joined-blob form.  Host glue only: no compute."""
    global _pystr
    if _pystr is False:
        _pystr = None
        p = lib_path().parent / "_amdr_pystrings.so"
        if p.exists() and os.environ.get("AMDR_NO_PYSTRINGS") != "1":
            try:
                import importlib.machinery
                import importlib.util
                loader = importlib.machinery.ExtensionFileLoader("_amdr_pystrings", str(p))
                spec = importlib.util.spec_from_loader("_amdr_pystrings", loader)
                mod = importlib.util.module_from_spec(spec)
                loader.exec_module(mod)
                _pystr = mod
            except Exception:  # noqa: BLE001 - glue is optional
                _pystr = None
    return _pystr


def lib_path() -> Path:
    env = os.environ.get("AMDR_LIB")
    if env:
        return Path(env)
    return Path(__file__).resolve().parent / "lib" / LIB_NAME


def load() -> C.CDLL:
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own libamdhip64.so (SONAME libamdhip64.so.7).  If torch is
    # going to be used in this process it must be loaded FIRST so that this library's
    # NEEDED libamdhip64.so.7 resolves to the runtime torch already mapped: one HIP runtime
    # per process, and torch device pointers / stream handles are then valid here.
    if os.environ.get("AMDR_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:  # noqa: BLE001 - torch is optional for the numpy-only API
            pass
    p = lib_path()
    if not p.exists():
        raise NativeError(
            f"{p} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(or `make -C legal-rag_amd/csrc`). There is no CPU fallback.")
    lib = C.CDLL(str(p))
    lib.amdr_last_error.restype = C.c_char_p
    for name in EXPORTS:
        fn = getattr(lib, name)  # raises AttributeError if a declared symbol is missing
        if name != "amdr_last_error":
            fn.restype = C.c_int
        fn.argtypes = [_KIND[k] for k in SIGNATURES[name]]
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().amdr_last_error()
        raise NativeError(f"{what} failed (status {rc}): {msg.decode('utf-8', 'replace') if msg else ''}")


def dense_hi_supported(d: int) -> bool:
    """Widths the fp16 first pass of large dense scans (and its resident image) supports: csrc/dense_hi.hip."""
    return 128 <= int(d) <= 1024 and int(d) % 128 == 0


def device_count() -> int:
    n = C.c_int32(0)
    rc = load().amdr_device_count(C.byref(n))
    return int(n.value) if rc == 0 else 0


def device_name(device: int = 0) -> str:
    buf = C.create_string_buffer(256)
    _check(load().amdr_device_name(C.c_int32(device), buf, C.c_int32(256)), "amdr_device_name")
    return buf.value.decode()


def dense_workspace_plan(n: int, d: int, nq_max: int, k_max: int, nq: int,
                         k: int) -> Tuple[Tuple[int, int, int], Tuple[int, int, int]]:
    """(bytes DenseIndex.reserve(nq_max, k_max) sizes, bytes the largest pass of search_device(nq, k) uses), each as
    (score matrix, slab lists, candidate-tile lists) — host-only arithmetic."""
    out = (C.c_int64 * 6)()
    _check(load().amdr_dense_workspace_plan(C.c_int64(n), C.c_int32(d), C.c_int32(nq_max), C.c_int32(k_max), C.c_int32(nq),
                                            C.c_int32(k), out), "amdr_dense_workspace_plan")
    v = [int(x) for x in out]
    return tuple(v[:3]), tuple(v[3:])


def bm25_workspace_plan(n_docs: int, nq_max: int, k_max: int, nq: int, k: int) -> Tuple[int, int]:
    """(bytes BM25Index.reserve(nq_max, k_max) sizes, bytes a search_device(nq, k) uses) — host-only arithmetic."""
    out = (C.c_int64 * 2)()
    _check(load().amdr_bm25_workspace_plan(C.c_int64(n_docs), C.c_int32(nq_max), C.c_int32(k_max), C.c_int32(nq),
                                           C.c_int32(k), out), "amdr_bm25_workspace_plan")
    return int(out[0]), int(out[1])


TERM_SCOPE_TILE = 1024  # candidates per block of amdr_term_scope (kTsTile)


def term_scope_plan(n_cons: int, cand_max: int) -> int:
    """Workspace bytes of BM25Index.term_scope_device(n_cons constraints, longest driver cand_max) — host-only arithmetic."""
    out = C.c_int64(0)
    _check(load().amdr_term_scope_plan(C.c_int64(n_cons), C.c_int64(cand_max), C.byref(out)), "amdr_term_scope_plan")
    return int(out.value)


PHRASE_TILE = 256    # candidates per block of amdr_phrase_lists (kPhTile)
PHRASE_MAX_LEN = 16  # tokens of a phrase (kPhMaxLen)


def phrase_lists_plan(n_phr: int, cand_max: int) -> int:
    """Workspace bytes of BM25Index.phrase_lists_device(n_phr phrases, longest driver cand_max) — host-only arithmetic."""
    out = C.c_int64(0)
    _check(load().amdr_phrase_lists_plan(C.c_int64(n_phr), C.c_int64(cand_max), C.byref(out)), "amdr_phrase_lists_plan")
    return int(out.value)


NEAR_MAX_TERMS = 8    # tokens of a Near (kNearMaxTerms)
NEAR_MAX_DIST = 255   # the largest distance of a Near (kNearMaxDist)
SPAN_PHRASE, SPAN_NEAR_UNORDERED, SPAN_NEAR_ORDERED = 0, 1, 2  # the item kinds of amdr_span_lists (near_rule.hpp SpanKind)


def span_lists_plan(n_items: int, cand_max: int) -> int:
    """Workspace bytes of BM25Index.span_lists_device(n_items phrases and Nears, longest driver cand_max) — host-only
    arithmetic, the phrase plan's."""
    out = C.c_int64(0)
    _check(load().amdr_span_lists_plan(C.c_int64(n_items), C.c_int64(cand_max), C.byref(out)), "amdr_span_lists_plan")
    return int(out.value)


UNION_TILE = 32768  # documents per tile of amdr_union_lists (kUnTile)


def union_lists_plan(n_items: int, n_docs: int) -> int:
    """Workspace bytes of BM25Index.union_lists_device(n_items union items) on an index of n_docs documents — host-only
    arithmetic."""
    out = C.c_int64(0)
    _check(load().amdr_union_lists_plan(C.c_int64(n_items), C.c_int64(n_docs), C.byref(out)), "amdr_union_lists_plan")
    return int(out.value)


def class_spans_plan(n_items: int, cand_max: int) -> int:
    """Workspace bytes of BM25Index.class_spans_device(n_items class spans, longest driver cand_max) — host-only arithmetic:
    per cell (item, tile of PHRASE_TILE candidates) two i64 and the parked ranks."""
    out = C.c_int64(0)
    _check(load().amdr_class_spans_plan(C.c_int64(n_items), C.c_int64(cand_max), C.byref(out)), "amdr_class_spans_plan")
    return int(out.value)


def unit_spans_plan(n_items: int, cand_max: int) -> int:
    """Workspace bytes of BM25Index.unit_spans_device(n_items unit items, longest driver cand_max) — host-only arithmetic:
    per cell (item, tile of PHRASE_TILE candidates) two i64 and the parked ranks."""
    out = C.c_int64(0)
    _check(load().amdr_unit_spans_plan(C.c_int64(n_items), C.c_int64(cand_max), C.byref(out)), "amdr_unit_spans_plan")
    return int(out.value)


FACET_TILE_ROWS = 2048  # rows of a scope per block of amdr_facet_counts (AMDR_FACET_TILE_ROWS)
FACET_LDS_BINS = 4096   # the widest field a block bins in LDS (AMDR_FACET_LDS_BINS)
FACET_MAX_TOP = 64      # AMDR_FACET_MAX_TOP
FACET_MAX_FIELDS = 8


def facet_plan(n_cons: int, n_codes: Sequence[int]) -> int:
    """Workspace bytes of facet_counts_device(n_cons constraints, fields of n_codes values each) — host-only arithmetic."""
    nc = _c(n_codes, np.int64).ravel()
    out = C.c_int64(0)
    _check(load().amdr_facet_plan(C.c_int64(n_cons), C.c_int32(nc.size), _p(nc, C.c_int64), C.byref(out)), "amdr_facet_plan")
    return int(out.value)


def facet_counts_device(scope_ptr: int, rows: int, n_cons: int, rows_max: int, codes: int, n_rows: int, n_codes: Sequence[int],
                        top: int, out_total: int, out_missing: int, out_distinct: int, out_code: int, out_count: int,
                        work: int, work_bytes: int, stream: int = 0) -> None:
    """amdr_facet_counts_device: device pointers in, enqueue only, on the current device.  n_codes is a host sequence, one
    entry per field of the field-major code columns `codes` i32 [n_fields, n_rows]."""
    nc = _c(n_codes, np.int64).ravel()
    _check(load().amdr_facet_counts_device(_vp(scope_ptr), _vp(rows), C.c_int64(n_cons), C.c_int64(rows_max), _vp(codes),
                                           C.c_int64(n_rows), C.c_int32(nc.size), _p(nc, C.c_int64), C.c_int32(top),
                                           _vp(out_total), _vp(out_missing), _vp(out_distinct), _vp(out_code), _vp(out_count),
                                           _vp(work), C.c_int64(work_bytes), _vp(stream)), "amdr_facet_counts_device")


VOCAB_TILE_TERMS = 8192   # term ids per tile of amdr_vocab_match (AMDR_VOCAB_TILE_TERMS, kVmTile)
VOCAB_MAX_PATTERN = 64    # code points of a pattern (AMDR_VOCAB_MAX_PATTERN)
VOCAB_MAX_ITEMS = 4096    # the widest row of matches (AMDR_VOCAB_MAX_ITEMS)
VOCAB_ANY_ONE = 0x110000  # '?' in a Wildcard's code points
VOCAB_ANY_RUN = 0x110001  # '*'


def vocab_match_plan(n_terms: int, n_pat: int) -> int:
    """Workspace bytes of VocabIndex.match_device(n_pat patterns) on a vocabulary of n_terms — host-only arithmetic: per
    cell (pattern, tile of VOCAB_TILE_TERMS terms) two i64 and the 1 KiB bitmap, each region aligned to 256 bytes."""
    out = C.c_int64(0)
    _check(load().amdr_vocab_match_plan(C.c_int64(n_terms), C.c_int64(n_pat), C.byref(out)), "amdr_vocab_match_plan")
    return int(out.value)


def maxsim_workspace_plan(n_docs: int, split_image: bool, nq_max: int, k_max: int, nq: int, k: int) -> Tuple[int, int]:
    """(bytes MaxSimIndex.reserve(nq_max, k_max) sizes, bytes a search_device(nq, k) uses) on a store with / without
    its split-fp16 images — host-only arithmetic."""
    out = (C.c_int64 * 2)()
    _check(load().amdr_maxsim_workspace_plan(C.c_int64(n_docs), C.c_int32(1 if split_image else 0), C.c_int32(nq_max),
                                             C.c_int32(k_max), C.c_int32(nq), C.c_int32(k), out),
           "amdr_maxsim_workspace_plan")
    return int(out[0]), int(out[1])


def workspace_growths() -> int:
    """Device workspace (re)allocations of every handle in this process so far: a "_device" call within its handle's
    reserve leaves the count unchanged (what makes it capturable)."""
    n = C.c_int64(0)
    _check(load().amdr_workspace_growths(C.byref(n)), "amdr_workspace_growths")
    return int(n.value)


def _p(a: Optional[np.ndarray], ctype):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(ctype))


def _vp(ptr: int):
    return C.c_void_p(int(ptr) if ptr else 0)


def _c(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=dtype)


class _Handle:
    """An opaque library handle `_h`, released by close() or garbage collection through the export `_destroy` names
    (tolerant of a missing `_h`: a constructor can raise before it exists)."""
    _destroy = ""

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            getattr(load(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _plan_info(self, name: str, *dims: int) -> str:
        """The text an amdr_*_plan_info export writes for these dimensions (no device work)."""
        buf = C.create_string_buffer(1024)
        _check(getattr(load(), name)(self._h, *(C.c_int32(x) for x in dims), buf, C.c_int32(len(buf))), name)
        return buf.value.decode()


# ---------------------------------------------------------------------------
class DenseIndex(_Handle):
    """Exact inner-product index resident in HBM (replaces faiss IndexFlatIP /
    IndexHNSWFlat behind `index.search`, dense_retriever.py:42)."""
    _destroy = "amdr_dense_destroy"

    def __init__(self, X: Optional[np.ndarray] = None, *, device: int = 0, dim: Optional[int] = None,
                 device_ptr: Optional[int] = None, n: Optional[int] = None, keepalive=None):
        lib = load()
        self._h = C.c_void_p()
        self.device = int(device)
        self._keepalive = keepalive
        if device_ptr is not None:
            assert n is not None and dim is not None
            _check(lib.amdr_dense_create_from_device(_vp(device_ptr), C.c_int64(n), C.c_int32(dim),
                                                     C.c_int32(device), C.byref(self._h)),
                   "amdr_dense_create_from_device")
            self.d = int(dim)
        else:
            if X is None:
                X = np.zeros((0, int(dim)), dtype=np.float32)
            X = _c(X, np.float32)
            if X.ndim != 2:
                raise ValueError("X must be [n, d]")
            self.d = int(X.shape[1])
            _check(lib.amdr_dense_create(_p(X, C.c_float), C.c_int64(X.shape[0]), C.c_int32(self.d),
                                         C.c_int32(device), C.byref(self._h)), "amdr_dense_create")

    @property
    def ntotal(self) -> int:
        n = C.c_int64(0)
        _check(load().amdr_dense_ntotal(self._h, C.byref(n)), "amdr_dense_ntotal")
        return int(n.value)

    def add(self, X: np.ndarray) -> None:
        X = _c(X, np.float32)
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError(f"add: expected [*, {self.d}]")
        _check(load().amdr_dense_add(self._h, _p(X, C.c_float), C.c_int64(X.shape[0])), "amdr_dense_add")

    def remove(self, ids) -> None:
        """Remove rows (amdr_dense_remove): ids strictly ascending old row ids; the survivors are renumbered
        0 .. n-1 in their old order and the handle is then what DenseIndex makes of them, bit for bit.  Row ids held
        elsewhere (graph tables, scope tables, row2uid maps) name the old rows and are the caller's to rebuild."""
        ids = _c(np.asarray(ids, dtype=np.int64).reshape(-1), np.int64)
        _check(load().amdr_dense_remove(self._h, _p(ids, C.c_int64), C.c_int64(ids.shape[0])), "amdr_dense_remove")

    def remove_kernel_ms(self) -> float:
        """Device time of the last remove's compaction kernel, in ms (-1.0 before the first remove)."""
        ms = C.c_double(0)
        _check(load().amdr_dense_remove_kernel_ms(self._h, C.byref(ms)), "amdr_dense_remove_kernel_ms")
        return float(ms.value)

    def replace(self, ids, X: np.ndarray) -> None:
        """Replace rows under their ids (amdr_dense_replace): ids strictly ascending row ids, row ids[i] takes X[i].  No
        row moves; the handle is then what DenseIndex makes of the edited matrix, bit for bit."""
        ids = _c(np.asarray(ids, dtype=np.int64).reshape(-1), np.int64)
        X = _c(X, np.float32)
        if X.ndim != 2 or X.shape[1] != self.d or X.shape[0] != ids.shape[0]:
            raise ValueError(f"replace: expected [{ids.shape[0]}, {self.d}]")
        _check(load().amdr_dense_replace(self._h, _p(ids, C.c_int64), _p(X, C.c_float), C.c_int64(ids.shape[0])),
               "amdr_dense_replace")

    def replace_kernel_ms(self) -> float:
        """Device time of the last replace's scatter kernel, in ms (-1.0 before the first replace)."""
        ms = C.c_double(0)
        _check(load().amdr_dense_replace_kernel_ms(self._h, C.byref(ms)), "amdr_dense_replace_kernel_ms")
        return float(ms.value)

    def reserve(self, nq_max: int, k_max: int) -> None:
        _check(load().amdr_dense_reserve(self._h, C.c_int32(nq_max), C.c_int32(k_max)), "amdr_dense_reserve")

    def search(self, Q: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """faiss-shaped: (scores f32[nq,k], ids i64[nq,k]), -1 padded."""
        Q = _c(Q, np.float32)
        if Q.ndim == 1:
            Q = Q[None, :]
        if Q.shape[1] != self.d:
            raise ValueError(f"search: query dim {Q.shape[1]} != index dim {self.d}")
        nq = Q.shape[0]
        scores = np.empty((nq, k), dtype=np.float32)
        ids = np.empty((nq, k), dtype=np.int64)
        _check(load().amdr_dense_search(self._h, _p(Q, C.c_float), C.c_int32(nq), C.c_int32(k),
                                        _p(scores, C.c_float), _p(ids, C.c_int64)), "amdr_dense_search")
        return scores, ids

    def search_device(self, q_ptr: int, nq: int, k: int, scores_ptr: int, ids_ptr: int, stream: int = 0) -> None:
        _check(load().amdr_dense_search_device(self._h, _vp(q_ptr), C.c_int32(nq), C.c_int32(k), _vp(scores_ptr),
                                               _vp(ids_ptr), _vp(stream)), "amdr_dense_search_device")

    def two_pass_fallbacks(self) -> int:
        """Queries of the two-pass long-batch searches so far that re-scored their whole row (amdr_dense_two_pass_fallbacks)."""
        out = C.c_int64(0)
        _check(load().amdr_dense_two_pass_fallbacks(self._h, C.byref(out)), "amdr_dense_two_pass_fallbacks")
        return int(out.value)

    def search_fuse_device(self, params: "FuseParams", q_ptr: int, nq: int, k: int, bm25, dense_row2uid: int,
                           scores_ptr: int, ids_ptr: int, out_ids: int, out_vals: int, out_mask: int, out_count: int,
                           stream: int = 0) -> None:
        """search_device + fuse_device(dense, bm25) as one native call (amdr_dense_search_fuse_device).
        bm25 = (ids_ptr, scores_ptr, kb, row2uid_ptr | 0)."""
        _check(load().amdr_dense_search_fuse_device(
            self._h, _vp(q_ptr), C.c_int32(nq), C.c_int32(k), C.byref(params), _vp(dense_row2uid), _vp(bm25[0]),
            _vp(bm25[1]), C.c_int32(bm25[2]), _vp(bm25[3]), _vp(scores_ptr), _vp(ids_ptr), _vp(out_ids), _vp(out_vals),
            _vp(out_mask), _vp(out_count), _vp(stream)), "amdr_dense_search_fuse_device")

    def score_rows(self, Q: np.ndarray, rows: np.ndarray) -> np.ndarray:
        """out[q, j] = <Q[q], X[rows[q, j]]> (rows outside [0, n) -> -FLT_MAX)."""
        Q = _c(Q, np.float32)
        if Q.ndim == 1:
            Q = Q[None, :]
        rows = _c(rows, np.int64).reshape(Q.shape[0], -1)
        out = np.empty(rows.shape, dtype=np.float32)
        _check(load().amdr_dense_score_rows(self._h, _p(Q, C.c_float), C.c_int32(Q.shape[0]), _p(rows, C.c_int64),
                                            C.c_int32(rows.shape[1]), _p(out, C.c_float)), "amdr_dense_score_rows")
        return out

    def mmr(self, rows: np.ndarray, rel: np.ndarray, count: np.ndarray, pool: int, k_sel: int,
            lam: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """Maximal-marginal-relevance selection (amdr_mmr; the definition is in include/amdretrieval.h): rows [nq, >= pool]
        int64 rows of this index in rank order, rel [nq, >= pool] float64 (a strided view, such as the score column of a
        packed fused result, is read in place), count [nq].  -> (pos, mmr, maxsim) [nq, k_sel] and count [nq]."""
        rows = np.asarray(rows, dtype=np.int64)
        if rows.ndim != 2 or rows.shape[0] and (rows.strides[1] != 8 or rows.strides[0] % 8 or rows.strides[0] < 0):
            rows = _c(rows, np.int64).reshape(len(rows), -1)
        nq = rows.shape[0]
        rel = np.asarray(rel, dtype=np.float64)
        if rel.ndim != 2 or nq and (rel.strides[1] % 8 or rel.strides[1] < 8 or rel.strides[0] % 8 or rel.strides[0] < 0):
            rel = _c(rel, np.float64).reshape(nq, -1)
        count = _c(count, np.int32).reshape(-1)
        if rel.shape[0] != nq or count.shape[0] != nq:
            raise ValueError(f"mmr: rows, rel and count disagree on the batch ({nq}, {rel.shape[0]}, {count.shape[0]})")
        if nq and rel.shape[1] < min(int(pool), rows.shape[1]):
            raise ValueError(f"mmr: rel holds {rel.shape[1]} columns, fewer than the pool of {pool}")
        ks = max(int(k_sel), 0)
        pos = np.empty((nq, ks), dtype=np.int32)
        val = np.empty((nq, ks), dtype=np.float64)
        sim = np.empty((nq, ks), dtype=np.float64)
        cnt = np.empty(nq, dtype=np.int32)
        ld_rows = rows.strides[0] // 8 if nq > 1 else rows.shape[1]
        rel_stride, rel_ld = (rel.strides[1] // 8, rel.strides[0] // 8) if nq else (1, 0)
        _check(load().amdr_mmr(self._h, _p(rows, C.c_int64), C.c_int32(ld_rows), _p(rel, C.c_double), C.c_int64(rel_stride),
                               C.c_int64(rel_ld), _p(count, C.c_int32), C.c_int32(nq), C.c_int32(pool), C.c_int32(k_sel),
                               C.c_double(lam), _p(pos, C.c_int32), _p(val, C.c_double), _p(sim, C.c_double),
                               _p(cnt, C.c_int32)), "amdr_mmr")
        return pos, val, sim, cnt

    def mmr_device(self, rows, rel, count, nq: int, pool: int, k_sel: int, lam: float, out_pos, out_mmr, out_maxsim,
                   out_count, *, ld_rows: Optional[int] = None, rel_stride: Optional[int] = None,
                   rel_ld: Optional[int] = None, stream: int = 0) -> None:
        """amdr_mmr_device: enqueue only, no workspace.  Every buffer is a torch tensor on this index's device or a device
        address; the strides (in elements) default to those of the tensors `rows` [nq, ld] and `rel` [nq, pool] (a view)."""
        def addr(t):
            return int(t.data_ptr()) if hasattr(t, "data_ptr") else int(t or 0)

        def stride(t, axis, given, what):
            if given is not None:
                return int(given)
            if not hasattr(t, "stride"):
                raise ValueError(f"mmr_device: {what} is needed when a device address is passed")
            return int(t.stride(axis))
        _check(load().amdr_mmr_device(self._h, _vp(addr(rows)), C.c_int32(stride(rows, 0, ld_rows, "ld_rows")), _vp(addr(rel)),
                                      C.c_int64(stride(rel, 1, rel_stride, "rel_stride")),
                                      C.c_int64(stride(rel, 0, rel_ld, "rel_ld")), _vp(addr(count)), C.c_int32(nq),
                                      C.c_int32(pool), C.c_int32(k_sel), C.c_double(lam), _vp(addr(out_pos)),
                                      _vp(addr(out_mmr)), _vp(addr(out_maxsim)), _vp(addr(out_count)), _vp(stream)),
               "amdr_mmr_device")

    def read_rows(self, row0: int, nrows: int) -> np.ndarray:
        out = np.empty((nrows, self.d), dtype=np.float32)
        _check(load().amdr_dense_read_rows(self._h, C.c_int64(row0), C.c_int64(nrows), _p(out, C.c_float)),
               "amdr_dense_read_rows")
        return out

    def plan_info(self, nq: int, k: int) -> str:
        """Kernels a search of nq queries at depth k launches on this index, and the cut of the work."""
        return self._plan_info("amdr_dense_plan_info", nq, k)

    def hi_counters(self) -> Tuple[int, int, int, bool, int, int]:
        """(queries that took the fp16 first pass of large scans, those it could not resolve, current width level 0-2,
        pass still in use, passes, passes that also ran the exact chain).  Synchronises the device."""
        out = (C.c_int64 * 6)()
        _check(load().amdr_dense_hi_counters(self._h, out), "amdr_dense_hi_counters")
        return int(out[0]), int(out[1]), int(out[2]), bool(out[3]), int(out[4]), int(out[5])

    def build_image(self) -> None:
        """Resident fp16 image for the fp16 first pass of large scans (amdr_dense_image_build): synchronous, idempotent,
        +50 % memory, no returned bit changes.  NativeError for a width the pass does not support or a matrix whose
        statistics are not finite."""
        _check(load().amdr_dense_image_build(self._h), "amdr_dense_image_build")

    def drop_image(self) -> None:
        _check(load().amdr_dense_image_drop(self._h), "amdr_dense_image_drop")

    def image_info(self) -> Tuple[bool, int, int, int]:
        """(present, bytes, rows covered, e of the scale 2^-e)."""
        out = (C.c_int64 * 4)()
        _check(load().amdr_dense_image_info(self._h, out), "amdr_dense_image_info")
        return bool(out[0]), int(out[1]), int(out[2]), int(out[3])

    def profile_begin(self, max_launches: int) -> None:
        _check(load().amdr_dense_profile_begin(self._h, C.c_int32(max_launches)), "amdr_dense_profile_begin")

    def profile_end(self) -> Tuple[float, int]:
        ms, n = C.c_double(0), C.c_int32(0)
        _check(load().amdr_dense_profile_end(self._h, C.byref(ms), C.byref(n)), "amdr_dense_profile_end")
        return float(ms.value), int(n.value)


# ---------------------------------------------------------------------------
class BM25Index(_Handle):
    """Okapi BM25 over term-major CSR postings (replaces BM25Okapi.get_scores +
    the Python sort, bm25_retriever.py:74-75)."""
    _destroy = "amdr_bm25_destroy"

    def __init__(self, term_ptr, post_doc, post_tf, idf, doc_len, avgdl: float, k1: float = 1.5, b: float = 0.75,
                 *, device: int = 0):
        lib = load()
        self._arrs = (_c(term_ptr, np.int64), _c(post_doc, np.int32), _c(post_tf, np.int32), _c(idf, np.float64),
                      _c(doc_len, np.int32))
        tp, pd, pt, idf_, dl = self._arrs
        self.n_terms = int(tp.shape[0] - 1)
        self.n_docs = int(dl.shape[0])
        self.device = int(device)
        self._h = C.c_void_p()
        _check(lib.amdr_bm25_create(_p(tp, C.c_int64), _p(pd, C.c_int32), _p(pt, C.c_int32), _p(idf_, C.c_double),
                                    _p(dl, C.c_int32), C.c_int64(self.n_terms), C.c_int64(self.n_docs),
                                    C.c_double(avgdl), C.c_double(k1), C.c_double(b), C.c_int32(device),
                                    C.byref(self._h)), "amdr_bm25_create")
        self._arrs = None  # the library holds its own device copy

    @staticmethod
    def _token_args(tokens, n_docs: int, what: str):
        """(tok_ptr_add i64 [n_docs + 1], tok_add i32 or None when it is empty) of a carrying update."""
        tp, tk = _c(tokens[0], np.int64), _c(tokens[1], np.int32)
        if tp.ndim != 1 or tk.ndim != 1 or tp.shape[0] != n_docs + 1 or (n_docs >= 0 and tk.shape[0] < int(tp[-1])):
            raise ValueError(f"{what}: tokens = (tok_ptr_add [n + 1], tok_add [tok_ptr_add[-1]])")
        return tp, (tk if tk.shape[0] else None)

    def add(self, term_ptr_add, post_doc_add, post_tf_add, idf, doc_len_add, avgdl: float, tokens=None) -> None:
        """Append documents (amdr_bm25_add): the added documents' own term-major CSR over the new term table (local
        document ids from 0; len(term_ptr_add) - 1 = the new number of terms >= n_terms), their lengths, the WHOLE new
        idf vector and the new avgdl.  Afterwards the index is what BM25Index makes of the concatenated arrays, bit for
        bit.  A "_device" caller finishes its work first and reserves again.  The token stream is dropped; with
        tokens = (tok_ptr_add [n_add + 1], tok_add) — the added documents' texts as term ids over the new table — the call
        is amdr_bm25_add_carry: a resident stream gets the added documents behind it instead."""
        tp, pd, pt = _c(term_ptr_add, np.int64), _c(post_doc_add, np.int32), _c(post_tf_add, np.int32)
        idf_, dl = _c(idf, np.float64), _c(doc_len_add, np.int32)
        if tp.ndim != 1 or tp.shape[0] < 1 or idf_.shape != (tp.shape[0] - 1,) or pd.shape != pt.shape:
            raise ValueError("add: term_ptr_add [V + 1], idf [V], post_doc_add and post_tf_add of one length")
        if dl.shape[0] and (pd.shape[0] < int(tp[-1])):
            raise ValueError("add: term_ptr_add points past the postings")
        args = (self._h, _p(tp, C.c_int64), _p(pd, C.c_int32), _p(pt, C.c_int32), _p(idf_, C.c_double), _p(dl, C.c_int32),
                C.c_int64(tp.shape[0] - 1), C.c_int64(dl.shape[0]), C.c_double(avgdl))
        if tokens is None:
            _check(load().amdr_bm25_add(*args), "amdr_bm25_add")
        else:
            kp, kt = self._token_args(tokens, int(dl.shape[0]), "add")
            _check(load().amdr_bm25_add_carry(*args, _p(kp, C.c_int64), None if kt is None else _p(kt, C.c_int32)),
                   "amdr_bm25_add_carry")
        self.n_docs, self.n_terms = self.info()[:2]

    def remove(self, remove_ids, idf, avgdl: float, term_map=None, carry: bool = False) -> None:
        """Remove documents (amdr_bm25_remove): remove_ids strictly ascending old ids (not all of them); the survivors are
        renumbered 0 .. n-1 in their old order.  term_map[n_terms]: the new id of each old term or -1, a bijection onto
        [0, len(idf)) (None: the identity, len(idf) == n_terms); idf: the WHOLE new vector; avgdl: the new value.
        Afterwards the index is what BM25Index makes of the survivors' arrays, bit for bit.  A "_device" caller finishes
        its work first and reserves again.  The token stream is dropped; carry=True is amdr_bm25_remove_carry: a resident
        stream keeps the survivors' texts, rewritten through the map."""
        ids, idf_ = _c(remove_ids, np.int64), _c(idf, np.float64)
        tm = None if term_map is None else _c(term_map, np.int32)
        if ids.ndim != 1 or idf_.ndim != 1 or (tm is not None and tm.shape != (self.n_terms,)):
            raise ValueError("remove: remove_ids [n_remove], idf [n_terms_new], term_map [n_terms] or None")
        name = "amdr_bm25_remove_carry" if carry else "amdr_bm25_remove"
        _check(getattr(load(), name)(self._h, _p(ids, C.c_int64), C.c_int64(ids.shape[0]),
                                     None if tm is None else _p(tm, C.c_int32), C.c_int64(idf_.shape[0]),
                                     _p(idf_, C.c_double), C.c_double(avgdl)), name)
        self.n_docs, self.n_terms = self.info()[:2]

    def remove_kernel_ms(self) -> float:
        """Summed device time of the last remove's passes in ms (-1 before the first remove)."""
        ms = C.c_double(-1.0)
        _check(load().amdr_bm25_remove_kernel_ms(self._h, C.byref(ms)), "amdr_bm25_remove_kernel_ms")
        return float(ms.value)

    def replace(self, replace_ids, term_ptr_add, post_doc_add, post_tf_add, doc_len_add, idf, avgdl: float,
                term_map=None, tokens=None) -> None:
        """Replace documents under their ids (amdr_bm25_replace): replace_ids strictly ascending; the new documents' own
        term-major CSR over the NEW term table (local id i = document replace_ids[i]) and their lengths; term_map[n_terms]:
        the new id of each old term or -1, injective (None: the identity, new terms behind the old); new ids no old term
        maps to are new terms; idf: the WHOLE new vector; avgdl: the new value.  No document id moves.  Afterwards the
        index is what BM25Index makes of the edited arrays, bit for bit.  A "_device" caller finishes its work first and
        reserves again.  The token stream is dropped; with tokens = (tok_ptr_add [n_rep + 1], tok_add) — the new
        documents' texts as term ids over the new table — the call is amdr_bm25_replace_carry: a resident stream takes them
        in place and keeps every other document's text, rewritten through the map."""
        ids = _c(replace_ids, np.int64)
        tp, pd, pt = _c(term_ptr_add, np.int64), _c(post_doc_add, np.int32), _c(post_tf_add, np.int32)
        idf_, dl = _c(idf, np.float64), _c(doc_len_add, np.int32)
        tm = None if term_map is None else _c(term_map, np.int32)
        if (ids.ndim != 1 or tp.ndim != 1 or tp.shape[0] < 1 or idf_.shape != (tp.shape[0] - 1,) or pd.shape != pt.shape
                or dl.shape != ids.shape or (tm is not None and tm.shape != (self.n_terms,))):
            raise ValueError("replace: replace_ids and doc_len_add [n_rep], term_ptr_add [V + 1], idf [V], post_doc_add and "
                             "post_tf_add of one length, term_map [n_terms] or None")
        if ids.shape[0] and pd.shape[0] < int(tp[-1]):
            raise ValueError("replace: term_ptr_add points past the postings")
        args = (self._h, _p(ids, C.c_int64), C.c_int64(ids.shape[0]), _p(tp, C.c_int64), _p(pd, C.c_int32),
                _p(pt, C.c_int32), _p(dl, C.c_int32), None if tm is None else _p(tm, C.c_int32), C.c_int64(idf_.shape[0]),
                _p(idf_, C.c_double), C.c_double(avgdl))
        if tokens is None:
            _check(load().amdr_bm25_replace(*args), "amdr_bm25_replace")
        else:
            kp, kt = self._token_args(tokens, int(ids.shape[0]), "replace")
            _check(load().amdr_bm25_replace_carry(*args, _p(kp, C.c_int64), None if kt is None else _p(kt, C.c_int32)),
                   "amdr_bm25_replace_carry")
        self.n_docs, self.n_terms = self.info()[:2]

    def replace_kernel_ms(self) -> float:
        """Summed device time of the last replace's passes in ms (-1 before the first replace)."""
        ms = C.c_double(-1.0)
        _check(load().amdr_bm25_replace_kernel_ms(self._h, C.byref(ms)), "amdr_bm25_replace_kernel_ms")
        return float(ms.value)

    def carry_kernel_ms(self) -> float:
        """Summed device time of the carry passes of the last carrying update that carried a stream, in ms (-1 before
        the first one)."""
        ms = C.c_double(-1.0)
        _check(load().amdr_bm25_carry_kernel_ms(self._h, C.byref(ms)), "amdr_bm25_carry_kernel_ms")
        return float(ms.value)

    def replaces(self) -> int:
        """Replaces so far (amdr_bm25_replaces)."""
        n = C.c_int64(0)
        _check(load().amdr_bm25_replaces(self._h, C.byref(n)), "amdr_bm25_replaces")
        return int(n.value)

    def info(self) -> Tuple[int, int, int, int, int, int]:
        """(n_docs, n_terms, postings, adds so far, the tile length in postings of the add's and the remove's kernels,
        removes so far)."""
        out = (C.c_int64 * 6)()
        _check(load().amdr_bm25_info(self._h, out), "amdr_bm25_info")
        return tuple(int(x) for x in out)

    def add_kernel_ms(self) -> float:
        """Device time of the last add's merge kernel in ms (-1 before the first add)."""
        ms = C.c_double(-1.0)
        _check(load().amdr_bm25_add_kernel_ms(self._h, C.byref(ms)), "amdr_bm25_add_kernel_ms")
        return float(ms.value)

    def read(self):
        """The resident arrays, copied to the host: (term_ptr, post_doc, post_tf, post_w, idf, doc_len)."""
        n, V, nnz = self.info()[:3]
        out = (np.empty(V + 1, np.int64), np.empty(nnz, np.int32), np.empty(nnz, np.int32), np.empty(nnz, np.float64),
               np.empty(V, np.float64), np.empty(n, np.int32))
        _check(load().amdr_bm25_read(self._h, _p(out[0], C.c_int64), _p(out[1], C.c_int32), _p(out[2], C.c_int32),
                                     _p(out[3], C.c_double), _p(out[4], C.c_double), _p(out[5], C.c_int32)),
               "amdr_bm25_read")
        return out

    @staticmethod
    def pack_queries(queries: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
        q_ptr = np.zeros(len(queries) + 1, dtype=np.int64)
        for i, q in enumerate(queries):
            q_ptr[i + 1] = q_ptr[i] + len(q)
        q_terms = np.empty(max(int(q_ptr[-1]), 1), dtype=np.int32)
        for i, q in enumerate(queries):
            q_terms[q_ptr[i]:q_ptr[i + 1]] = np.asarray(q, dtype=np.int32).reshape(-1)
        return q_terms, q_ptr

    def reserve(self, nq_max: int, k_max: int, total_terms_max: int) -> None:
        _check(load().amdr_bm25_reserve(self._h, C.c_int32(nq_max), C.c_int32(k_max), C.c_int64(total_terms_max)),
               "amdr_bm25_reserve")

    def search(self, queries: Sequence[Sequence[int]], k: int) -> Tuple[np.ndarray, np.ndarray]:
        q_terms, q_ptr = self.pack_queries(queries)
        nq = len(queries)
        scores = np.empty((nq, k), dtype=np.float64)
        ids = np.empty((nq, k), dtype=np.int64)
        _check(load().amdr_bm25_search(self._h, _p(q_terms, C.c_int32), _p(q_ptr, C.c_int64), C.c_int32(nq),
                                       C.c_int32(k), _p(scores, C.c_double), _p(ids, C.c_int64)), "amdr_bm25_search")
        return scores, ids

    def plan_info(self, nq: int, k: int) -> str:
        """Which kernels a search of nq queries at depth k would launch, and the slabs (no device work)."""
        return self._plan_info("amdr_bm25_plan_info", nq, k)

    def search_device(self, q_terms_ptr: int, q_ptr_ptr: int, nq: int, k: int, scores_ptr: int, ids_ptr: int,
                      stream: int = 0) -> None:
        _check(load().amdr_bm25_search_device(self._h, _vp(q_terms_ptr), _vp(q_ptr_ptr), C.c_int32(nq), C.c_int32(k),
                                              _vp(scores_ptr), _vp(ids_ptr), _vp(stream)), "amdr_bm25_search_device")

    # -- term constraints -> scope table (amdr_term_scope, csrc/term_scope.hip) ---------------------------------------
    # operands, in the ABI's order: (grp_ptr i64, grp_kind i32, grp_term_ptr i64, grp_terms i32, base_ptr i64,
    # base_rows i64, cons_base i32); retrieval/terms.py pack() makes them
    TERM_OPS = (np.int64, np.int32, np.int64, np.int32, np.int64, np.int64, np.int32)

    def term_scope(self, ops, cand_max: int, rows_cap: int, lists=None):
        """The host twin: (scope_ptr i64 [n_cons + 1], rows i64 [scope_ptr[-1]], status i32 [n_cons]) of the constraints
        `ops` — validated, staged, resolved on the handle's own stream.  status: 0, 1 (driver longer than cand_max: scope
        empty), 2 (rows beyond rows_cap dropped).  lists = (x_ptr i64 [n_x + 1], x_doc i32): the virtual posting lists of
        the call (amdr_term_scope_lists; term id n_terms + p names list p) — what phrase_lists returns."""
        a = [_c(x, t).ravel() for x, t in zip(ops, self.TERM_OPS)]
        n_cons, n_groups, n_base = a[6].size, a[1].size, max(a[4].size - 1, 0)
        if a[0].size != n_cons + 1 or a[2].size != n_groups + 1:
            raise ValueError("term_scope: grp_ptr [n_cons + 1], grp_term_ptr [n_groups + 1]")
        sp = np.zeros(n_cons + 1, dtype=np.int64)
        rows = np.full(max(int(rows_cap), 1), -1, dtype=np.int64)
        status = np.zeros(max(n_cons, 1), dtype=np.int32)
        op_ptrs = [_p(x, C.c_int64 if t is np.int64 else C.c_int32) for x, t in zip(a, self.TERM_OPS)]
        tail = (C.c_int64(n_base), C.c_int64(n_cons), C.c_int64(n_groups), C.c_int64(cand_max), C.c_int64(rows_cap),
                _p(sp, C.c_int64), _p(rows, C.c_int64), _p(status, C.c_int32))
        if lists is None:
            _check(load().amdr_term_scope(self._h, *op_ptrs, *tail), "amdr_term_scope")
        else:
            x_ptr, x_doc = _c(lists[0], np.int64).ravel(), _c(lists[1], np.int32).ravel()
            if x_ptr.size < 1:
                raise ValueError("term_scope: x_ptr [n_x + 1]")
            x_doc_arg = x_doc if x_doc.size else np.zeros(1, dtype=np.int32)
            _check(load().amdr_term_scope_lists(self._h, *op_ptrs, _p(x_ptr, C.c_int64), _p(x_doc_arg, C.c_int32),
                                                C.c_int64(x_ptr.size - 1), *tail), "amdr_term_scope_lists")
        return sp, rows[:int(sp[-1])], status[:n_cons]

    def term_scope_device(self, op_ptrs: Sequence[int], n_base: int, n_cons: int, n_groups: int, cand_max: int, rows_cap: int,
                          scope_ptr_ptr: int, rows_ptr: int, status_ptr: int, work_ptr: int, work_bytes: int,
                          stream: int = 0, lists=None) -> None:
        """The "_device" form: the seven operand arrays and the outputs as device pointers; enqueues only.
        lists = (x_ptr device pointer, x_doc device pointer, n_x): the virtual posting lists (amdr_term_scope_lists_device),
        the outputs of phrase_lists_device enqueued before on the same stream."""
        tail = (C.c_int64(n_base), C.c_int64(n_cons), C.c_int64(n_groups), C.c_int64(cand_max), C.c_int64(rows_cap),
                _vp(scope_ptr_ptr), _vp(rows_ptr), _vp(status_ptr), _vp(work_ptr), C.c_int64(work_bytes), _vp(stream))
        if lists is None:
            _check(load().amdr_term_scope_device(self._h, *(_vp(x) for x in op_ptrs), *tail), "amdr_term_scope_device")
        else:
            _check(load().amdr_term_scope_lists_device(self._h, *(_vp(x) for x in op_ptrs), _vp(lists[0]), _vp(lists[1]),
                                                       C.c_int64(lists[2]), *tail), "amdr_term_scope_lists_device")

    # -- the token stream and phrases -> virtual posting lists (amdr_phrase_lists, csrc/phrase_scope.hip) -------------
    def set_tokens(self, doc_ptr, tokens) -> None:
        """The token stream of the corpus (amdr_bm25_set_tokens): document d's text as the term ids
        tokens[doc_ptr[d] : doc_ptr[d + 1]], checked against the resident doc_len.  add / remove / replace drop it."""
        dp, tk = _c(doc_ptr, np.int64).ravel(), _c(tokens, np.int32).ravel()
        if dp.size != self.n_docs + 1 or (dp.size and tk.size < int(dp[-1])):
            raise ValueError("set_tokens: doc_ptr [n_docs + 1], tokens [doc_ptr[-1]]")
        tk_arg = tk if tk.size else np.zeros(1, dtype=np.int32)
        _check(load().amdr_bm25_set_tokens(self._h, _p(dp, C.c_int64), _p(tk_arg, C.c_int32)), "amdr_bm25_set_tokens")

    def tokens_info(self) -> Tuple[bool, int]:
        """(whether a token stream is resident, its token count)."""
        out = (C.c_int64 * 2)()
        _check(load().amdr_bm25_tokens_info(self._h, out), "amdr_bm25_tokens_info")
        return bool(out[0]), int(out[1])

    def read_tokens(self):
        """The resident token stream, copied to the host: (doc_ptr i64 [n_docs + 1], tokens i32)."""
        n_tok = self.tokens_info()[1]
        dp, tk = np.empty(self.info()[0] + 1, np.int64), np.empty(n_tok, np.int32)
        _check(load().amdr_bm25_read_tokens(self._h, _p(dp, C.c_int64), _p(tk, C.c_int32) if n_tok else None),
               "amdr_bm25_read_tokens")
        return dp, tk

    def token_doc_ptr(self) -> np.ndarray:
        """doc_ptr i64 [n_docs + 1] of the resident token stream alone (amdr_bm25_read_tokens with a null token array)."""
        dp = np.empty(self.info()[0] + 1, np.int64)
        _check(load().amdr_bm25_read_tokens(self._h, _p(dp, C.c_int64), None), "amdr_bm25_read_tokens")
        return dp

    def phrase_lists(self, phr_ptr, phr_terms, cand_max: int, rows_cap: int):
        """The host twin: (list_ptr i64 [n_phr + 1], docs i32 [list_ptr[-1]], status i32 [n_phr]) of the phrases
        phr_terms[phr_ptr[p] : phr_ptr[p + 1]] — each list the ascending documents that hold the phrase.  status as
        term_scope."""
        pp, pt = _c(phr_ptr, np.int64).ravel(), _c(phr_terms, np.int32).ravel()
        if pp.size < 1:
            raise ValueError("phrase_lists: phr_ptr [n_phr + 1]")
        n_phr = pp.size - 1
        lp = np.zeros(n_phr + 1, dtype=np.int64)
        docs = np.full(max(int(rows_cap), 1), -1, dtype=np.int32)
        status = np.zeros(max(n_phr, 1), dtype=np.int32)
        pt_arg = pt if pt.size else np.zeros(1, dtype=np.int32)
        _check(load().amdr_phrase_lists(self._h, _p(pp, C.c_int64), _p(pt_arg, C.c_int32), C.c_int64(n_phr),
                                        C.c_int64(cand_max), C.c_int64(rows_cap), _p(lp, C.c_int64), _p(docs, C.c_int32),
                                        _p(status, C.c_int32)), "amdr_phrase_lists")
        return lp, docs[:int(lp[-1])], status[:n_phr]

    def phrase_lists_device(self, phr_ptr_ptr: int, phr_terms_ptr: int, n_phr: int, cand_max: int, rows_cap: int,
                            list_ptr_ptr: int, docs_ptr: int, status_ptr: int, work_ptr: int, work_bytes: int,
                            stream: int = 0) -> None:
        """The "_device" form: operands and outputs as device pointers; enqueues only."""
        _check(load().amdr_phrase_lists_device(self._h, _vp(phr_ptr_ptr), _vp(phr_terms_ptr), C.c_int64(n_phr),
                                               C.c_int64(cand_max), C.c_int64(rows_cap), _vp(list_ptr_ptr), _vp(docs_ptr),
                                               _vp(status_ptr), _vp(work_ptr), C.c_int64(work_bytes), _vp(stream)),
               "amdr_phrase_lists_device")

    # -- phrases and Nears side by side -> one array of virtual posting lists (amdr_span_lists) -----------------------
    def span_lists(self, item_ptr, item_terms, item_kind, item_dist, cand_max: int, rows_cap: int):
        """The host twin: (list_ptr i64 [n + 1], docs i32 [list_ptr[-1]], status i32 [n]) of the items
        item_terms[item_ptr[p] : item_ptr[p + 1]] of kind item_kind[p] (0 phrase, 1 Near unordered, 2 Near ordered) and
        distance item_dist[p] — each list the ascending documents that hold the item.  status as term_scope."""
        pp, pt = _c(item_ptr, np.int64).ravel(), _c(item_terms, np.int32).ravel()
        kd, ds = _c(item_kind, np.int32).ravel(), _c(item_dist, np.int32).ravel()
        if pp.size < 1 or kd.size != pp.size - 1 or ds.size != pp.size - 1:
            raise ValueError("span_lists: item_ptr [n + 1], item_kind [n], item_dist [n]")
        n = pp.size - 1
        lp = np.zeros(n + 1, dtype=np.int64)
        docs = np.full(max(int(rows_cap), 1), -1, dtype=np.int32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        pad = np.zeros(1, dtype=np.int32)
        _check(load().amdr_span_lists(self._h, _p(pp, C.c_int64), _p(pt if pt.size else pad, C.c_int32),
                                      _p(kd if n else pad, C.c_int32), _p(ds if n else pad, C.c_int32), C.c_int64(n),
                                      C.c_int64(cand_max), C.c_int64(rows_cap), _p(lp, C.c_int64), _p(docs, C.c_int32),
                                      _p(status, C.c_int32)), "amdr_span_lists")
        return lp, docs[:int(lp[-1])], status[:n]

    def span_lists_device(self, item_ptr_ptr: int, item_terms_ptr: int, item_kind_ptr: int, item_dist_ptr: int, n_items: int,
                          cand_max: int, rows_cap: int, list_ptr_ptr: int, docs_ptr: int, status_ptr: int, work_ptr: int,
                          work_bytes: int, stream: int = 0) -> None:
        """The "_device" form: operands and outputs as device pointers; enqueues only."""
        _check(load().amdr_span_lists_device(self._h, _vp(item_ptr_ptr), _vp(item_terms_ptr), _vp(item_kind_ptr),
                                             _vp(item_dist_ptr), C.c_int64(n_items), C.c_int64(cand_max), C.c_int64(rows_cap),
                                             _vp(list_ptr_ptr), _vp(docs_ptr), _vp(status_ptr), _vp(work_ptr),
                                             C.c_int64(work_bytes), _vp(stream)), "amdr_span_lists_device")

    # -- unions of posting lists -> virtual posting lists (amdr_union_lists, csrc/union_lists.hip) ---------------------
    def union_lists(self, item_ptr, item_terms, rows_cap: int):
        """The host twin: (list_ptr i64 [n + 1], docs i32 [list_ptr[-1]], status i32 [n]) of the union items
        item_terms[item_ptr[p] : item_ptr[p + 1]] — each list the ascending documents that have a posting for at least one
        of the item's term ids.  status: 0, or 2 (documents beyond rows_cap dropped).  Needs no token stream."""
        pp, pt = _c(item_ptr, np.int64).ravel(), _c(item_terms, np.int32).ravel()
        if pp.size < 1:
            raise ValueError("union_lists: item_ptr [n + 1]")
        n = pp.size - 1
        lp = np.zeros(n + 1, dtype=np.int64)
        docs = np.full(max(int(rows_cap), 1), -1, dtype=np.int32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        pt_arg = pt if pt.size else np.zeros(1, dtype=np.int32)
        _check(load().amdr_union_lists(self._h, _p(pp, C.c_int64), _p(pt_arg, C.c_int32), C.c_int64(n), C.c_int64(rows_cap),
                                       _p(lp, C.c_int64), _p(docs, C.c_int32), _p(status, C.c_int32)), "amdr_union_lists")
        return lp, docs[:int(lp[-1])], status[:n]

    def union_lists_device(self, item_ptr_ptr: int, item_terms_ptr: int, n_items: int, n_before: int, rows_cap: int,
                           list_ptr_ptr: int, docs_ptr: int, status_ptr: int, work_ptr: int, work_bytes: int,
                           stream: int = 0) -> None:
        """The "_device" form: operands and outputs as device pointers; enqueues only.  Continues the list array whose
        first n_before + 1 entries of list_ptr were written earlier on the same stream (n_before = 0: starts one);
        rows_cap is the capacity of the whole docs array."""
        _check(load().amdr_union_lists_device(self._h, _vp(item_ptr_ptr), _vp(item_terms_ptr), C.c_int64(n_items),
                                              C.c_int64(n_before), C.c_int64(rows_cap), _vp(list_ptr_ptr), _vp(docs_ptr),
                                              _vp(status_ptr), _vp(work_ptr), C.c_int64(work_bytes), _vp(stream)),
               "amdr_union_lists_device")

    # -- class spans: a Prefix or a OneOf inside a phrase or a Near (amdr_class_spans, csrc/class_span.hip) ---------------
    def class_spans(self, item_ptr, item_slots, item_kind, item_dist, cls_ptr, cls_terms, cand_max: int, rows_cap: int):
        """The host twin: (list_ptr i64 [n + 1], docs i32 [list_ptr[-1]], status i32 [n]) of the items
        item_slots[item_ptr[p] : item_ptr[p + 1]] of kind item_kind[p] and distance item_dist[p] (as span_lists) whose slot
        ids are plain term ids or n_terms + c for class c, the strictly ascending member ids
        cls_terms[cls_ptr[c] : cls_ptr[c + 1]].  Runs the union step for the classes and then the class step; returns only
        the items' lists.  status as term_scope."""
        pp, pt = _c(item_ptr, np.int64).ravel(), _c(item_slots, np.int32).ravel()
        kd, ds = _c(item_kind, np.int32).ravel(), _c(item_dist, np.int32).ravel()
        cp, ct = _c(cls_ptr, np.int64).ravel(), _c(cls_terms, np.int32).ravel()
        if pp.size < 1 or kd.size != pp.size - 1 or ds.size != pp.size - 1 or cp.size < 1:
            raise ValueError("class_spans: item_ptr [n + 1], item_kind [n], item_dist [n], cls_ptr [n_cls + 1]")
        n, n_cls = pp.size - 1, cp.size - 1
        lp = np.zeros(n + 1, dtype=np.int64)
        docs = np.full(max(int(rows_cap), 1), -1, dtype=np.int32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        pad = np.zeros(1, dtype=np.int32)
        _check(load().amdr_class_spans(self._h, _p(pp, C.c_int64), _p(pt if pt.size else pad, C.c_int32),
                                       _p(kd if n else pad, C.c_int32), _p(ds if n else pad, C.c_int32), C.c_int64(n),
                                       _p(cp, C.c_int64), _p(ct if ct.size else pad, C.c_int32), C.c_int64(n_cls),
                                       C.c_int64(cand_max), C.c_int64(rows_cap), _p(lp, C.c_int64), _p(docs, C.c_int32),
                                       _p(status, C.c_int32)), "amdr_class_spans")
        return lp, docs[:int(lp[-1])], status[:n]

    def class_spans_device(self, item_ptr_ptr: int, item_slots_ptr: int, item_kind_ptr: int, item_dist_ptr: int, n_items: int,
                           cls_ptr_ptr: int, cls_terms_ptr: int, n_cls: int, cls_first: int, n_before: int, cand_max: int,
                           rows_cap: int, list_ptr_ptr: int, docs_ptr: int, status_ptr: int, work_ptr: int, work_bytes: int,
                           stream: int = 0) -> None:
        """The "_device" form: operands and outputs as device pointers; enqueues only.  Continues the list array whose
        first n_before + 1 entries of list_ptr were written earlier on the same stream; class c is the slot id
        n_terms + cls_first + c and its documents are list cls_first + c of that array (cls_first + n_cls <= n_before);
        rows_cap is the capacity of the whole docs array."""
        _check(load().amdr_class_spans_device(self._h, _vp(item_ptr_ptr), _vp(item_slots_ptr), _vp(item_kind_ptr),
                                              _vp(item_dist_ptr), C.c_int64(n_items), _vp(cls_ptr_ptr), _vp(cls_terms_ptr),
                                              C.c_int64(n_cls), C.c_int64(cls_first), C.c_int64(n_before), C.c_int64(cand_max),
                                              C.c_int64(rows_cap), _vp(list_ptr_ptr), _vp(docs_ptr), _vp(status_ptr),
                                              _vp(work_ptr), C.c_int64(work_bytes), _vp(stream)), "amdr_class_spans_device")

    # -- unit spans: same sentence, same paragraph (amdr_unit_spans, csrc/unit_span.hip) ---------------------------------
    def set_breaks(self, breaks) -> None:
        """The break flags beside the resident token stream (amdr_bm25_set_breaks): one byte per token, 1 a sentence start, 3
        a paragraph start, 0 neither.  set_tokens and every update drop them."""
        bk = _c(breaks, np.uint8).ravel()
        arg = bk if bk.size else np.zeros(1, dtype=np.uint8)
        _check(load().amdr_bm25_set_breaks(self._h, _p(arg, C.c_uint8), C.c_int64(bk.size)), "amdr_bm25_set_breaks")

    def breaks_info(self) -> Tuple[bool, int]:
        """(whether break flags are resident, their count)."""
        out = (C.c_int64 * 2)()
        _check(load().amdr_bm25_breaks_info(self._h, out), "amdr_bm25_breaks_info")
        return bool(out[0]), int(out[1])

    def read_breaks(self) -> np.ndarray:
        """The resident break flags, copied to the host: u8 [n_tokens]."""
        n = self.breaks_info()[1]
        bk = np.empty(max(n, 1), np.uint8)
        _check(load().amdr_bm25_read_breaks(self._h, _p(bk, C.c_uint8)), "amdr_bm25_read_breaks")
        return bk[:n]

    def unit_spans(self, item_ptr, item_slots, item_kind, cls_ptr, cls_terms, cand_max: int, rows_cap: int):
        """The host twin: (list_ptr i64 [n + 1], docs i32 [list_ptr[-1]], status i32 [n]) of the unit items
        item_slots[item_ptr[p] : item_ptr[p + 1]] of kind item_kind[p] (bit 0 ordered, bit 1 paragraph) whose slot ids are
        plain term ids or n_terms + c for class c, as class_spans takes them.  Runs the union step for the classes and then
        the unit step; returns only the items' lists.  status as term_scope."""
        pp, pt = _c(item_ptr, np.int64).ravel(), _c(item_slots, np.int32).ravel()
        kd = _c(item_kind, np.int32).ravel()
        cp, ct = _c(cls_ptr, np.int64).ravel(), _c(cls_terms, np.int32).ravel()
        if pp.size < 1 or kd.size != pp.size - 1 or cp.size < 1:
            raise ValueError("unit_spans: item_ptr [n + 1], item_kind [n], cls_ptr [n_cls + 1]")
        n, n_cls = pp.size - 1, cp.size - 1
        lp = np.zeros(n + 1, dtype=np.int64)
        docs = np.full(max(int(rows_cap), 1), -1, dtype=np.int32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        pad = np.zeros(1, dtype=np.int32)
        _check(load().amdr_unit_spans(self._h, _p(pp, C.c_int64), _p(pt if pt.size else pad, C.c_int32),
                                      _p(kd if n else pad, C.c_int32), C.c_int64(n), _p(cp, C.c_int64),
                                      _p(ct if ct.size else pad, C.c_int32), C.c_int64(n_cls), C.c_int64(cand_max),
                                      C.c_int64(rows_cap), _p(lp, C.c_int64), _p(docs, C.c_int32), _p(status, C.c_int32)),
               "amdr_unit_spans")
        return lp, docs[:int(lp[-1])], status[:n]

    def unit_spans_device(self, item_ptr_ptr: int, item_slots_ptr: int, item_kind_ptr: int, n_items: int, cls_ptr_ptr: int,
                          cls_terms_ptr: int, n_cls: int, cls_first: int, n_before: int, cand_max: int, rows_cap: int,
                          list_ptr_ptr: int, docs_ptr: int, status_ptr: int, work_ptr: int, work_bytes: int,
                          stream: int = 0) -> None:
        """The "_device" form, as class_spans_device without the distances; needs the break flags (set_breaks)."""
        _check(load().amdr_unit_spans_device(self._h, _vp(item_ptr_ptr), _vp(item_slots_ptr), _vp(item_kind_ptr),
                                             C.c_int64(n_items), _vp(cls_ptr_ptr), _vp(cls_terms_ptr), C.c_int64(n_cls),
                                             C.c_int64(cls_first), C.c_int64(n_before), C.c_int64(cand_max),
                                             C.c_int64(rows_cap), _vp(list_ptr_ptr), _vp(docs_ptr), _vp(status_ptr),
                                             _vp(work_ptr), C.c_int64(work_bytes), _vp(stream)), "amdr_unit_spans_device")

    # -- marks and best passages of the hit documents (amdr_bm25_marks, csrc/marks.hip) ---------------------------------
    def marks(self, docs, mk_ptr, mk_terms, mk_slot, slot_w, slot_loose, sq_ptr, sq_off, sq_slots, window: int,
              marks_cap: int):
        """The host twin: for the hit ids docs i64 [nq, k] (-1: no hit) and per query a mark table
        (mk_terms[mk_ptr[q] : mk_ptr[q + 1]] strictly ascending, mk_slot parallel, slots 0 .. 31), weights slot_w f64 [nq, 32],
        loose slots slot_loose u32 [nq] and sequences (sq_ptr [nq + 1] into sq_off [n_seq + 1] into sq_slots) ->
        (win i32 [nq, k, 4]: start, end, marks in the window, marks in the document; score f64 [nq, k]; slots u32 [nq, k, 2];
        marks i32 [nq, k, marks_cap, 2]: (position, slot) or (-1, -1); status i32 [nq, k]).  csrc/marks_rule.hpp is the rule."""
        d = _c(docs, np.int64)
        if d.ndim != 2:
            raise ValueError("marks: docs [nq, k]")
        nq, k = d.shape
        mp, mt, ms = _c(mk_ptr, np.int64).ravel(), _c(mk_terms, np.int32).ravel(), _c(mk_slot, np.int32).ravel()
        sw, sl = _c(slot_w, np.float64).reshape(-1), _c(slot_loose, np.uint32).ravel()
        sp, so, ss = _c(sq_ptr, np.int64).ravel(), _c(sq_off, np.int64).ravel(), _c(sq_slots, np.int32).ravel()
        if mp.size != nq + 1 or sp.size != nq + 1 or sw.size != nq * 32 or sl.size != nq or so.size < 1 or ms.size != mt.size:
            raise ValueError("marks: mk_ptr [nq + 1], sq_ptr [nq + 1], slot_w [nq, 32], slot_loose [nq], sq_off [n_seq + 1]")
        if (mp.size and mt.size < int(mp[-1])) or (sp.size and so.size < int(sp[-1]) + 1) or ss.size < int(so[-1]):
            raise ValueError("marks: an array shorter than its pointers say")
        cap = int(marks_cap)
        win = np.zeros((nq, k, 4), np.int32)
        score = np.zeros((nq, k), np.float64)
        slots = np.zeros((nq, k, 2), np.uint32)
        marks = np.full((nq, k, max(cap, 0), 2), -1, np.int32)
        status = np.zeros((nq, k), np.int32)
        pad, padw, padu = np.zeros(1, np.int32), np.zeros(1, np.float64), np.zeros(1, np.uint32)
        full = lambda a, z: a if a.size else z  # noqa: E731
        _check(load().amdr_bm25_marks(self._h, _p(full(d, np.zeros(1, np.int64)), C.c_int64), C.c_int64(nq), C.c_int64(k),
                                      C.c_int64(k), _p(mp, C.c_int64), _p(full(mt, pad), C.c_int32), _p(full(ms, pad), C.c_int32),
                                      _p(full(sw, padw), C.c_double), _p(full(sl, padu), C.c_uint32), _p(sp, C.c_int64),
                                      _p(so, C.c_int64), _p(full(ss, pad), C.c_int32), C.c_int32(window), C.c_int32(cap),
                                      _p(full(win, pad), C.c_int32), _p(full(score, padw), C.c_double),
                                      _p(full(slots, padu), C.c_uint32), _p(full(marks, pad), C.c_int32),
                                      _p(full(status, pad), C.c_int32)), "amdr_bm25_marks")
        return win, score, slots, marks, status

    def marks_device(self, docs_ptr: int, nq: int, k: int, ld_docs: int, mk_ptr_ptr: int, mk_terms_ptr: int, mk_slot_ptr: int,
                     slot_w_ptr: int, slot_loose_ptr: int, sq_ptr_ptr: int, sq_off_ptr: int, sq_slots_ptr: int, window: int,
                     marks_cap: int, win_ptr: int, score_ptr: int, slots_ptr: int, marks_ptr: int, status_ptr: int,
                     stream: int = 0) -> None:
        """The "_device" form: operands and outputs as device pointers; enqueues one launch and allocates nothing.  Any hit
        id outside [0, n_docs) is no hit."""
        _check(load().amdr_bm25_marks_device(self._h, _vp(docs_ptr), C.c_int64(nq), C.c_int64(k), C.c_int64(ld_docs),
                                             _vp(mk_ptr_ptr), _vp(mk_terms_ptr), _vp(mk_slot_ptr), _vp(slot_w_ptr),
                                             _vp(slot_loose_ptr), _vp(sq_ptr_ptr), _vp(sq_off_ptr), _vp(sq_slots_ptr),
                                             C.c_int32(window), C.c_int32(marks_cap), _vp(win_ptr), _vp(score_ptr),
                                             _vp(slots_ptr), _vp(marks_ptr), _vp(status_ptr), _vp(stream)),
               "amdr_bm25_marks_device")

    def marks_kernel_ms(self) -> float:
        """Device time of the kernel of the last marks() call, in ms; -1.0 when there is none."""
        ms = C.c_double(0.0)
        _check(load().amdr_bm25_marks_kernel_ms(self._h, C.byref(ms)), "amdr_bm25_marks_kernel_ms")
        return float(ms.value)

    def get_scores(self, queries: Sequence[Sequence[int]]) -> np.ndarray:
        q_terms, q_ptr = self.pack_queries(queries)
        nq = len(queries)
        out = np.empty((nq, self.n_docs), dtype=np.float64)
        _check(load().amdr_bm25_scores(self._h, _p(q_terms, C.c_int32), _p(q_ptr, C.c_int64), C.c_int32(nq),
                                       _p(out, C.c_double)), "amdr_bm25_scores")
        return out


# ---------------------------------------------------------------------------
class Tokenizer(_Handle):
    """Batched native query tokeniser + vocabulary lookup (include/amdretrieval.h, csrc/tokenize.cpp): the jieba.cut
    rule for text without Han characters, then term ids — one call per batch, GIL released.
    han: what a query holding a Han character gets (amdr_tokenizer_set_han) — "flag" (the default: needs_segmenter, no
    terms), "char" (text.jieba_cut_restated: one Han character per token) or a text.HanDict (text.dict_cut over it)."""
    _destroy = "amdr_tokenizer_destroy"
    HAN_MODES = {"flag": 0, "char": 1, "dict": 2}

    def __init__(self, vocab: Sequence[str], han="flag"):
        enc = [w.encode("utf-8") for w in vocab]
        blob = b"".join(enc)
        offs = np.zeros(len(enc) + 1, dtype=np.int64)
        np.cumsum([len(e) for e in enc], out=offs[1:])
        self._h = C.c_void_p()
        _check(load().amdr_tokenizer_create(C.c_char_p(blob), _p(offs, C.c_int64), C.c_int64(len(enc)), C.byref(self._h)),
               "amdr_tokenizer_create")
        self.han = "flag"
        if isinstance(han, str):
            if han not in ("flag", "char"):
                raise ValueError(f"Tokenizer: han must be 'flag', 'char' or a text.HanDict, got {han!r}")
            if han == "char":
                self.set_han(1)
                self.han = "char"
        else:
            keys, logw, word, unknown = han.native_tables()
            self.set_han(2, keys, logw, word, unknown)
            self.han = "dict"

    def set_han(self, mode: int, keys: Sequence[str] = (), logw=None, is_word=None, logw_unknown: float = 0.0) -> None:
        """amdr_tokenizer_set_han as it is (before any encode and before a DeviceTokenizer is made of this handle)."""
        enc = [k.encode("utf-8") for k in keys]
        blob = b"".join(enc)
        offs = np.zeros(len(enc) + 1, dtype=np.int64)
        np.cumsum([len(e) for e in enc], out=offs[1:])
        logw = np.ascontiguousarray(logw if logw is not None else np.zeros(len(enc)), dtype=np.float64)
        word = np.ascontiguousarray(is_word if is_word is not None else np.zeros(len(enc)), dtype=np.uint8)
        if logw.shape != (len(enc),) or word.shape != (len(enc),):
            raise ValueError("set_han: logw and is_word take one entry per key")
        _check(load().amdr_tokenizer_set_han(self._h, C.c_int32(mode), C.c_char_p(blob), _p(offs, C.c_int64),
                                             _p(logw, C.c_double), _p(word, C.c_uint8), C.c_int64(len(enc)),
                                             C.c_double(logw_unknown)), "amdr_tokenizer_set_han")

    @property
    def han_mode(self) -> int:
        m = C.c_int32(-1)
        _check(load().amdr_tokenizer_han_mode(self._h, C.byref(m)), "amdr_tokenizer_han_mode")
        return int(m.value)

    def cut_han(self, text: str) -> Optional[list]:
        """Token strings of one text under this handle's Han mode (None: Han text in the "flag" mode)."""
        b = text.encode("utf-8")
        cap = max(len(b), 1)
        st, en = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)
        n = C.c_int32(0)
        _check(load().amdr_tokenizer_spans_han(self._h, C.c_char_p(b), C.c_int64(len(b)), _p(st, C.c_int32),
                                               _p(en, C.c_int32), C.c_int32(cap), C.byref(n)), "amdr_tokenizer_spans_han")
        if n.value < 0:
            return None
        return [b[int(a):int(e)].decode("utf-8") for a, e in zip(st[: n.value], en[: n.value])]

    def encode(self, texts: Sequence[str]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(term_ids i32 [total], q_ptr i64 [n+1], needs_segmenter bool [n]) — the CSR BM25Index.search takes.
        Queries flagged needs_segmenter hold a Han character and got NO terms here (han="flag" only).  The batch crosses into native code
        as ONE blob: the queries joined by NUL bytes and encoded once (two C-level operations however long the batch);
        a batch that itself contains a NUL takes the per-query offsets form."""
        n = len(texts)
        if n == 0:
            return np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, bool)
        views = _pystrings()
        if views is not None:
            # zero-copy: the UTF-8 bytes where CPython keeps them (csrc/pystrings.c), pointers + lengths to the native call
            ptrs, lens = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
            cap = max(int(views.utf8_views(texts, ptrs.ctypes.data, lens.ctypes.data)), 1)
            terms = np.empty(cap, dtype=np.int32)
            q_ptr = np.empty(n + 1, dtype=np.int64)
            flags = np.empty(n, dtype=np.int32)
            _check(load().amdr_tokenizer_encode_ptrs(self._h, ptrs.ctypes.data, lens.ctypes.data, n, terms.ctypes.data, cap,
                                                     q_ptr.ctypes.data, flags.ctypes.data), "amdr_tokenizer_encode_ptrs")
            return terms[: int(q_ptr[-1])], q_ptr, flags.astype(bool)
        blob = "\0".join(t or "" for t in texts).encode("utf-8")
        cap = max(len(blob), 1)
        terms = np.empty(cap, dtype=np.int32)
        q_ptr = np.zeros(n + 1, dtype=np.int64)
        flags = np.zeros(n, dtype=np.int32)
        if blob.count(b"\0") == n - 1:
            _check(load().amdr_tokenizer_encode_joined(self._h, blob, len(blob), n, _p(terms, C.c_int32), cap,
                                                       _p(q_ptr, C.c_int64), _p(flags, C.c_int32)),
                   "amdr_tokenizer_encode_joined")
        else:
            enc = [t.encode("utf-8") for t in texts]
            blob = b"".join(enc)
            offs = np.zeros(n + 1, dtype=np.int64)
            np.cumsum([len(e) for e in enc], out=offs[1:])
            cap = max(len(blob), 1)
            terms = np.empty(cap, dtype=np.int32)
            _check(load().amdr_tokenizer_encode(self._h, C.c_char_p(blob), _p(offs, C.c_int64), C.c_int32(n),
                                                _p(terms, C.c_int32), C.c_int64(cap), _p(q_ptr, C.c_int64), _p(flags, C.c_int32)),
                   "amdr_tokenizer_encode")
        return terms[: int(q_ptr[-1])], q_ptr, flags.astype(bool)

    @staticmethod
    def cut(text: str) -> Optional[list]:
        """Token strings of one text by the native rule (None: Han text)."""
        b = text.encode("utf-8")
        cap = max(len(b), 1)
        st, en = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)
        n = C.c_int32(0)
        _check(load().amdr_tokenizer_spans(C.c_char_p(b), C.c_int64(len(b)), _p(st, C.c_int32), _p(en, C.c_int32),
                                           C.c_int32(cap), C.byref(n)), "amdr_tokenizer_spans")
        if n.value < 0:
            return None
        return [b[int(a):int(e)].decode("utf-8") for a, e in zip(st[: n.value], en[: n.value])]


class VocabIndex(_Handle):
    """A resident copy of a vocabulary (token i is term id i) that Wildcard and Fuzzy patterns are matched against on the
    device (amdr_vocab_*, csrc/vocab_match.hip).  Patterns cross as code points: pack_patterns."""
    _destroy = "amdr_vocab_destroy"

    def __init__(self, vocab: Sequence[str], *, device: int = 0):
        enc = [w.encode("utf-8") for w in vocab]
        blob = b"".join(enc)
        offs = np.zeros(len(enc) + 1, dtype=np.int64)
        np.cumsum([len(e) for e in enc], out=offs[1:])
        self._h = C.c_void_p()
        self.device = int(device)
        self.n_terms = len(enc)
        _check(load().amdr_vocab_create(C.c_char_p(blob), _p(offs, C.c_int64), C.c_int64(len(enc)), C.c_int32(device),
                                        C.byref(self._h)), "amdr_vocab_create")

    def info(self) -> Tuple[int, int]:
        """(n_terms, bytes of the blob)."""
        out = (C.c_int64 * 2)()
        _check(load().amdr_vocab_info(self._h, out), "amdr_vocab_info")
        return int(out[0]), int(out[1])

    @staticmethod
    def pack_patterns(patterns: Sequence[Tuple[int, int, Sequence[int]]]):
        """(pat_cp u32, pat_ptr i64 [n + 1], pat_kind i32, pat_arg i32) of (kind, arg, code points) triples."""
        ptr = np.zeros(len(patterns) + 1, dtype=np.int64)
        np.cumsum([len(p[2]) for p in patterns], out=ptr[1:])
        cp = np.fromiter((c for p in patterns for c in p[2]), dtype=np.uint32, count=int(ptr[-1]))
        return (cp, ptr, np.asarray([p[0] for p in patterns], dtype=np.int32), np.asarray([p[1] for p in patterns], dtype=np.int32))

    def match(self, pat_cp, pat_ptr, pat_kind, pat_arg, item_cap: int):
        """The host twin: (ids i32 [n, item_cap], dist u8 [n, item_cap], n_match i64 [n]) — per pattern the first item_cap
        term ids it names, ascending, then -1; their distances, then 255; the true count."""
        cp, ptr = _c(pat_cp, np.uint32).ravel(), _c(pat_ptr, np.int64).ravel()
        kind, arg = _c(pat_kind, np.int32).ravel(), _c(pat_arg, np.int32).ravel()
        if ptr.size < 1 or kind.size != ptr.size - 1 or arg.size != kind.size:
            raise ValueError("match: pat_ptr [n + 1], pat_kind [n], pat_arg [n]")
        n = ptr.size - 1
        rows = max(n, 1) * max(int(item_cap), 1)
        ids, dist = np.full(rows, -2, dtype=np.int32), np.full(rows, 254, dtype=np.uint8)
        n_match = np.zeros(max(n, 1), dtype=np.int64)
        pad = lambda a, dt: a if a.size else np.zeros(1, dtype=dt)  # noqa: E731
        _check(load().amdr_vocab_match(self._h, _p(pad(cp, np.uint32), C.c_uint32), _p(ptr, C.c_int64),
                                       _p(pad(kind, np.int32), C.c_int32), _p(pad(arg, np.int32), C.c_int32), C.c_int64(n),
                                       C.c_int64(cp.size), C.c_int32(item_cap), _p(ids, C.c_int32), _p(dist, C.c_uint8),
                                       _p(n_match, C.c_int64)), "amdr_vocab_match")
        return ids[:n * int(item_cap)].reshape(n, int(item_cap)), dist[:n * int(item_cap)].reshape(n, int(item_cap)), n_match[:n]

    def match_device(self, pat_cp_ptr: int, pat_ptr_ptr: int, pat_kind_ptr: int, pat_arg_ptr: int, n_pat: int, cp_total: int,
                     item_cap: int, ids_ptr: int, dist_ptr: int, n_match_ptr: int, work_ptr: int, work_bytes: int,
                     stream: int = 0) -> None:
        """The "_device" form: operands and outputs as device pointers; enqueues only, on the current device."""
        _check(load().amdr_vocab_match_device(self._h, _vp(pat_cp_ptr), _vp(pat_ptr_ptr), _vp(pat_kind_ptr), _vp(pat_arg_ptr),
                                              C.c_int64(n_pat), C.c_int64(cp_total), C.c_int32(item_cap), _vp(ids_ptr),
                                              _vp(dist_ptr), _vp(n_match_ptr), _vp(work_ptr), C.c_int64(work_bytes),
                                              _vp(stream)), "amdr_vocab_match_device")


def utf8_views(texts: Sequence[Optional[str]]):
    """(ptrs i64 [n], lens i64 [n], total bytes, maybe_han bool [n], keepalive) of a list of str: the UTF-8 bytes where
    CPython keeps them (csrc/pystrings.c; without that glue, one encode per text, held by `keepalive`).  maybe_han[i] is
    False where text i certainly holds no Han character (its storage kind cannot represent U+4E00 and above): an O(1)
    test per string, no scan.  `texts` (or keepalive) must stay alive while the pointers are used."""
    n = len(texts)
    ptrs, lens = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    wide = np.zeros(n, dtype=np.uint8)
    views = _pystrings()
    if views is not None:
        total = int(views.utf8_views(texts, ptrs.ctypes.data, lens.ctypes.data, wide.ctypes.data)) if n else 0
        return ptrs, lens, total, wide.astype(bool), None
    enc = [(t or "").encode("utf-8") for t in texts]
    for i, e in enumerate(enc):
        ptrs[i] = C.cast(C.c_char_p(e), C.c_void_p).value or 0
        lens[i] = len(e)
        wide[i] = any(ord(ch) >= 0x4E00 for ch in (texts[i] or ""))
    return ptrs, lens, int(lens.sum()), wide.astype(bool), enc


def pack_utf8(ptrs: np.ndarray, lens: np.ndarray, blob_addr: int, capacity: int, offs_addr: int) -> None:
    """The texts behind (ptrs, lens) back to back into the caller's buffer at blob_addr (capacity bytes), offsets
    [n + 1] at offs_addr (amdr_tokenizer_pack; GIL released, the copies on the tokeniser's worker pool)."""
    n = int(ptrs.shape[0])
    _check(load().amdr_tokenizer_pack(ptrs.ctypes.data, lens.ctypes.data, n, _vp(blob_addr), int(capacity), _vp(offs_addr)),
           "amdr_tokenizer_pack")


def pack_texts(texts: Sequence[Optional[str]]) -> Tuple[np.ndarray, np.ndarray]:
    """(blob u8 [total], offsets i64 [n + 1]): b"".join(t.encode() for t in texts) and its cumulative lengths, built by
    amdr_tokenizer_pack from the strings' own UTF-8 views."""
    ptrs, lens, total, _, keep = utf8_views(texts)
    blob = np.empty(max(total, 1), dtype=np.uint8)
    offs = np.empty(len(texts) + 1, dtype=np.int64)
    pack_utf8(ptrs, lens, blob.ctypes.data, blob.size, offs.ctypes.data)
    del keep
    return blob[:total], offs


class DeviceTokenizer(_Handle):
    """The batched query tokeniser on the device (amdr_tokenizer_*_device, csrc/tokenize.hip): a copy of a host
    Tokenizer's vocabulary in HBM; encode_device turns a UTF-8 blob + offsets already on the device into the term-id
    CSR amdr_bm25_search_device takes, byte for byte what Tokenizer.encode gives for the same bytes.  Enqueue only;
    capturable after reserve()."""
    _destroy = "amdr_tokenizer_device_destroy"

    def __init__(self, tok: "Tokenizer", *, device: int = 0):
        self.device = int(device)
        self._h = C.c_void_p()
        self._tok = tok  # the host table is copied at creation; kept for callers that want both forms
        _check(load().amdr_tokenizer_device_create(tok._h, C.c_int32(device), C.byref(self._h)),
               "amdr_tokenizer_device_create")
        self.nq_max, self.bytes_max = 0, -1

    def reserve(self, nq_max: int, bytes_max: int) -> None:
        _check(load().amdr_tokenizer_device_reserve(self._h, C.c_int32(nq_max), C.c_int64(bytes_max)),
               "amdr_tokenizer_device_reserve")
        self.nq_max, self.bytes_max = max(self.nq_max, int(nq_max)), max(self.bytes_max, int(bytes_max))

    def encode_device_ptrs(self, text: int, offs: int, nq: int, n_bytes: int, term_ids: int, capacity: int, q_ptr: int,
                           needs_segmenter: int, stream: int = 0) -> None:
        _check(load().amdr_tokenizer_encode_device(self._h, _vp(text), _vp(offs), C.c_int32(nq), C.c_int64(n_bytes),
                                                   _vp(term_ids), C.c_int64(capacity), _vp(q_ptr), _vp(needs_segmenter),
                                                   _vp(stream)), "amdr_tokenizer_encode_device")

    def encode_device(self, blob, offs, term_ids, q_ptr, needs_segmenter, *, nq: Optional[int] = None,
                      n_bytes: Optional[int] = None, stream: Optional[int] = None) -> None:
        """On torch device tensors: blob u8 [>= n_bytes], offs i64 [nq + 1] -> term_ids i32 [capacity = its length],
        q_ptr i64 [nq + 1], needs_segmenter i32 [nq].  nq / n_bytes default to the tensors' sizes; stream to torch's
        current stream."""
        import torch
        nq = int(offs.numel()) - 1 if nq is None else int(nq)
        n_bytes = int(blob.numel()) if n_bytes is None else int(n_bytes)
        for t in (blob, offs, term_ids, q_ptr, needs_segmenter):
            assert t.is_cuda and t.is_contiguous()
        assert offs.dtype == torch.int64 and term_ids.dtype == torch.int32 and q_ptr.dtype == torch.int64
        assert needs_segmenter.dtype == torch.int32 and blob.element_size() == 1
        if stream is None:
            stream = int(torch.cuda.current_stream(blob.device).cuda_stream)
        self.encode_device_ptrs(blob.data_ptr(), offs.data_ptr(), nq, n_bytes, term_ids.data_ptr(), int(term_ids.numel()),
                                q_ptr.data_ptr(), needs_segmenter.data_ptr(), stream)


class MaxSimIndex(_Handle):
    """Exhaustive ColBERT late interaction over fp32 token embeddings."""
    _destroy = "amdr_maxsim_destroy"

    def __init__(self, D: np.ndarray, doc_ptr: np.ndarray, *, device: int = 0):
        D = _c(D, np.float32)
        doc_ptr = _c(doc_ptr, np.int64)
        if D.ndim != 2:
            raise ValueError("D must be [tokens, dim]")
        self.dim = int(D.shape[1])
        self.n_docs = int(doc_ptr.shape[0] - 1)
        self.device = int(device)
        if int(doc_ptr[-1]) != D.shape[0]:
            raise ValueError("doc_ptr[-1] != number of token rows")
        self._h = C.c_void_p()
        _check(load().amdr_maxsim_create(_p(D, C.c_float), _p(doc_ptr, C.c_int64), C.c_int64(self.n_docs),
                                         C.c_int32(self.dim), C.c_int32(device), C.byref(self._h)),
               "amdr_maxsim_create")

    def add(self, D: np.ndarray, doc_ptr: np.ndarray) -> None:
        """Append documents (doc_ptr: their own offsets, from 0); new pids follow the store's.  The handle is then what
        MaxSimIndex makes of the concatenated store, bit for bit (amdr_maxsim_add)."""
        D = _c(D, np.float32)
        doc_ptr = _c(doc_ptr, np.int64)
        if D.ndim != 2 or D.shape[1] != self.dim:
            raise ValueError(f"add: D must be [tokens, {self.dim}]")
        if doc_ptr.ndim != 1 or doc_ptr.shape[0] < 1:
            raise ValueError("add: doc_ptr must be [n_add + 1]")
        if int(doc_ptr[-1]) != D.shape[0]:
            raise ValueError("doc_ptr[-1] != number of token rows")
        _check(load().amdr_maxsim_add(self._h, _p(D, C.c_float), _p(doc_ptr, C.c_int64), C.c_int64(doc_ptr.shape[0] - 1)),
               "amdr_maxsim_add")
        self.n_docs = self.info()[0]

    def remove(self, ids) -> None:
        """Remove documents (amdr_maxsim_remove): ids strictly ascending old pids (not all of them); the survivors are
        renumbered 0 .. n-1 in their old order and the handle is then what MaxSimIndex makes of the surviving store,
        bit for bit — its scale and first-pass bound can fall."""
        ids = _c(np.asarray(ids, dtype=np.int64).reshape(-1), np.int64)
        _check(load().amdr_maxsim_remove(self._h, _p(ids, C.c_int64), C.c_int64(ids.shape[0])), "amdr_maxsim_remove")
        self.n_docs = self.info()[0]

    def remove_kernel_ms(self) -> float:
        """Device time of the last remove's doc_ptr rebuild and compaction kernel, in ms (-1.0 before the first remove)."""
        ms = C.c_double(0)
        _check(load().amdr_maxsim_remove_kernel_ms(self._h, C.byref(ms)), "amdr_maxsim_remove_kernel_ms")
        return float(ms.value)

    def replace(self, ids, D: np.ndarray, doc_ptr: np.ndarray) -> None:
        """Replace documents under their pids (amdr_maxsim_replace): ids strictly ascending pids, document ids[i] takes
        the token rows D[doc_ptr[i]:doc_ptr[i + 1]] (doc_ptr: their own offsets, from 0).  No pid moves; the handle is then
        what MaxSimIndex makes of the edited store, bit for bit — its scale and first-pass bound can fall."""
        ids = _c(np.asarray(ids, dtype=np.int64).reshape(-1), np.int64)
        D = _c(D, np.float32)
        doc_ptr = _c(doc_ptr, np.int64)
        if D.ndim != 2 or D.shape[1] != self.dim:
            raise ValueError(f"replace: D must be [tokens, {self.dim}]")
        if doc_ptr.ndim != 1 or doc_ptr.shape[0] != ids.shape[0] + 1:
            raise ValueError("replace: doc_ptr must be [len(ids) + 1]")
        if int(doc_ptr[-1]) != D.shape[0]:
            raise ValueError("doc_ptr[-1] != number of token rows")
        _check(load().amdr_maxsim_replace(self._h, _p(ids, C.c_int64), _p(D, C.c_float), _p(doc_ptr, C.c_int64),
                                          C.c_int64(ids.shape[0])), "amdr_maxsim_replace")

    def replace_kernel_ms(self) -> float:
        """Device time of the last replace's doc_ptr rebuild and splice kernel, in ms (-1.0 before the first replace)."""
        ms = C.c_double(0)
        _check(load().amdr_maxsim_replace_kernel_ms(self._h, C.byref(ms)), "amdr_maxsim_replace_kernel_ms")
        return float(ms.value)

    def read(self) -> Tuple[np.ndarray, np.ndarray]:
        """(D f32[n_tokens, dim], doc_ptr i64[n_docs + 1]): the resident store copied to the host (amdr_maxsim_read)."""
        info = self.info()
        D = np.empty((info[1], self.dim), dtype=np.float32)
        doc_ptr = np.empty(info[0] + 1, dtype=np.int64)
        _check(load().amdr_maxsim_read(self._h, _p(D, C.c_float), _p(doc_ptr, C.c_int64)), "amdr_maxsim_read")
        return D, doc_ptr

    def info(self) -> Tuple[int, int, int, int, int, int]:
        """(n_docs, n_tokens, token capacity, e of the store's scale 2^e, 1 if the split-fp16 images exist, whole-store
        conversions so far)."""
        out = (C.c_int64 * 6)()
        _check(load().amdr_maxsim_info(self._h, out), "amdr_maxsim_info")
        return tuple(int(x) for x in out)

    def stats(self) -> Tuple[float, float]:
        """(d_scale, d_norm_max): the store's power-of-two scale and its largest scaled token norm (amdr_maxsim_stats)."""
        out = (C.c_float * 2)()
        _check(load().amdr_maxsim_stats(self._h, out), "amdr_maxsim_stats")
        return float(out[0]), float(out[1])

    def plan_info(self, nq: int) -> str:
        """Kernels and arithmetic form a search of nq queries launches (no device work)."""
        return self._plan_info("amdr_maxsim_plan_info", nq)

    def reserve(self, nq_max: int, k_max: int) -> None:
        _check(load().amdr_maxsim_reserve(self._h, C.c_int32(nq_max), C.c_int32(k_max)), "amdr_maxsim_reserve")

    def _q(self, Q):
        Q = _c(Q, np.float32)
        if Q.ndim == 2:
            Q = Q[None]
        if Q.ndim != 3 or Q.shape[2] != self.dim:
            raise ValueError(f"Q must be [nq, q_len, {self.dim}]")
        return Q

    def search(self, Q: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
        Q = self._q(Q)
        nq, q_len = Q.shape[0], Q.shape[1]
        scores = np.empty((nq, k), dtype=np.float32)
        ids = np.empty((nq, k), dtype=np.int64)
        _check(load().amdr_maxsim_search(self._h, _p(Q, C.c_float), C.c_int32(nq), C.c_int32(q_len), C.c_int32(k),
                                         _p(scores, C.c_float), _p(ids, C.c_int64)), "amdr_maxsim_search")
        return scores, ids

    def search_device(self, q_ptr: int, nq: int, q_len: int, k: int, scores_ptr: int, ids_ptr: int,
                      stream: int = 0) -> None:
        _check(load().amdr_maxsim_search_device(self._h, _vp(q_ptr), C.c_int32(nq), C.c_int32(q_len), C.c_int32(k),
                                                _vp(scores_ptr), _vp(ids_ptr), _vp(stream)),
               "amdr_maxsim_search_device")

    def scores(self, Q: np.ndarray) -> np.ndarray:
        Q = self._q(Q)
        nq, q_len = Q.shape[0], Q.shape[1]
        out = np.empty((nq, self.n_docs), dtype=np.float32)
        _check(load().amdr_maxsim_scores(self._h, _p(Q, C.c_float), C.c_int32(nq), C.c_int32(q_len),
                                         _p(out, C.c_float)), "amdr_maxsim_scores")
        return out


# ---------------------------------------------------------------------------
class GraphIndex(_Handle):
    """The law graph in HBM for the graph channel (amdr_graph_*, csrc/graph.hip): CSR adjacency over interned article
    ids plus the node <-> chunk-row maps; walk + re-scoring + top-k of a whole batch against a DenseIndex's matrix
    (replaces LawGraphStore.walk + GraphRetriever.search per query, graph_store.py:89-169, graph_retriever.py:82-219)."""
    _destroy = "amdr_graph_destroy"

    def __init__(self, node_ptr, edge_dst, edge_rel, edge_conf_raw, edge_conf_eff, edge_has_evidence, node_present,
                 node_row, row_node, row_norm, row_lang=None, *, n_rel: int, device: int = 0):
        a = dict(node_ptr=_c(node_ptr, np.int64), edge_dst=_c(edge_dst, np.int32), edge_rel=_c(edge_rel, np.int32),
                 conf_raw=_c(edge_conf_raw, np.float64), conf_eff=_c(edge_conf_eff, np.float64),
                 evid=_c(edge_has_evidence, np.int32), present=_c(node_present, np.int32), node_row=_c(node_row, np.int64),
                 row_node=_c(row_node, np.int32), row_norm=_c(row_norm, np.float32))
        lang = None if row_lang is None else _c(row_lang, np.int32)
        self.n_nodes = int(a["present"].shape[0])
        self.n_edges = int(a["edge_dst"].shape[0])
        self.n_rows = int(a["row_node"].shape[0])
        self.n_rel = int(n_rel)
        self.device = int(device)
        if a["node_ptr"].shape[0] != self.n_nodes + 1 or a["node_row"].shape[0] != self.n_nodes:
            raise ValueError("GraphIndex: node tables disagree in length")
        self._h = C.c_void_p()
        _check(load().amdr_graph_create(*(x.ctypes.data for x in a.values()), None if lang is None else lang.ctypes.data,
                                        self.n_nodes, self.n_edges, self.n_rows, self.n_rel, self.device,
                                        C.byref(self._h)), "amdr_graph_create")

    def reserve(self, nq_max: int, k_max: int, limit_max: int) -> None:
        _check(load().amdr_graph_reserve(self._h, int(nq_max), int(k_max), int(limit_max)), "amdr_graph_reserve")

    @staticmethod
    def host_params(limit: int, default_depth: int, min_conf: float, rel_max_depth, rel_allowed, rel_weight, decay,
                    lang: int = -1):
        """(GraphParams over host arrays, the arrays: keep them alive for the call)."""
        keep = (_c(rel_max_depth, np.int32), _c(rel_allowed, np.int32), _c(rel_weight, np.float64), _c(decay, np.float64))
        if keep[3].shape[0] < int(limit) + 1:
            raise ValueError("decay needs limit + 1 entries")
        p = GraphParams(int(limit), int(default_depth), int(lang), 0, float(min_conf), *(x.ctypes.data or None for x in keep))
        return p, keep

    def walk(self, seeds: Sequence[Sequence[int]], params: GraphParams):
        """Per query, the walk from NODE ids: list of (node, depth, parent, relation, has_evidence, conf_raw) tuples."""
        nq = len(seeds)
        ld = max([len(s) for s in seeds] + [1])
        S = np.full((max(nq, 1), ld), -1, dtype=np.int64)
        for i, s in enumerate(seeds):
            S[i, :len(s)] = s
        cnt = np.array([len(s) for s in seeds] + [0] * (nq == 0), dtype=np.int32)
        L = int(params.limit)
        outs = [np.empty((max(nq, 1), L), dtype=t) for t in (np.int32,) * 5 + (np.float64,)]
        oc = np.zeros(max(nq, 1), dtype=np.int32)
        _check(load().amdr_graph_walk(self._h, S.ctypes.data, cnt.ctypes.data, ld, ld, nq, C.byref(params), oc.ctypes.data,
                                      *(o.ctypes.data for o in outs)), "amdr_graph_walk")
        node, depth, parent, rel, evid, conf = outs
        return [[(int(node[q, i]), int(depth[q, i]), int(parent[q, i]), int(rel[q, i]), bool(evid[q, i]),
                  float(conf[q, i])) for i in range(int(oc[q]))] for q in range(nq)]

    def search(self, dense: "DenseIndex", Q: np.ndarray, seeds: np.ndarray, seed_count: np.ndarray, seed_n: int, k: int,
               params: GraphParams, out=None):
        """Host-pointer search: Q f32 [nq, d], seeds i64 chunk rows [nq, ld], seed_count i32 [nq] -> dict of
        count [nq] and rows / final / semantic / depth / relation / edge_conf [nq, k] (`out`: the caller's arrays of
        _outputs(nq, k), written in place)."""
        Q = _c(Q, np.float32).reshape(-1, dense.d)
        nq = Q.shape[0]
        seeds = _c(seeds, np.int64).reshape(nq, -1)
        seed_count = _c(seed_count, np.int32).reshape(nq)
        out = self._outputs(nq, k) if out is None else out
        _check(load().amdr_graph_search(self._h, dense._h, Q.ctypes.data, seeds.ctypes.data, seed_count.ctypes.data,
                                        seeds.shape[1], int(seed_n), nq, int(k), C.byref(params),
                                        *(out[n].ctypes.data for n in self.OUTS)), "amdr_graph_search")
        return out

    OUTS = ("count", "rows", "final", "semantic", "depth", "relation", "edge_conf")
    _OUT_T = (np.int32, np.int64, np.float64, np.float32, np.int32, np.int32, np.float64)

    @classmethod
    def _outputs(cls, nq: int, k: int):
        return {n: np.empty((nq,) if n == "count" else (nq, k), dtype=t) for n, t in zip(cls.OUTS, cls._OUT_T)}

    def search_device(self, dense: "DenseIndex", q_ptr: int, qsel_ptr: int, seeds_ptr: int, seed_count_ptr: int, ld: int,
                      seed_n: int, ng: int, k: int, params: GraphParams, outs: Sequence[int], stream: int = 0) -> None:
        """Device pointers; outs = the seven output pointers in OUTS order.  Enqueue only."""
        _check(load().amdr_graph_search_device(self._h, dense._h, _vp(q_ptr), _vp(qsel_ptr), _vp(seeds_ptr),
                                               _vp(seed_count_ptr), int(ld), int(seed_n), int(ng), int(k),
                                               C.byref(params), *(_vp(o) for o in outs), _vp(stream)),
               "amdr_graph_search_device")


# ---------------------------------------------------------------------------
def scope_workspace_plan(nq_max: int, k_max: int, rows_max_reserve: int, nq: int, k: int,
                         rows_max: int) -> Tuple[Tuple[int, int, int], Tuple[int, int, int]]:
    """(bytes ScopeWorkspace.reserve(nq_max, k_max, rows_max_reserve) sizes, bytes the scoped "_device" calls of
    (nq, k, rows_max) use), each as (dense, BM25, MaxSim region) — host-only arithmetic."""
    out = (C.c_int64 * 6)()
    _check(load().amdr_scope_workspace_plan(C.c_int32(nq_max), C.c_int32(k_max), C.c_int64(rows_max_reserve), C.c_int32(nq),
                                            C.c_int32(k), C.c_int64(rows_max), out), "amdr_scope_workspace_plan")
    v = [int(x) for x in out]
    return tuple(v[:3]), tuple(v[3:])


def hybrid_scope_plan(nq: int, kd: int, kb: int, kc: int, rows_max_dense: int, rows_max_bm25: int) -> Tuple[bool, int]:
    """(whether ScopeWorkspace.hybrid of these sizes is the one launch of scope_hybrid_kernel, its dynamic LDS bytes) —
    host-only; AMDR_SCOPE_FUSED=0 and AMDR_SCOPE_SLAB are read per call."""
    fused, lds = C.c_int32(0), C.c_int64(0)
    _check(load().amdr_hybrid_scope_plan(C.c_int32(nq), C.c_int32(kd), C.c_int32(kb), C.c_int32(kc), C.c_int64(rows_max_dense),
                                         C.c_int64(rows_max_bm25), C.byref(fused), C.byref(lds)), "amdr_hybrid_scope_plan")
    return bool(fused.value), int(lds.value)


def check_scope_table(scope_ptr, rows, qscope) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """(scope_ptr i64 [n_scopes + 1], rows i64, qscope i32 [nq], rows_max) as contiguous arrays of the ABI's types."""
    scope_ptr, rows, qscope = _c(scope_ptr, np.int64).ravel(), _c(rows, np.int64).ravel(), _c(qscope, np.int32).ravel()
    if scope_ptr.size < 1:
        raise ValueError("scope table: scope_ptr needs at least one entry")
    if int(scope_ptr.min()) < 0 or int(scope_ptr.max()) > rows.size:
        raise ValueError("scope table: scope_ptr points outside rows")
    rows_max = int(np.diff(scope_ptr).max()) if scope_ptr.size > 1 else 0
    return scope_ptr, rows, qscope, max(rows_max, 0)


class ScopeWorkspace(_Handle):
    """Workspace of the scoped channel searches (amdr_scope_t, csrc/scope.hip): the top-k of each query's OWN rows — a
    scope table (scope_ptr, rows, qscope) travels with every call — in the dense, BM25 and ColBERT channels, with the
    score bits and the order of the unscoped channel.  Owns no table; one slab-list region per channel."""
    _destroy = "amdr_scope_destroy"

    def __init__(self, *, device: int = 0):
        self._h = C.c_void_p()
        self.device = int(device)
        self.nq_max = self.k_max = self.rows_max = 0
        _check(load().amdr_scope_create(C.c_int32(device), C.byref(self._h)), "amdr_scope_create")

    def reserve(self, nq_max: int, k_max: int, rows_max: int) -> None:
        _check(load().amdr_scope_reserve(self._h, C.c_int32(nq_max), C.c_int32(k_max), C.c_int64(rows_max)),
               "amdr_scope_reserve")
        self.nq_max, self.k_max, self.rows_max = int(nq_max), int(k_max), int(rows_max)

    def plan_info(self, nq: int, k: int, rows_max: int) -> str:
        buf = C.create_string_buffer(1024)
        _check(load().amdr_scope_plan_info(self._h, C.c_int32(nq), C.c_int32(k), C.c_int64(rows_max), buf,
                                           C.c_int32(len(buf))), "amdr_scope_plan_info")
        return buf.value.decode()

    # -- host-pointer twins: (scores [nq, k], ids i64 [nq, k]), -1 padded -------------------------------------------
    def dense_search(self, dense: "DenseIndex", Q: np.ndarray, scope_ptr, rows, qscope, k: int):
        Q = _c(Q, np.float32)
        if Q.ndim == 1:
            Q = Q[None, :]
        if Q.shape[1] != dense.d:
            raise ValueError(f"dense_search: query dim {Q.shape[1]} != index dim {dense.d}")
        scope_ptr, rows, qscope, _ = check_scope_table(scope_ptr, rows, qscope)
        nq = Q.shape[0]
        if qscope.size != nq:
            raise ValueError("dense_search: one qscope entry per query")
        scores = np.empty((nq, k), dtype=np.float32)
        ids = np.empty((nq, k), dtype=np.int64)
        _check(load().amdr_scope_dense_search(self._h, dense._h, _p(Q, C.c_float), _p(scope_ptr, C.c_int64),
                                              _p(rows, C.c_int64), _p(qscope, C.c_int32), C.c_int32(scope_ptr.size - 1),
                                              C.c_int32(nq), C.c_int32(k), _p(scores, C.c_float), _p(ids, C.c_int64)),
               "amdr_scope_dense_search")
        return scores, ids

    def bm25_search(self, bm25: "BM25Index", queries: Sequence[Sequence[int]], scope_ptr, rows, qscope, k: int):
        q_terms, q_ptr = BM25Index.pack_queries(queries)
        scope_ptr, rows, qscope, _ = check_scope_table(scope_ptr, rows, qscope)
        nq = len(queries)
        if qscope.size != nq:
            raise ValueError("bm25_search: one qscope entry per query")
        scores = np.empty((nq, k), dtype=np.float64)
        ids = np.empty((nq, k), dtype=np.int64)
        _check(load().amdr_scope_bm25_search(self._h, bm25._h, _p(q_terms, C.c_int32), _p(q_ptr, C.c_int64),
                                             _p(scope_ptr, C.c_int64), _p(rows, C.c_int64), _p(qscope, C.c_int32),
                                             C.c_int32(scope_ptr.size - 1), C.c_int32(nq), C.c_int32(k),
                                             _p(scores, C.c_double), _p(ids, C.c_int64)), "amdr_scope_bm25_search")
        return scores, ids

    def maxsim_search(self, maxsim: "MaxSimIndex", Q: np.ndarray, scope_ptr, rows, qscope, k: int):
        Q = maxsim._q(Q)
        scope_ptr, rows, qscope, _ = check_scope_table(scope_ptr, rows, qscope)
        nq = Q.shape[0]
        if qscope.size != nq:
            raise ValueError("maxsim_search: one qscope entry per query")
        scores = np.empty((nq, k), dtype=np.float32)
        ids = np.empty((nq, k), dtype=np.int64)
        _check(load().amdr_scope_maxsim_search(self._h, maxsim._h, _p(Q, C.c_float), C.c_int32(Q.shape[1]),
                                               _p(scope_ptr, C.c_int64), _p(rows, C.c_int64), _p(qscope, C.c_int32),
                                               C.c_int32(scope_ptr.size - 1), C.c_int32(nq), C.c_int32(k),
                                               _p(scores, C.c_float), _p(ids, C.c_int64)), "amdr_scope_maxsim_search")
        return scores, ids

    def facet_counts(self, scope_ptr, rows, codes, n_codes: Sequence[int], top: int, rows_max: Optional[int] = None):
        """amdr_facet_counts, the host-pointer twin: (total i64 [n_cons], missing i64 [n_cons, n_fields], distinct i32
        [n_cons, n_fields], code i32 [n_cons, n_fields, top], count i64 [n_cons, n_fields, top]) of the scope table
        (scope_ptr i64 [n_cons + 1], rows i64) over the code columns codes i32 [n_fields, n_rows]; n_codes: one entry per
        field.  rows_max (None: the longest scope) is the bound the call takes."""
        scope_ptr, rows = _c(scope_ptr, np.int64).ravel(), _c(rows, np.int64).ravel()
        codes = np.atleast_2d(_c(codes, np.int32))
        nc = _c(n_codes, np.int64).ravel()
        n_cons, (n_fields, n_rows) = max(int(scope_ptr.size) - 1, 0), codes.shape
        if nc.size != n_fields:
            raise ValueError("facet_counts: one n_codes entry per code column")
        if rows_max is None:
            rows_max = int(np.diff(scope_ptr).max()) if n_cons else 0
        t = max(int(top), 0)
        total = np.empty(n_cons, dtype=np.int64)
        missing = np.empty((n_cons, n_fields), dtype=np.int64)
        distinct = np.empty((n_cons, n_fields), dtype=np.int32)
        code = np.empty((n_cons, n_fields, t), dtype=np.int32)
        count = np.empty((n_cons, n_fields, t), dtype=np.int64)
        _check(load().amdr_facet_counts(self._h, _p(scope_ptr, C.c_int64), _p(rows, C.c_int64), C.c_int64(n_cons),
                                        C.c_int64(rows_max), _p(codes, C.c_int32), C.c_int64(n_rows), C.c_int32(n_fields),
                                        _p(nc, C.c_int64), C.c_int32(top), _p(total, C.c_int64), _p(missing, C.c_int64),
                                        _p(distinct, C.c_int32), _p(code, C.c_int32), _p(count, C.c_int64)),
               "amdr_facet_counts")
        return total, missing, distinct, code, count

    # -- "_device" forms: pointers in, enqueue only; table = (scope_ptr, rows, qscope, n_scopes, rows_max) ----------
    def dense_search_device(self, dense: "DenseIndex", q_ptr: int, table, nq: int, k: int, scores_ptr: int, ids_ptr: int,
                            stream: int = 0) -> None:
        sp, rw, qs, ns, rmax = table
        _check(load().amdr_scope_dense_search_device(self._h, dense._h, _vp(q_ptr), _vp(sp), _vp(rw), _vp(qs), C.c_int32(ns),
                                                     C.c_int64(rmax), C.c_int32(nq), C.c_int32(k), _vp(scores_ptr),
                                                     _vp(ids_ptr), _vp(stream)), "amdr_scope_dense_search_device")

    def bm25_search_device(self, bm25: "BM25Index", q_terms_ptr: int, q_ptr_ptr: int, table, nq: int, k: int,
                           scores_ptr: int, ids_ptr: int, stream: int = 0) -> None:
        sp, rw, qs, ns, rmax = table
        _check(load().amdr_scope_bm25_search_device(self._h, bm25._h, _vp(q_terms_ptr), _vp(q_ptr_ptr), _vp(sp), _vp(rw),
                                                    _vp(qs), C.c_int32(ns), C.c_int64(rmax), C.c_int32(nq), C.c_int32(k),
                                                    _vp(scores_ptr), _vp(ids_ptr), _vp(stream)),
               "amdr_scope_bm25_search_device")

    def maxsim_search_device(self, maxsim: "MaxSimIndex", q_ptr: int, q_len: int, table, nq: int, k: int, scores_ptr: int,
                             ids_ptr: int, stream: int = 0) -> None:
        sp, rw, qs, ns, rmax = table
        _check(load().amdr_scope_maxsim_search_device(self._h, maxsim._h, _vp(q_ptr), C.c_int32(q_len), _vp(sp), _vp(rw),
                                                      _vp(qs), C.c_int32(ns), C.c_int64(rmax), C.c_int32(nq), C.c_int32(k),
                                                      _vp(scores_ptr), _vp(ids_ptr), _vp(stream)),
               "amdr_scope_maxsim_search_device")

    def hybrid(self, dense: "DenseIndex", bm25: "BM25Index", params: "FuseParams", q_ptr: int, q_terms_ptr: int,
               q_ptr_ptr: int, dense_table, bm25_table, nq: int, kd: int, kb: int, maps, colbert, lists, outs,
               stream: int = 0) -> None:
        """The scoped step as one call (amdr_hybrid_scope_device): the dense and the BM25 top-k of each query's own rows
        and their fusion — one launch when both scopes fit a slab and kd + kb + kc <= 32, the separate calls inside
        otherwise.  maps = (dense, BM25, ColBERT) row -> uid pointers (0: none); colbert = (ids, scores, kc) of lists
        finished earlier on the stream, or None; lists = (dense scores, dense ids, BM25 scores, BM25 ids) and outs =
        (ids, vals, mask, count): output pointers."""
        dsp, drw, dqs, dns, drm = dense_table
        bsp, brw, bqs, bns, brm = bm25_table
        ci, cs, kc = colbert if colbert is not None else (0, 0, 0)
        _check(load().amdr_hybrid_scope_device(
            self._h, dense._h, bm25._h, _vp(q_ptr), _vp(q_terms_ptr), _vp(q_ptr_ptr), _vp(dsp), _vp(drw), _vp(dqs),
            C.c_int32(dns), C.c_int64(drm), _vp(bsp), _vp(brw), _vp(bqs), C.c_int32(bns), C.c_int64(brm), C.c_int32(nq),
            C.c_int32(kd), C.c_int32(kb), C.byref(params), _vp(maps[0]), _vp(maps[1]), _vp(ci), _vp(cs), C.c_int32(kc),
            _vp(maps[2]), *(_vp(x) for x in lists), *(_vp(x) for x in outs), _vp(stream)), "amdr_hybrid_scope_device")


def make_fuse_params(*, method: str = "rrf_norm_blend", rrf_k: int = 60, alpha: float = 0.5, w_dense: float = 0.6,
                     w_bm25: float = 0.4, w_colbert: float = 0.35, min_final_score: float = -math.inf) -> FuseParams:
    m = FUSE_METHODS.get(str(method).lower(), 0)  # unknown strings fall to the blend, like the reference's `else`
    return FuseParams(m, int(rrf_k), float(alpha), float(w_dense), float(w_bm25), float(w_colbert),
                      float(min_final_score))


def _chan(ids, scores, sdtype, nq):
    if ids is None or scores is None:
        return None, None, 0
    ids = _c(ids, np.int64).reshape(nq, -1)
    scores = _c(scores, sdtype).reshape(nq, -1)
    assert ids.shape == scores.shape
    if ids.shape[1] == 0:
        return None, None, 0
    return ids, scores, int(ids.shape[1])


def fuse(params: FuseParams, nq: int, dense=None, bm25=None, colbert=None):
    """Host-pointer fusion. Each channel is (ids i64[nq,k], scores[nq,k]) or None.
    Returns (ids [nq,max_out], vals [nq,max_out,9], mask [nq,max_out], count [nq])."""
    di, ds, kd = _chan(*(dense or (None, None)), np.float64, nq)
    bi, bs, kb = _chan(*(bm25 or (None, None)), np.float64, nq)
    ci, cs, kc = _chan(*(colbert or (None, None)), np.float64, nq)
    mo = kd + kb + kc
    out_ids = np.full((nq, max(mo, 1)), -1, dtype=np.int64)
    out_vals = np.zeros((nq, max(mo, 1), FUSE_NVALS), dtype=np.float64)
    out_mask = np.zeros((nq, max(mo, 1)), dtype=np.int32)
    out_count = np.zeros((nq,), dtype=np.int32)
    if mo == 0 or nq == 0:
        return out_ids[:, :0], out_vals[:, :0], out_mask[:, :0], out_count
    _check(load().amdr_fuse(C.byref(params), C.c_int32(nq), _p(di, C.c_int64), _p(ds, C.c_double), C.c_int32(kd),
                            _p(bi, C.c_int64), _p(bs, C.c_double), C.c_int32(kb), _p(ci, C.c_int64),
                            _p(cs, C.c_double), C.c_int32(kc), _p(out_ids, C.c_int64), _p(out_vals, C.c_double),
                            _p(out_mask, C.c_int32), _p(out_count, C.c_int32)), "amdr_fuse")
    return out_ids, out_vals, out_mask, out_count


def fuse_device(params: FuseParams, nq: int, dense, bm25, colbert, out_ids: int, out_vals: int, out_mask: int,
                out_count: int, *, device: int = 0, stream: int = 0) -> None:
    """Device-pointer fusion. Each channel = (ids_ptr, scores_ptr, k, row2uid_ptr|0) or None."""
    def un(c):
        return c if c is not None else (0, 0, 0, 0)
    d, b, c = un(dense), un(bm25), un(colbert)
    _check(load().amdr_fuse_device(C.byref(params), C.c_int32(nq),
                                   _vp(d[0]), _vp(d[1]), C.c_int32(d[2]), _vp(d[3]),
                                   _vp(b[0]), _vp(b[1]), C.c_int32(b[2]), _vp(b[3]),
                                   _vp(c[0]), _vp(c[1]), C.c_int32(c[2]), _vp(c[3]),
                                   _vp(out_ids), _vp(out_vals), _vp(out_mask), _vp(out_count),
                                   C.c_int32(device), _vp(stream)), "amdr_fuse_device")


def rerank_blend(count: np.ndarray, ids: np.ndarray, vals: np.ndarray, mask: np.ndarray, ce_raw: np.ndarray,
                 beta: float):
    """In-place rerank blend on host arrays (copies through the device).
    ce_raw: [nq, top_n].  Returns out_rerank [nq, max_out, 2] (raw, norm)."""
    nq, max_out = ids.shape
    ce_raw = _c(ce_raw, np.float64).reshape(nq, -1)
    top_n = int(ce_raw.shape[1])
    out = np.full((nq, max_out, 2), np.nan, dtype=np.float64)
    assert ids.flags.c_contiguous and vals.flags.c_contiguous and mask.flags.c_contiguous
    count = _c(count, np.int32)
    _check(load().amdr_rerank_blend(C.c_int32(nq), C.c_int32(max_out), _p(count, C.c_int32), _p(ids, C.c_int64),
                                    _p(vals, C.c_double), _p(mask, C.c_int32), _p(ce_raw, C.c_double),
                                    C.c_int32(top_n), C.c_double(beta), _p(out, C.c_double)), "amdr_rerank_blend")
    return out


def rerank_blend_device(nq: int, max_out: int, count: int, ids: int, vals: int, mask: int, ce_raw: int, top_n: int,
                        beta: float, out_rerank: int, *, device: int = 0, stream: int = 0) -> None:
    _check(load().amdr_rerank_blend_device(C.c_int32(nq), C.c_int32(max_out), _vp(count), _vp(ids), _vp(vals),
                                           _vp(mask), _vp(ce_raw), C.c_int32(top_n), C.c_double(beta),
                                           _vp(out_rerank), C.c_int32(device), _vp(stream)),
           "amdr_rerank_blend_device")


class DenseSmallApprox(_Handle):
    """The fp16 first pass over a short corpus on its own (amdr_dense_small_*; tests and measurements — the search calls
    run it inside): approximate scores of every (query, row) with a proven per-query bound on their distance from the
    exact dot product."""
    _destroy = "amdr_dense_small_destroy"

    def __init__(self, dense: "DenseIndex"):
        self._h = C.c_void_p()
        self._dense = dense  # must outlive this handle
        _check(load().amdr_dense_small_create(dense._h, C.byref(self._h)), "amdr_dense_small_create")

    def approx_device(self, q_ptr: int, nq: int, s_ptr: int, ld: int, eps_ptr: int = 0, stream: int = 0) -> None:
        _check(load().amdr_dense_small_approx_device(self._h, _vp(q_ptr), C.c_int32(nq), _vp(s_ptr), C.c_int64(ld), _vp(eps_ptr),
                                                     _vp(stream)), "amdr_dense_small_approx_device")


def hybrid_small_plan(dense: "DenseIndex", bm25: "BM25Index", nq: int, kd: int, kb: int, dense_row2uid: int,
                      bm25_row2uid: int, dense_scores: int, dense_ids: int, bm25_scores: int, bm25_ids: int, out_ids: int,
                      out_vals: int, out_mask: int, out_count: int):
    """The per-shape part of an amdr_hybrid_small_device call as ready ctypes values (the serving call is issued once per
    query: building twenty ctypes objects per call costs more than the enqueue)."""
    return (load().amdr_hybrid_small_device, dense._h, bm25._h, C.c_int32(nq), C.c_int32(kd), C.c_int32(kb),
            _vp(dense_row2uid), _vp(bm25_row2uid), _vp(dense_scores), _vp(dense_ids), _vp(bm25_scores), _vp(bm25_ids),
            _vp(out_ids), _vp(out_vals), _vp(out_mask), _vp(out_count))


def hybrid_small_device(plan, params: "FuseParams", q_emb: int, q_terms: int, q_ptr: int, stream: int = 0) -> None:
    """BM25 top-k + dense top-k + fusion of 1-4 queries on a serving corpus as ONE launch (amdr_hybrid_small_device);
    every other shape runs bm25.search_device + dense.search_fuse_device inside.  Same five outputs, bit for bit."""
    fn, dh, bh, nq, kd, kb, m0, m1, ds, di, bs, bi, oi, ov, om, oc = plan
    rc = fn(dh, bh, q_emb, q_terms, q_ptr, nq, kd, kb, C.byref(params), m0, m1, ds, di, bs, bi, oi, ov, om, oc, stream)
    if rc:
        _check(rc, "amdr_hybrid_small_device")


def hybrid_batch_device(dense: "DenseIndex", bm25: "BM25Index", params: "FuseParams", q_emb: int, q_terms: int, q_ptr: int,
                        nq: int, kd: int, kb: int, dense_row2uid: int, bm25_row2uid: int, dense_scores: int, dense_ids: int,
                        bm25_scores: int, bm25_ids: int, out_ids: int, out_vals: int, out_mask: int, out_count: int,
                        stream: int = 0) -> None:
    """The long-batch hybrid step as one native call (amdr_hybrid_batch_device): bm25.search_device +
    dense.search_fuse_device, the same five outputs bit for bit; where the two-pass dense form applies BM25 runs on the
    dense handle's side stream beside the second dense pass (AMDR_HYBRID_BATCH=0: the serial calls)."""
    _check(load().amdr_hybrid_batch_device(
        dense._h, bm25._h, _vp(q_emb), _vp(q_terms), _vp(q_ptr), C.c_int32(nq), C.c_int32(kd), C.c_int32(kb), C.byref(params),
        _vp(dense_row2uid), _vp(bm25_row2uid), _vp(dense_scores), _vp(dense_ids), _vp(bm25_scores), _vp(bm25_ids),
        _vp(out_ids), _vp(out_vals), _vp(out_mask), _vp(out_count), _vp(stream)), "amdr_hybrid_batch_device")


def fuse_compact_device(nq: int, max_out: int, w: int, ids: int, vals: int, mask: int, count: int, out_rows: int,
                        out_scores: int, out_mask: int, out_count: int, *, device: int = 0, stream: int = 0) -> None:
    _check(load().amdr_fuse_compact_device(nq, max_out, w, ids, vals, mask, count, out_rows, out_scores, out_mask, out_count,
                                           device, stream), "amdr_fuse_compact_device")


def merge_topk_device(scores: int, ids: int, n_parts: int, nq: int, k_in: int, k_out: int, out_scores: int,
                      out_ids: int, *, f64: bool, device: int = 0, stream: int = 0) -> None:
    fn = load().amdr_merge_topk_f64_device if f64 else load().amdr_merge_topk_f32_device
    _check(fn(_vp(scores), _vp(ids), C.c_int32(n_parts), C.c_int32(nq), C.c_int32(k_in), C.c_int32(k_out),
              _vp(out_scores), _vp(out_ids), C.c_int32(device), _vp(stream)), "amdr_merge_topk_device")


# ---------------------------------------------------------------------------
def shard_chans(chans):
    """[(scores_ptr, ids_ptr, k, is_f64)] -> (amdr_shard_chan_t array, n): the argument block of the shard calls."""
    arr = (ShardChan * len(chans))()
    for c, (sp, ip, k, f64) in zip(arr, chans):
        c.scores, c.ids, c.k, c.f64 = int(sp) if sp else None, int(ip) if ip else None, int(k), 1 if f64 else 0
    return arr, len(chans)


def shard_row_words(ks: Sequence[int]) -> int:
    """int64 words per query row of the packed exchange buffer: sum of 2 * k_c."""
    arr, n = shard_chans([(0, 0, k, False) for k in ks])
    w = C.c_int64(0)
    _check(load().amdr_shard_row_words(arr, C.c_int32(n), C.byref(w)), "amdr_shard_row_words")
    return int(w.value)


def shard_pack_args(args, nq: int, id_offset: int, send_ptr: int, *, device: int = 0, stream: int = 0) -> None:
    _check(load().amdr_shard_pack_device(args[0], args[1], nq, id_offset, send_ptr, device, stream),
           "amdr_shard_pack_device")


def shard_merge_args(gathered_ptr: int, world: int, nq: int, args, *, device: int = 0, stream: int = 0) -> None:
    _check(load().amdr_shard_merge_device(gathered_ptr, world, nq, args[0], args[1], device, stream),
           "amdr_shard_merge_device")


def shard_pack_device(chans, nq: int, id_offset: int, send_ptr: int, *, device: int = 0, stream: int = 0) -> None:
    """chans: [(scores_ptr, local_ids_ptr, k, is_f64)] of this rank -> send [nq, row] (ONE launch, all channels)."""
    shard_pack_args(shard_chans(chans), nq, id_offset, send_ptr, device=device, stream=stream)


def shard_merge_device(gathered_ptr: int, world: int, nq: int, out_chans, *, device: int = 0, stream: int = 0) -> None:
    """gathered [world, nq, row] -> out_chans [(out_scores_ptr, out_ids_ptr, k, is_f64)] (ONE launch, all channels)."""
    shard_merge_args(gathered_ptr, world, nq, shard_chans(out_chans), device=device, stream=stream)

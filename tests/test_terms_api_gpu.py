"""Required and excluded terms through the public interface, on the UCC-en fixture (tests/golden/corpus/law_en.jsonl, 592
articles): search(q, terms=T) equals search(q, scope=Scope(chunk_ids=ids)) with `ids` computed on the host from the index's
own token lists — the path a caller had before — hit for hit, with tolerance 0; every returned chunk satisfies T."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import assert_hits_equal_mod_ties
from test_replace_api_gpu import _build, _cfg

pytestmark = pytest.mark.gpu

QUESTIONS = ["what warranty does a merchant give that goods are merchantable", "Short Titles",
             "statute of frauds signed writing sale of goods price of $500", "risk of loss passes to the buyer"]
TOP_K = 20


def dump(h):
    return {"id": h.chunk.id, "score": float(h.score), "rank": h.rank, "source": h.source, "breakdown": h.score_breakdown}


def same(got, exp):
    assert_hits_equal_mod_ties([dump(h) for h in got], [dump(h) for h in exp], float_tol=0.0)


@pytest.fixture(scope="module")
def live(tmp_path_factory):
    """The whole fixture behind a live HybridRetriever (stand-in encoders, ColBERT included; min_final_score below every
    fused score, so a list is cut by top_k and by the constraint alone)."""
    from legal_rag_amd.retrieval.corpus_loader import load_chunks_from_dir
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    root = tmp_path_factory.mktemp("terms_api")
    seen, chunks = set(), []
    for c in load_chunks_from_dir(str(GOLDEN / "corpus"), "law_en.jsonl"):  # (592 lines, one id twice: the first is kept)
        if c.id not in seen:
            seen.add(c.id)
            chunks.append(c)
    assert len(chunks) == 591
    cfg = _cfg(root / "live")
    cfg.retrieval.min_final_score = -1.0
    _build(cfg, chunks, root / "all.jsonl")
    r = HybridRetriever(cfg)
    assert r.colbert is not None and r.colbert.enabled
    return cfg, r


def token_sets(r):
    """[(chunk id, the token set of the chunk)] from the BM25 index's own token lists."""
    r.bm25.load()
    return [(c.id, set(f)) for c, f in zip(r.bm25.chunks, r.bm25.bm25.doc_freqs)]


def ids_of(r, terms, scope_pred=None):
    return [cid for (cid, toks), c in zip(token_sets(r), r.bm25.chunks)
            if terms.matches(toks) and (scope_pred is None or scope_pred(c))]


def constraints():
    from legal_rag_amd.retrieval.terms import Terms
    return (Terms(any_of=["warranty", "lease"]),                        # larger than top_k
            Terms(all_of=["seller", "goods"], none_of=["buyer"]),       # smaller than top_k: the list is shorter
            Terms(all_of=["seller", ("goods", "zzz-not-a-token")]))     # empty


def test_search_with_terms_equals_the_explicit_scope_and_every_hit_satisfies_them(live):
    from legal_rag_amd.retrieval.scope import Scope
    cfg, r = live
    big, small, empty = constraints()
    toks = dict(token_sets(r))
    n_big, n_small, n_empty = (len(ids_of(r, t)) for t in (big, small, empty))
    # the three kinds, from the token lists
    assert n_big > TOP_K and 0 < n_small < TOP_K and n_empty == 0 and len(toks) == len(r.bm25.chunks) == 591
    for q in QUESTIONS[:3]:
        for t, n in ((big, n_big), (small, n_small)):
            got = r.search(q, top_k=TOP_K, terms=t)
            same(got, r.search(q, top_k=TOP_K, scope=Scope(chunk_ids=ids_of(r, t))))
            assert len(got) == min(TOP_K, n) and all(t.matches(toks[h.chunk.id]) for h in got)
            assert [h.rank for h in got] == list(range(1, len(got) + 1))
        assert r.search(q, top_k=TOP_K, terms=empty) == []
    # nothing given: today's path
    from legal_rag_amd.retrieval.terms import Terms
    assert [dump(h) for h in r.search(QUESTIONS[0], top_k=TOP_K, terms=Terms())] == \
        [dump(h) for h in r.search(QUESTIONS[0], top_k=TOP_K)]
    with pytest.raises(ValueError, match="graph"):
        r.search(QUESTIONS[0], top_k=TOP_K, terms=big, decision=SimpleNamespace(mode="GRAPH_AUGMENTED"))


def best_section(r, terms):
    """The section that holds the most chunks satisfying `terms`, but not all of them."""
    count = {}
    for (cid, toks), c in zip(token_sets(r), r.bm25.chunks):
        if terms.matches(toks) and c.section:
            count[c.section] = count.get(c.section, 0) + 1
    return max(count, key=count.get), sum(count.values())


def test_terms_with_a_scope_rank_the_intersection(live):
    from legal_rag_amd.retrieval.scope import Scope
    cfg, r = live
    big = constraints()[0]
    sec, total = best_section(r, big)
    both = ids_of(r, big, lambda c: c.section == sec)
    assert 0 < len(both) < total
    for q in QUESTIONS[:2]:
        got = r.search(q, top_k=TOP_K, terms=big, scope=Scope(section=sec))
        same(got, r.search(q, top_k=TOP_K, scope=Scope(chunk_ids=both)))
        assert len(got) == min(TOP_K, len(both)) and all(h.chunk.section == sec for h in got)
    assert r.search(QUESTIONS[0], top_k=TOP_K, terms=big, scope=Scope(section="no such section")) == []


def test_mixed_batch_is_re_interleaved_and_the_columnar_form_agrees(live):
    from legal_rag_amd.retrieval.scope import Scope
    cfg, r = live
    big, small, empty = constraints()
    sec, _ = best_section(r, big)
    s = Scope(section=sec)
    terms = [None, None, big, big, empty, small, big]
    scopes = [None, s, None, s, None, None, None]
    qs = [QUESTIONS[j % len(QUESTIONS)] for j in range(len(terms))]
    out = r.search_batch(qs, top_k=TOP_K, terms=terms, scopes=scopes)
    for j, hits in enumerate(out):
        same(hits, r.search(qs[j], top_k=TOP_K, terms=terms[j], scope=scopes[j]))
    assert out[4] == [] and all(out[j] for j in (0, 1, 2, 3, 5, 6))
    same(out[0], r.search_batch([qs[0]], top_k=TOP_K)[0])
    same(out[1], r.search_batch([qs[1]], top_k=TOP_K, scopes=[s])[0])
    for values in (True, False):
        arr = r.search_batch_arrays(qs, top_k=TOP_K, terms=terms, scopes=scopes, values=values)
        for j, hits in enumerate(out):
            assert arr["count"][j] == len(hits)
            assert arr["scores"][j, :len(hits)].tolist() == [h.score for h in hits]
            assert sorted(arr["chunks"][int(x)].id for x in arr["rows"][j, :len(hits)]) == sorted(h.chunk.id for h in hits)
            assert np.all(arr["rows"][j, len(hits):] == -1)


def test_per_channel_searches_take_terms(live):
    from legal_rag_amd.retrieval.scope import Scope
    cfg, r = live
    big, small, empty = constraints()
    q = QUESTIONS[0]
    for fn in (r.search_dense, r.search_bm25, r.search_colbert):
        for t in (big, small):
            got = fn(q, TOP_K, terms=t)
            same(got, fn(q, TOP_K, scope=Scope(chunk_ids=ids_of(r, t))))
            assert len(got) == min(TOP_K, len(ids_of(r, t)))
        assert fn(q, TOP_K, terms=empty) == []


def test_a_status_word_raises_and_names_the_constraint(live, monkeypatch):
    from legal_rag_amd.retrieval import hybrid_retriever as HR
    cfg, r = live
    big, small, _ = constraints()
    pack = HR._pack_terms

    def short(*a, **k):
        tt = pack(*a, **k)
        tt.cand_max -= 1  # one below the longest driver: that constraint's status word is 1
        return tt
    monkeypatch.setattr(HR, "_pack_terms", short)
    with pytest.raises(RuntimeError, match="term constraint 1 of the batch"):
        r.search_batch([QUESTIONS[0]] * 2, top_k=TOP_K, terms=[small, big])


def test_after_a_removal_the_same_terms_follow_the_renumbered_index(live):
    """Last in this file: it edits the live indexes."""
    from legal_rag_amd.retrieval.builders.remove import remove_chunk_ids
    from legal_rag_amd.retrieval.scope import Scope
    cfg, r = live
    small = constraints()[1]
    q = QUESTIONS[2]
    before = r.search(q, top_k=TOP_K, terms=small)
    victim = before[0].chunk.id
    n_before = len(ids_of(r, small))
    assert remove_chunk_ids(cfg, [victim]) == {"bm25": 1, "dense": 1, "colbert": 1}
    ids = ids_of(r, small)
    assert len(ids) == n_before - 1 and victim not in ids and len(r.bm25.chunks) == 590
    got = r.search(q, top_k=TOP_K, terms=small)
    assert victim not in [h.chunk.id for h in got] and len(got) == len(ids)
    same(got, r.search(q, top_k=TOP_K, scope=Scope(chunk_ids=ids)))
    w = type(r)(copy.deepcopy(cfg))  # a retriever loaded from the files the removal wrote
    same(got, w.search(q, top_k=TOP_K, terms=small))

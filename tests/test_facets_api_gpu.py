"""Facets through the public interface, on the UCC-en fixture (tests/golden/corpus/law_en.jsonl, 591 articles; the chapter of
a chunk is its source file here and one chunk in nine has no section, so that every field kind is met): facets() and count()
equal a count over the chunk list with `Terms.matches` on each chunk's document tokens — for a Prefix, a Near, a Phrase, a
NearOf, a none_of and a Scope base — facets_batch equals the single calls and resolves a duplicated pair once, the form
without terms equals the resolver's rows, the counts follow an ingest, a removal and a replacement on a live retriever, and
a sharded engine or a foreign BM25 retriever raises before any launch."""
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest

from test_phrase_api_gpu import ucc_chunks
from test_tok_carry_api_gpu import _jsonl

pytestmark = pytest.mark.gpu

FIELDS = ("law_name", "chapter", "section", "article_id")


def _cfg(root):
    from legal_rag_amd.config import AppConfig
    cfg = AppConfig.for_data_dir(str(root), "en")
    cfg.retrieval.encoder_backend = "hashing"
    cfg.retrieval.enable_colbert = False
    cfg.retrieval.enable_rerank = False
    return cfg


def corpus():
    return [c.model_copy(update={"chapter": c.source, "section": None if i % 9 == 4 else c.section})
            for i, c in enumerate(ucc_chunks())]


def retriever(root, chunks, incremental=False):
    """A live HybridRetriever over a BM25 index of `chunks` alone: the facet calls need no other channel.  The batch
    builder's index is cut by the English index rule; `incremental`: the index the live updates continue."""
    from legal_rag_amd.retrieval.builders.bm25_builder import build_bm25_index
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    from legal_rag_amd.retrieval.hybrid_retriever import HybridRetriever
    root.mkdir(parents=True, exist_ok=True)
    cfg = _cfg(root / "live")
    if incremental:
        assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(root / "all.jsonl", chunks)) == len(chunks)
    else:
        build_bm25_index(cfg, chunks)
    r = HybridRetriever(cfg)
    r.bm25.load()
    assert incremental or r.bm25.index_tokenizer == "en_regex"
    assert [c.id for c in r.bm25.chunks] == [c.id for c in chunks]
    return cfg, r


@pytest.fixture(scope="module")
def live(tmp_path_factory):
    cfg, r = retriever(tmp_path_factory.mktemp("facets_api"), corpus())
    return r


def rows_of(r, scope, terms, seqs=None):
    """The rows of the BM25 chunk list inside `scope` whose tokens satisfy `terms`, by the host rule."""
    from legal_rag_amd.retrieval.scope import ScopeResolver
    chunks = r.bm25.chunks
    seqs = seqs if seqs is not None else [r.bm25.document_tokens(c.text) for c in chunks]
    inside = set(ScopeResolver(chunks).rows(scope).tolist()) if scope is not None else None
    return [i for i in range(len(chunks)) if (inside is None or i in inside) and (terms is None or terms.matches(seqs[i]))]


def expected(chunks, rows, spec):
    """(total, {field: (values in the kernel's order, distinct, missing)}): a Counter per field, sorted by count descending
    and then by the row of the value's first appearance in the whole list."""
    out = {}
    for f in spec.by:
        first = {}
        for i, c in enumerate(chunks):
            v = getattr(c, f)
            if v is not None:
                first.setdefault(str(v), i)
        per = Counter(str(getattr(chunks[i], f)) for i in rows if getattr(chunks[i], f) is not None)
        order = sorted(per, key=lambda v: (-per[v], first[v]))
        out[f] = ([(v, per[v]) for v in order[:spec.top]], len(per), len(rows) - sum(per.values()))
    return len(rows), out


def assert_facets(got, want, what):
    total, fields = want
    assert got.total == total, (what, got.total, total)
    assert list(got.fields) == list(fields), what
    for f, (values, distinct, missing) in fields.items():
        g = got.fields[f]
        assert (g.values, g.distinct, g.missing) == (values, distinct, missing), (what, f, g, values[:5], distinct, missing)


def constraints(r):
    from legal_rag_amd.retrieval.scope import Scope
    from legal_rag_amd.retrieval.terms import Near, NearOf, Phrase, Prefix, Terms
    part = next(c.section for c in r.bm25.chunks if c.section and "Perfection" in c.section)
    return [("prefix", None, Terms(all_of=[Prefix("sell")])),
            ("near", None, Terms(all_of=[Near("buyer", "seller", distance=5)])),
            ("phrase", None, Terms(all_of=[Phrase("security", "interest")])),
            ("near-of", None, Terms(all_of=[NearOf(Prefix("buy"), Prefix("sell"), distance=5)])),
            ("none-of", None, Terms(all_of=["goods"], none_of=[Prefix("leas")])),
            ("scope-base", Scope(chapter="ucc_9.txt"), Terms(any_of=[Prefix("secur"), "debtor"])),
            ("scope-section", Scope(section=part), Terms(none_of=["collateral"]))]


def test_facets_and_count_equal_a_count_over_the_chunk_list(live):
    from legal_rag_amd.retrieval.facets import FacetCounts, Facets
    r = live
    chunks = r.bm25.chunks
    seqs = [r.bm25.document_tokens(c.text) for c in chunks]
    specs = (Facets(), Facets(by=("section", "chapter"), top=5), Facets(by=FIELDS, top=64), Facets(by=("article_id",), top=1))
    for name, scope, terms in constraints(r):
        rows = rows_of(r, scope, terms, seqs)
        assert 0 < len(rows) < len(chunks), name
        assert r.count(terms=terms, scope=scope) == len(rows), name
        for spec in specs:
            got = r.facets(terms=terms, scope=scope, spec=spec)
            assert isinstance(got, FacetCounts)
            assert_facets(got, expected(chunks, rows, spec), (name, spec))
    # the fixture holds what the checks need: chunks without a section among the matches, more sections than `top`
    got = r.facets(terms=constraints(r)[0][2], spec=Facets(by=("section",), top=5))
    assert got.fields["section"].missing > 0 and got.fields["section"].distinct > 5 and len(got.fields["section"].values) == 5
    # a constraint nothing satisfies, and an unrestricted one
    from legal_rag_amd.retrieval.terms import Prefix, Terms
    none = r.facets(terms=Terms(all_of=[Prefix("zzzq")]))
    assert none.total == 0 and none.fields["chapter"].values == [] and none.fields["chapter"].distinct == 0
    assert r.count(terms=Terms(all_of=[Prefix("zzzq")])) == 0 and r.count() == len(chunks) and r.count(terms=Terms()) == len(chunks)


def test_the_batch_equals_the_single_calls_and_a_duplicated_pair_is_resolved_once(live, monkeypatch):
    from legal_rag_amd.retrieval import hybrid_retriever as HR
    from legal_rag_amd.retrieval.facets import Facets
    from legal_rag_amd.retrieval.scope import Scope
    r = live
    cons = constraints(r)
    terms = [t for _, _, t in cons] + [cons[0][2], None, None, cons[5][2]]
    scopes = [s for _, s, _ in cons] + [None, Scope(chapter="ucc_2.txt"), None, cons[5][1]]
    spec = Facets(by=("section", "chapter"), top=7)
    tables = []
    pack = HR._pack_terms

    def recording(*a, **k):
        tables.append(pack(*a, **k))
        return tables[-1]
    monkeypatch.setattr(HR, "_pack_terms", recording)
    out = r.facets_batch(terms=terms, scopes=scopes, spec=spec)
    assert len(tables) == 1 and len(out) == len(terms) == 11
    assert tables[0].n_cons == 9 and tables[0].qscope.tolist() == [0, 1, 2, 3, 4, 5, 6, 0, 7, 8, 5]  # equal pairs stored once
    for i, (t, s) in enumerate(zip(terms, scopes)):
        assert out[i] == r.facets(terms=t, scope=s, spec=spec), i
    assert out[7] == out[0] and out[10] == out[5] and out[9].total == len(r.bm25.chunks)
    assert r.count_batch(terms=terms, scopes=scopes) == [o.total for o in out]
    assert r.facets_batch(terms=[], scopes=[]) == []
    with pytest.raises(ValueError, match="one entry per pair"):
        r.facets_batch(terms=terms, scopes=scopes[:3])
    with pytest.raises(TypeError):
        r.facets_batch(terms=["goods"])
    with pytest.raises(TypeError):
        r.facets_batch(scopes=["ucc_2.txt"])
    with pytest.raises(TypeError):
        r.facets(spec=("chapter",))


def test_without_terms_the_counts_are_those_of_the_resolvers_rows(live, monkeypatch):
    from legal_rag_amd.retrieval import hybrid_retriever as HR
    from legal_rag_amd.retrieval.facets import Facets
    from legal_rag_amd.retrieval.scope import Scope, resolver_for
    r = live
    chunks = r.bm25.chunks

    def no_pack(*a, **k):
        raise AssertionError("a batch without terms packed a term table")
    monkeypatch.setattr(HR, "_pack_terms", no_pack)
    part = next(c.section for c in chunks if c.section)
    scopes = [None, Scope(chapter="ucc_9.txt"), Scope(section=part), Scope(article_ids=["2-201", "9-102", "no-such"]),
              Scope(chapter="no such chapter"), Scope(chapter="ucc_9.txt")]
    spec = Facets(by=("chapter", "section", "article_id"), top=12)
    out = r.facets_batch(scopes=scopes, spec=spec)
    for i, s in enumerate(scopes):
        rows = resolver_for(chunks).rows(s if s is not None else Scope()).tolist()
        assert rows == rows_of(r, s, None, seqs=[()] * len(chunks))
        assert_facets(out[i], expected(chunks, rows, spec), i)
        assert r.count(scope=s) == len(rows)
    assert out[0].total == len(chunks) and out[4].total == 0 and out[5] == out[1]
    assert r.count_batch(scopes=scopes) == [o.total for o in out]
    assert r.facets_batch(terms=[None] * len(scopes), scopes=scopes, spec=spec) == out


def test_the_counts_follow_an_ingest_a_removal_and_a_replacement(tmp_path):
    from legal_rag_amd.retrieval.builders.incremental_bm25_builder import IncrementalBM25Builder
    from legal_rag_amd.retrieval.facets import Facets
    from legal_rag_amd.retrieval.scope import Scope
    from legal_rag_amd.retrieval.terms import Prefix, Terms
    every = corpus()
    chunks, more = every[:150:2] + every[400:460], every[1:40:2]
    cfg, r = retriever(tmp_path, chunks, incremental=True)
    spec = Facets(by=("section", "chapter", "article_id"), top=10)
    pairs = [(None, Terms(all_of=[Prefix("sell")])), (Scope(chapter="ucc_2.txt"), Terms(any_of=[Prefix("buy"), "goods"])), (None, None)]

    def check(what, n):
        cur = r.bm25.chunks
        assert len(cur) == n, what
        out = r.facets_batch(terms=[t for _, t in pairs], scopes=[s for s, _ in pairs], spec=spec)
        for (s, t), got in zip(pairs, out):
            assert_facets(got, expected(cur, rows_of(r, s, t), spec), (what, s, t))
        return out
    before = check("built", len(chunks))
    native = r.bm25.gpu_index()
    assert IncrementalBM25Builder(cfg).add_jsonl(_jsonl(tmp_path / "more.jsonl", more)) == len(more)
    grown = check("ingest", len(chunks) + len(more))
    assert r.bm25.gpu_index() is native and grown[2].total == before[2].total + len(more) and grown[0].total > before[0].total
    gone = [c.id for c in r.bm25.chunks if Terms(all_of=[Prefix("sell")]).matches(r.bm25.document_tokens(c.text))][:3]
    assert IncrementalBM25Builder(cfg).remove_ids(gone) == 3
    left = check("removal", len(chunks) + len(more) - 3)
    assert left[0].total == grown[0].total - 3
    # a replacement at the same row: the chunk moves to another section and gains the stem
    victim = next(c for c in r.bm25.chunks if c.section and not Terms(all_of=[Prefix("sell")]).matches(r.bm25.document_tokens(c.text)))
    amended = victim.model_copy(update={"section": "Part Of Its Own", "text": victim.text + " The seller sells."})
    assert IncrementalBM25Builder(cfg).replace_jsonl(_jsonl(tmp_path / "amend.jsonl", [amended])) == 1
    after = check("replacement", len(chunks) + len(more) - 3)
    assert r.bm25.gpu_index() is native and after[0].total == left[0].total + 1
    assert ("Part Of Its Own", 1) in r.facets(terms=pairs[0][1], spec=Facets(by=("section",), top=64)).fields["section"].values


def test_a_sharded_engine_and_a_foreign_bm25_retriever_raise_before_any_launch(live, monkeypatch):
    from legal_rag_amd import _native
    from legal_rag_amd.retrieval.engine import HybridEngine
    from legal_rag_amd.retrieval.scope import Scope, resolver_for
    from legal_rag_amd.retrieval.terms import Prefix, Terms
    r = live
    t = Terms(all_of=[Prefix("sell")])
    assert r.count(terms=t) > 0  # (the engine and the index exist before the launches are forbidden)

    def no_launch(*a, **k):
        raise AssertionError("a refused call reached the library")
    monkeypatch.setattr(_native, "facet_counts_device", no_launch)
    monkeypatch.setattr(_native.BM25Index, "term_scope_device", no_launch)
    eng = HybridEngine(None, r.bm25.gpu_index(), None, device=0, shard_offset=0)
    cols, values = resolver_for(r.bm25.chunks).code_columns(("section",))
    table = (None, None, None, 1, 5)
    with pytest.raises(ValueError, match="row-sharded engine"):
        eng.facet_counts(table, cols, [len(values[0])], 5)
    with pytest.raises(ValueError, match="row-sharded engine"):
        eng.check_facets()
    monkeypatch.setattr(r.bm25, "shard", object(), raising=False)
    for call in (lambda: r.facets(terms=t), lambda: r.count(terms=t), lambda: r.count(scope=Scope(chapter="ucc_2.txt")),
                 lambda: r.facets_batch(terms=[t, None]), lambda: r.count_batch(terms=[t])):
        with pytest.raises(ValueError, match="row-sharded index"):
            call()
    monkeypatch.undo()
    monkeypatch.setattr(_native, "facet_counts_device", no_launch)
    own = r.bm25
    try:
        r.bm25 = SimpleNamespace(search=lambda *a, **k: [], chunks=own.chunks)
        for call in (lambda: r.facets(terms=t), lambda: r.count(terms=t), lambda: r.facets_batch(terms=[t])):
            with pytest.raises(ValueError, match="own BM25 retriever"):
                call()
    finally:
        r.bm25 = own
    monkeypatch.undo()
    assert r.count(terms=t) > 0

"""Certificates of the update sequences (update_sequence_cases.py), from the scripts and the models alone — no GPU:
the scripts visit every transition, every step changes what is checked, numpy restatements of handles with stale derived
state cannot pass, the models equal a fit from nothing, and the exactness budgets hold on every state."""
import numpy as np
import pytest

import dense_adversary as DA
import maxsim_adversary as MS
import update_sequence_cases as C

ALL_PAIRS = {(a, b) for a in C.KINDS for b in C.KINDS}


# ---- 1. transition coverage ---------------------------------------------------------------------------------------------
def test_dense_transitions_and_events():
    states = C.dense_states("dense-tiles")
    print(C.coverage_table("dense-tiles"))
    pairs, refused_after = C.transitions(states)
    # a remove leaves cap_rows == n, so the add behind it always reallocates: the one pair a dense handle cannot take
    assert all(s.cap == s.n for s in states if s.kind == "Rm")
    assert pairs == ALL_PAIRS - {("Rm", "A-in")}, sorted(ALL_PAIRS - pairs)
    assert refused_after == set(C.KINDS)
    assert {s.note for s in states if s.kind == "X"} == {f"refused: {k}" for k in C.X_KINDS}
    for edge in (64, 96, 128, 160):
        assert C.crossings(states, edge) == {"up", "down"}, edge
    ev = C.events(states)
    for name in ("scale up by A-in", "scale down by Rm", "scale up by Rp", "scale down by Rp", "emptied",
                 "add to the empty index", "NaN row in by A-in", "NaN row out by Rp", "infinite row in by A-in",
                 "infinite row out by Rp", "image dropped", "add at cap == n",
                 "replace from mid-tile after an A-in that left img_rows mid-tile"):
        assert ev.get(name), name
    caps = [s.cap for s in states[:6]]
    assert 70 in caps and 140 in caps and 280 in caps  # 70 -> 140 -> 280, then adds inside it
    assert len(ev["image built"]) == 3 and len(ev["image dropped"]) == 2
    # a NaN row leaves the image (the statistics drop it), an infinite row takes it, and only build_image brings it back
    nan_in, inf_in, inf_out = ev["NaN row in by A-in"][0], ev["infinite row in by A-in"][0], ev["infinite row out by Rp"][0]
    assert states[nan_in].image[0] and not states[inf_in].image[0] and not states[inf_out].image[0]
    assert states[inf_out + 1].kind == "B" and states[inf_out + 1].image[0]
    assert sum(s.kind in C.KINDS for s in states[inf_out + 2:]) >= 2  # two more updates behind the last build


@pytest.mark.parametrize("profile, mark", [("dense-short", C.SHORT_MAX), ("dense-rowwaves", C.ROW_WAVES_MAX),
                                           ("dense-hi", C.HI_MIN_ROWS - 1)])
def test_dense_thresholds_are_crossed_both_ways(profile, mark):
    states = C.dense_states(profile)
    print(C.coverage_table(profile))
    assert C.crossings(states, mark) == {"up", "down"}
    kinds = {s.kind for s in states}
    assert {"A-grow", "Rm", "Rp", "X"} <= kinds
    if profile == "dense-short":
        forms = {(C.form_at(s, 64, 10, C.SHORT_PINS), s.n <= mark) for s in states}
        assert forms == {(DA.SMALL, True), (DA.PANEL, False)} or forms == {(DA.SMALL, True), (DA.TILES, False)}, forms
        assert {s.n for s in states} >= {1000, 1030, 1020, 1024, 1025, 1023}
    if profile == "dense-rowwaves":
        assert {DA.form_of(s.n, s.d, 3, 10, {}) for s in states} == {DA.ROWWAVES, DA.SCAN}
        assert {s.n for s in states} >= {16380, 16390, 16384, 16385, 16383}
    if profile == "dense-hi":
        assert C.HI_MIN_ROWS == 6817 and C.HI_KC0 == 33  # 2 hi_kc_max(10) = 214 tiles; hi_kc(10, 0)
        assert {C.form_at(s, 64, C.HI_K, C.HI_PINS) for s in states} == {DA.HI, DA.TWOLEVEL}
        ev = C.events(states)
        for name in ("scale up by A-grow", "scale down by Rm", "scale up by Rp", "scale down by Rp"):
            assert ev.get(name), name
        rp_tiles = {int(i) // 32 for s in states[:5] if s.kind == "Rp" for i in s.op[1]}  # (the replaces before the first remove)
        last = (states[0].n - 1) // 32
        assert 0 in rp_tiles and any(0 < t < last for t in rp_tiles) and any(t >= last - 1 for t in rp_tiles)
        # a replace at the SAME scale right behind an A-in that left img_rows mid-tile, its first row past the first tile:
        # the image is brought up to the matrix from that row's tile on only, and the pinned searches read it
        assert any(a.kind == "A-in" and b.kind == "Rp" and a.n % 32 and a.image[2] == b.image[2] and int(b.op[1][0]) >= 32 and
                   b.n >= C.HI_MIN_ROWS for a, b in zip(states, states[1:]))
        # every query of the pinned searches keeps k rows far above the background: the fp16 pass can resolve it
        Q = C.dense_queries(profile)
        for s in states:
            S = C.rank_scores(s.X, Q)
            kth = np.sort(S, axis=1)[:, -C.HI_K]
            assert np.all(kth >= 1.5 * np.abs(Q).sum(axis=1)), s.step  # (sum |q| is the most a background row can score)


def test_bm25_transitions_and_events():
    states = C.bm25_states()
    print(C.bm25_coverage_table())
    pairs, refused = C.bm25_transitions(states)
    assert pairs == {(a, b) for a in C.BM25_KINDS for b in C.BM25_KINDS}
    assert {k for k, _ in refused} == set(C.BM25_KINDS) and {w for _, w in refused} == set(C.BM25_X)
    ev = C.bm25_events(states)
    for kind in C.BM25_KINDS:
        for residue in ("tile", "tile+1", "tile-1"):
            assert ev.get(f"postings on {residue} by {kind}"), (residue, kind)
    for name in ("terms appear by A", "terms appear by Rp", "terms go with their last document by Rm",
                 "terms go with their last document by Rp", "the order of the surviving terms changes by Rp",
                 "the list of 'all' spans three tiles"):
        assert ev.get(name), name
    assert sum(s.kind in C.BM25_KINDS for s in states) >= 15


def test_colbert_transitions_and_events():
    states = C.ms_states()
    print(C.ms_coverage_table())
    pairs, refused_after = C.transitions(states)
    # a rebuild leaves both capacities exact, so the add behind a remove or a replace always reallocates
    assert all(s.cap_tokens == s.tokens and s.cap_docs == s.n for s in states if s.kind in ("Rm", "Rp"))
    assert pairs == ALL_PAIRS - {("Rm", "A-in"), ("Rp", "A-in")}, sorted(ALL_PAIRS - pairs)
    assert refused_after == set(C.KINDS)
    assert {s.note for s in states if s.kind == "X"} == {f"refused: {k}" for k in C.MS_X}
    assert [s.n for s in states[:5]] == [48, 38, 41, 39, 40]
    ev = C.ms_events(states)
    for name in ("scale up by A-in", "scale down by Rm", "scale up by Rp", "scale down by Rp", "images gone by A-grow",
                 "images back by Rm", "images back by Rp", "A-in on a store without images",
                 "the largest token norm rises by an add that keeps the scale",
                 "one-token and 220-token replacements", "two-pass condition on", "two-pass condition off"):
        assert ev.get(name), name
    assert len(ev["token capacity grows"]) >= 2 and len(ev["document capacity grows"]) >= 2
    assert any(a.kind == "A-in" for a, b in zip(states, states[1:]) if b.kind == "A-grow")  # A-in between the doublings
    lens = {len(d) for s in states for d in s.docs}
    assert 1 in lens and 220 in lens and max(lens) <= 220
    # the conversions: + 1 per rebuild of a finite store and per add that raises the scale, no other add
    for a, b in zip(states, states[1:]):
        rescaled = b.kind in ("A-in", "A-grow") and a.images and b.images and C.scale_exp(b.amax) != C.scale_exp(a.amax)
        assert b.conversions - a.conversions == int((b.kind in ("Rm", "Rp") and b.images) or rescaled), b.step


def test_serving_crosses_the_one_launch_boundary_both_ways():
    states = C.serving_states()
    ns = [s.n for s in states]
    assert ns[:6] == [2040, 2050, 2047, 2048, 2048, 2049]
    up = any(a <= C.SERVING_MAX < b for a, b in zip(ns, ns[1:]))
    down = any(b <= C.SERVING_MAX < a for a, b in zip(ns, ns[1:]))
    assert up and down and {"A", "Rm", "Rp", "X"} <= {s.kind for s in states}


# ---- 2. every step matters ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", C.DENSE_PROFILES)
def test_every_dense_step_changes_every_checked_list(profile):
    states = C.dense_states(profile)
    pairs = [(nq, k) for nq in C.DENSE_NQS for k in C.DENSE_KS]
    if profile == "dense-hi":
        pairs += [(nq, C.HI_K) for nq in C.HI_NQS]
    for prev, st in C.updates(states):
        for nq, k in pairs:
            (ps, pi), (es, ei) = C.expected_topk(profile, prev.step, nq, k), C.expected_topk(profile, st.step, nq, k)
            assert not (np.array_equal(pi, ei) and DA.bits_equal(ps, es)), (profile, st.step, st.note, nq, k)
        # query 0's best row changed, by construction
        assert C.expected_topk(profile, prev.step, 1, 1)[1][0, 0] != C.expected_topk(profile, st.step, 1, 1)[1][0, 0] or \
            not DA.bits_equal(C.expected_topk(profile, prev.step, 1, 1)[0], C.expected_topk(profile, st.step, 1, 1)[0])


def test_every_colbert_step_changes_every_checked_list():
    states = C.ms_states()
    Q = C.ms_queries()
    lists = [MS.topk_expected(C.ms_rank_scores(s.docs, Q).astype(np.float32), C.MS_K) for s in states]
    for j in range(1, len(states)):
        if states[j].kind not in C.KINDS:
            continue
        for nq in C.MS_NQS:
            assert not (np.array_equal(lists[j][1][:nq], lists[j - 1][1][:nq]) and
                        MS.same_scores(lists[j][0][:nq], lists[j - 1][0][:nq])), (j, states[j].note, nq)


def test_every_bm25_step_changes_every_checked_list():
    from bm25_update_cases import SEARCHES
    states = C.bm25_states()
    for j in range(1, len(states)):
        if states[j].kind not in C.BM25_KINDS:
            continue
        _, words = C.bm25_queries(j)
        now, before = C.bm25_oracle(j)[0], C.bm25_oracle(j - 1)[0]
        a = [np.asarray(now.get_scores(w)) for w in words[:SEARCHES[0][0]]]
        b = [np.asarray(before.get_scores(w)) for w in words[:SEARCHES[0][0]]]
        # the one-query list at depth 1 — part of every larger checked batch — has another document or another score
        top = lambda s: (int(np.argmax(s)), float(s.max()))  # noqa: E731  (argmax: the first of equal scores)
        assert [top(x) for x in a] != [top(x) for x in b], (j, states[j].note)


# ---- 3. handles with stale derived state cannot pass ------------------------------------------------------------------------
def test_stale_tile_maxima_lose_a_planted_row_at_every_add_and_replace():
    """(a) tile maxima of the PREVIOUS matrix, the hi_kc(10, 0) = 33 best tiles re-scored on the current one: the ids
    differ from the reference for some query of the pinned searches — unless the pass reports the query unresolved, which
    the counters assert it does not."""
    profile = "dense-hi"
    states, Q = C.dense_states(profile), C.dense_queries(profile)
    for prev, st in C.updates(states):
        if st.kind == "Rm" or st.n < C.HI_MIN_ROWS:
            continue
        ids = C.stale_image_topk(prev.X, st.X, Q, C.HI_K)
        want = C.expected_topk(profile, st.step, C.NQ_ALL, C.HI_K)[1]
        assert not np.array_equal(ids, want), (st.step, st.note)


def test_a_partial_image_refresh_under_a_new_scale_loses_rows():
    """(b) a replace that converts the image again only from the first replaced row's tile on while the scale changed:
    the tiles before it carry the old scale, their maxima are off by 8, and the 33 best tiles miss true rows."""
    profile = "dense-hi"
    states, Q = C.dense_states(profile), C.dense_queries(profile)
    hit = 0
    for prev, st in C.updates(states):
        if st.kind != "Rp" or C.scale_exp(C.amax_of(prev.X)) == C.scale_exp(C.amax_of(st.X)):
            continue
        assert int(st.op[1][0]) >= 32, "the first replaced row lies in the first tile: nothing before it is stale"
        wrong = C.wrong_partial_image(prev, st)
        T = C.tile_maxima(wrong, Q)
        S = C.rank_scores(st.X, Q)
        want = C.expected_topk(profile, st.step, C.NQ_ALL, C.HI_K)[1]
        differs = False
        for q in range(C.NQ_ALL):
            best = np.lexsort((np.arange(T.shape[1]), -T[q]))[:C.HI_KC0]
            rows = np.sort(np.concatenate([np.arange(t * 32, min(t * 32 + 32, st.n)) for t in best]))
            differs = differs or not np.array_equal(C.scoped_expected(st.X, Q[q:q + 1], rows, C.HI_K)[1][0], want[q])
        assert differs, (st.step, st.note)
        hit += 1
    assert hit >= 2  # the scale rises by one replace and falls by another


@pytest.mark.parametrize("profile", C.DENSE_PROFILES)
def test_wrong_row_positions_change_the_lists(profile):
    """(c) a remove that keeps the old rows' positions, (d) an in-place add that writes at cap_rows instead of n."""
    states, Q = C.dense_states(profile), C.dense_queries(profile)
    for prev, st in C.updates(states):
        if st.kind == "Rm" and st.n:
            wrong = C.wrong_remove_keeps_positions(prev, st)
        elif st.kind == "A-in":
            wrong = C.wrong_add_at_capacity(prev, st)
        else:
            continue
        ids = DA.oracle_topk(C.rank_scores(wrong, Q), C.HI_K)[1]
        assert not np.array_equal(ids, C.expected_topk(profile, st.step, C.NQ_ALL, C.HI_K)[1]), (profile, st.step, st.note)


def test_the_previous_idf_vector_changes_the_scores():
    """(f) BM25 scores taken with the idf vector of the previous step differ from the reference at every update."""
    import copy
    states = C.bm25_states()
    for j in range(1, len(states)):
        if states[j].kind not in C.BM25_KINDS:
            continue
        now, before = C.bm25_oracle(j)[0], C.bm25_oracle(j - 1)[0]
        stale = copy.copy(now)
        stale.idf = {w: before.idf.get(w, v) for w, v in now.idf.items()}
        q = ["all", "z0", "z1", "z2"]
        assert np.asarray(stale.get_scores(q)).tobytes() != np.asarray(now.get_scores(q)).tobytes(), (j, states[j].note)


def test_a_bound_kept_across_a_scale_lowering_rebuild_loses_a_true_top_10_document():
    """(e) the two-pass bound kept from before a remove (or replace) that lowers the store's largest component: by the
    fp64 model of the candidate rule (rounding_adversary.model_maxsim_hi + candidates, what maxsim_adversary.twopass_status
    is made of — twopass_status itself asserts the integer family's exactness, under which the first pass has no error and
    no bound matters) the candidate set of EVERY query loses a true top-10 document at the step after it, and holds all
    ten with the bound of the store as it is."""
    import rounding_adversary as RA
    c = C.ms_bound_case()
    Q, (Da, _), (Db, ptr) = c["Q"], c["before"], c["after"]
    assert RA.maxsim_scales(Q, Db)[0] == 8 * RA.maxsim_scales(Q, Da)[0]  # the scale exponent falls by three steps
    stale, true = C.ms_scaled_norm_max(Da), C.ms_scaled_norm_max(Db)
    assert stale < 1.0 < true and true / stale > 4  # the large token alone set the old bound
    exact, approx = RA.exact_maxsim(Q, Db, ptr), RA.model_maxsim_hi(Q, Db, ptr)
    assert np.array_equal(RA.topk_exact(exact, C.BOUND_K)[1], c["top"])
    eps_true, eps_stale = C.ms_eps_with_norm(Q, Db, true), C.ms_eps_with_norm(Q, Db, stale)
    assert np.array_equal(eps_true, RA.maxsim_eps(Q, Db))
    for b in range(len(Q)):
        want = set(c["top"][b].tolist())
        assert want <= set(RA.candidates(approx[b], eps_true[b], C.BOUND_K).tolist()), b
        assert not want <= set(RA.candidates(approx[b], eps_stale[b], C.BOUND_K).tolist()), b
    # the same store with the small document in the large one's place (the replace): the same scale, the same bound
    Dr = np.concatenate([c["small"], Db])
    assert RA.maxsim_scales(Q, Dr)[0] == RA.maxsim_scales(Q, Db)[0] and C.ms_scaled_norm_max(Dr) == true


def test_the_colbert_model_predicts_the_bound_of_every_state():
    """The model's stats(): the scale follows the largest component, the bound the largest scaled token norm — it rises
    with the heavy-token add that keeps the scale, and falls with the removes and replaces that lower it."""
    states = C.ms_states()
    ev = C.ms_events(states)
    j = ev["the largest token norm rises by an add that keeps the scale"][0]
    assert states[j].stats()[0] == states[j - 1].stats()[0] and states[j].stats()[1] > states[j - 1].stats()[1]
    for name in ("scale down by Rm", "scale down by Rp"):
        j = ev[name][0]
        assert states[j].stats()[0] == 8 * states[j - 1].stats()[0] and states[j].stats()[1] != states[j - 1].stats()[1]
    for s in states:
        assert (s.stats() == (1.0, 0.0)) == (not s.images)


# ---- 4. the models equal a fit from nothing -------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", C.DENSE_PROFILES)
def test_the_dense_model_equals_the_replay_of_its_operands(profile):
    states = C.dense_states(profile)
    rows = [r.copy() for r in states[0].op[1]]  # a plain list of rows: concatenation, filter, assignment
    for st in states[1:]:
        if st.op[0] == "add":
            rows += [r.copy() for r in st.op[1]]
        elif st.op[0] == "remove":
            gone = set(int(i) for i in st.op[1])
            rows = [r for i, r in enumerate(rows) if i not in gone]
        elif st.op[0] == "replace":
            for i, r in zip(st.op[1], st.op[2]):
                rows[int(i)] = r.copy()
        X = np.array(rows, dtype=np.float32).reshape(len(rows), st.d)
        assert X.shape == st.X.shape and X.tobytes() == st.X.tobytes(), (profile, st.step)
        if st.op[0] in ("remove", "replace"):
            ids = np.asarray(st.op[1])
            assert np.all(np.diff(ids) > 0) and ids[0] >= 0  # what the call requires: strictly ascending


def test_the_colbert_model_equals_the_replay_of_its_operands():
    states = C.ms_states()
    docs = [d.copy() for d in states[0].docs]
    for st in states[1:]:
        if st.op[0] == "add":
            docs += [d.copy() for d in st.op[1]]
        elif st.op[0] == "remove":
            docs = [d for i, d in enumerate(docs) if i not in set(st.op[1])]
        elif st.op[0] == "replace":
            for i, d in zip(st.op[1], st.op[2]):
                docs[i] = d.copy()
        assert len(docs) == st.n and all(a.tobytes() == b.tobytes() and a.shape == b.shape for a, b in zip(docs, st.docs)), st.step
        assert st.info()[:2] == (len(docs), sum(len(d) for d in docs))


def test_the_bm25_model_equals_the_replay_of_its_operands():
    states = C.bm25_states()
    docs = [list(d) for d in states[0].docs]
    adds = removes = replaces = 0
    for st in states[1:]:
        if st.op[0] == "add":
            docs, adds = docs + [list(d) for d in st.op[1]], adds + 1
        elif st.op[0] == "remove":
            docs, removes = [d for i, d in enumerate(docs) if i not in set(st.op[1])], removes + 1
        elif st.op[0] == "replace":
            for i, d in zip(st.op[1], st.op[2]):
                docs[i] = list(d)
            replaces += 1
        assert docs == st.docs and st.info()[3:] == (adds, removes, replaces), st.step
        csr = C.bm25_oracle(st.step)[1]
        assert st.info()[:3] == (len(csr["doc_len"]), len(csr["idf"]), len(csr["post_doc"])), st.step
        assert list(csr["vocab"]) == list(st.vocab), st.step


# ---- 5. exactness ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", C.DENSE_PROFILES)
def test_the_dense_budget_holds_on_every_state(profile):
    Q = C.dense_queries(profile)
    assert np.all(Q[:, 0] != 0) and np.all(Q[0] != 0) and np.abs(Q).max() == 3
    for st in C.dense_states(profile):
        if st.n:
            assert DA.assert_integer_budget(st.X[st.finite_rows], Q) <= 3 * 24 * st.d
        bad = np.setdiff1d(np.arange(st.n), st.finite_rows)
        assert bad.size <= 1 and np.all(np.isnan(st.X[bad, 1:]) | np.isfinite(st.X[bad, 1:]))  # an infinity: column 0 only
        assert st.n == 0 or st.finite_rows.size >= max(C.DENSE_KS)


def test_the_colbert_budget_holds_on_every_finite_state():
    Q = C.ms_queries()
    for st in C.ms_states():
        D, ptr = C.ms_store(st.docs)
        assert st.images == st.finite
        if st.finite:
            assert MS.same_scores(MS.split_expected(D, ptr, Q), MS.f32_expected(D, ptr, Q)), st.step
            assert np.abs(D).max() <= 56 and np.array_equal(D, np.rint(D))
        else:
            assert sum(not np.all(np.isfinite(d)) for d in st.docs) == 1, st.step

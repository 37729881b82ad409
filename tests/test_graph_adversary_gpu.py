"""Graph channel on the device (csrc/graph.hip) against the models of tests/graph_adversary.py: the score and top-k of
graph_score_select_kernel bit for bit on the exact and the float input family, amdr_graph_search_device against
amdr_graph_search, the walk of graph_walk_kernel at its LDS boundary, inside hub lists and over wide frontiers, the
limit-4096 launches, non-finite scores, and the reserve contract of the handle.  tests/test_graph_adversary.py checks on
the CPU that the cases hold what is claimed here."""
import numpy as np
import pytest

import graph_adversary as GA

pytestmark = pytest.mark.gpu

# every output buffer is filled with these before a call; amdr_graph_search copies its own device buffer over them, so an
# unwritten slot shows only through amdr_graph_search_device (device_search below), whose buffers are the caller's
SENT_I, SENT_F = -77, 1234.5


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    return _native


_worlds = {}


def world_of(d):
    if d not in _worlds:
        w = GA.score_world(d)
        _worlds[d] = (w, {})
    return _worlds[d]


def expected_of(d, c):
    w, cache = world_of(d)
    if c.name not in cache:
        cache[c.name] = GA.case_expected(w, c)
    return cache[c.name]


def sentinel_outputs(nat, nq, k):
    out = nat.GraphIndex._outputs(nq, k)
    for name, a in out.items():
        a.fill(SENT_F if a.dtype.kind == "f" else SENT_I)
    return out


def host_search(nat, g, dense, p, Q, seeds, seed_count, seed_n, k):
    hp, keep = GA.host_params(nat, p)
    out = g.search(dense, Q, seeds, seed_count, seed_n, k, hp, out=sentinel_outputs(nat, len(seed_count), k))
    del keep
    return out


def assert_no_sentinel(out, what):
    for name, a in out.items():
        assert not np.any(a == (SENT_F if a.dtype.kind == "f" else SENT_I)), (what, name)


# ---- 1. score and select, exact family ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", GA.D_GRID)
def test_score_select_bits_exact_family(nat, d):
    w, _ = world_of(d)
    g, dense = w.t.index(nat), nat.DenseIndex(w.X)
    checked = 0
    for c in w.cases:
        exp, _walks, _scored = expected_of(d, c)
        for k in GA.K_GRID:
            out = host_search(nat, g, dense, c.params, c.Q, c.seeds, c.seed_count, c.seed_n, k)
            assert_no_sentinel(out, (c.name, k))
            for q in range(len(c.seed_count)):
                GA.assert_outputs_equal(out, q, exp[k][q], (d, c.name, k, q))
                checked += 1
    assert checked == len(GA.K_GRID) * (len(GA.F_GRID) + 3 * len(GA.LIMIT_GRID))
    g.close()


# ---- 2. score and select, float family ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (256, 768))
def test_score_select_bits_float_family(nat, d):
    rng = np.random.default_rng(d)
    nq = 4
    t = GA.make_tables(rng, 3000, hubs={5: 600, 6: 257}, two_lang=True)
    n_dense = t.n_rows - 10
    Q = GA.unit_rows(rng, nq, d)
    X = np.concatenate([GA.unit_rows(rng, n_dense - nq, d), Q])  # every query is a row too: <q, q> from score_rows
    t.row_norm = np.ones(t.n_rows, np.float32)
    t.row_norm[:n_dense] = np.linalg.norm(X, axis=1)
    g, dense = t.index(nat), nat.DenseIndex(X)
    seeds = rng.integers(0, t.n_rows, size=(nq, 8)).astype(np.int64)
    seeds[0, 0], seeds[1, 1] = t.row_of(5), t.row_of(6)
    seed_count = np.array([8, 8, 8, 3], np.int32)
    X64, tol, hits = X.astype(np.float64), 2e-6, 0
    for limit, k in ((513, 64), (1024, 256), (80, 10), (4096, 255)):
        p = GA.make_params(limit, default_depth=3, rel_max_depth=[3, 2, 3, 4, 1, 3], lang=0 if limit == 80 else -1)
        out = host_search(nat, g, dense, p, Q, seeds, seed_count, 8, k)
        assert_no_sentinel(out, (limit, k))
        for q in range(nq):
            found = GA.walk_oracle(t, seeds[q, :seed_count[q]], p, False)
            rows = t.node_row[[f[0] for f in found]]
            safe = np.where((rows >= 0) & (rows < n_dense), rows, 0)
            dots = dense.score_rows(Q[q], safe)[0] if len(found) else np.zeros(0, np.float32)
            qq = dense.score_rows(Q[q], np.array([n_dense - nq + q]))[0, 0]
            exp = GA.score_oracle(t, X, Q[q], found, p, k, n_dense, dots=dots, qq=qq)
            GA.assert_outputs_equal(out, q, exp, (d, limit, k, q))
            # and the device's final against an fp64 evaluation of the same hit
            qn = np.linalg.norm(Q[q].astype(np.float64))
            for j in range(exp["count"]):
                r = int(out["rows"][q, j])
                sem = float(X64[r] @ Q[q].astype(np.float64)) / (qn * np.linalg.norm(X64[r]) + 1e-9)
                f64 = sem * p["decay"][out["depth"][q, j]] * p["rel_weight"][out["relation"][q, j]] * out["edge_conf"][q, j]
                assert abs(float(out["final"][q, j]) - f64) <= tol and abs(float(out["semantic"][q, j]) - sem) <= tol
                hits += 1
    assert hits > 1000
    g.close()


# ---- 3. search_device == search ----------------------------------------------------------------------------------------
def device_search(nat, g, dense, p, Q_t, qsel_t, seeds_t, cnt_t, seed_n, ng, k):
    """amdr_graph_search_device on torch tensors, outputs pre-filled with the sentinels -> (dict of numpy, growths)."""
    import torch
    dev = Q_t.device
    tabs = [torch.from_numpy(np.ascontiguousarray(p[n])).to(dev) for n in ("rel_max_depth", "rel_allowed", "rel_weight", "decay")]
    gp = nat.GraphParams(p["limit"], p["default_depth"], p["lang"], 0, p["min_conf"], *(x.data_ptr() for x in tabs))
    outs = {}
    for name, ty in zip(nat.GraphIndex.OUTS, nat.GraphIndex._OUT_T):
        tt = getattr(torch, np.dtype(ty).name)
        outs[name] = torch.full((ng,) if name == "count" else (ng, k), SENT_F if np.dtype(ty).kind == "f" else SENT_I,
                                dtype=tt, device=dev)
    g0 = nat.workspace_growths()
    g.search_device(dense, Q_t.data_ptr(), 0 if qsel_t is None else qsel_t.data_ptr(), seeds_t.data_ptr(), cnt_t.data_ptr(),
                    int(seeds_t.shape[1]), seed_n, ng, k, gp, [outs[n].data_ptr() for n in nat.GraphIndex.OUTS],
                    int(torch.cuda.current_stream().cuda_stream))
    grew = nat.workspace_growths() - g0  # read on the host before anything is synchronised
    torch.cuda.synchronize()
    del tabs
    return {n: v.cpu().numpy() for n, v in outs.items()}, grew


def assert_same_outputs(a, b, what):
    for name in GA.OUTS:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        if name in GA.BITS:
            x, y = x.view(GA.BITS[name]), y.view(GA.BITS[name])
        assert np.array_equal(x, y), (what, name)


def test_search_device_equals_search_on_qsel_and_seed_edges(nat):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(31)
    d, nqr, ld = 64, 6, GA.MAX_SEEDS
    t = GA.make_tables(rng, 3000, hubs={5: 300}, row_holes=0.1)
    n_dense = t.n_rows - 7
    X, Q = GA.exact_rows(rng, n_dense, d), GA.exact_queries(rng, nqr, d)
    g, dense = t.index(nat), nat.DenseIndex(X)
    seeds = rng.integers(0, 60, size=(nqr, ld)).astype(np.int64)          # 1 024 seeds, mostly duplicates
    seeds[5] = rng.integers(0, t.n_rows, size=ld)
    seeds[:, 0:3] = [-1, t.n_rows, int(np.nonzero(t.row_node < 0)[0][0])]  # dropped: outside [0, n_rows), no node
    seeds[3, 3] = seeds[4, 3] = t.row_of(5)
    seed_count = np.array([ld, 0, -3, 5, ld, 700], np.int32)
    Q_t, seeds_t, cnt_t = (torch.from_numpy(x).to(dev) for x in (Q, seeds, seed_count))
    dropped = 0
    for qsel in (None, [3, 3, 0], [5, 0, 2, 2, 4, 1, 3, 0, 5, 5, 2]):      # ng below and above the number of query rows
        sel = np.arange(nqr) if qsel is None else np.array(qsel)
        qsel_t = None if qsel is None else torch.tensor(qsel, dtype=torch.int32, device=dev)
        for seed_n, limit, k in ((ld, 800, 64), (4, 17, 10), (ld, 4096, 256), (0, 5, 1)):
            p = GA.make_params(limit, default_depth=3, rel_max_depth=[3, 2, 3, 4, 1, 3])
            got, _ = device_search(nat, g, dense, p, Q_t, qsel_t, seeds_t, cnt_t, seed_n, len(sel), k)
            exp = host_search(nat, g, dense, p, Q[sel], seeds[sel], seed_count[sel], seed_n, k)
            assert_same_outputs(got, exp, (qsel, seed_n, limit, k))
            for i, q in enumerate(sel):  # and both are the oracle's: the seed rules have an expectation of their own
                taken = seeds[q, :max(0, min(int(seed_count[q]), seed_n))]
                dropped += len(taken) - len(GA.seed_nodes(t, taken, False))
                found = GA.walk_oracle(t, taken, p, False)
                GA.assert_outputs_equal(got, i, GA.score_oracle(t, X, Q[q], found, p, k, n_dense), (qsel, seed_n, limit, k, i))
                if seed_count[q] <= 0 or seed_n == 0:
                    assert got["count"][i] == 0
    assert dropped > 20
    g.close()


# ---- 4. walk edges -----------------------------------------------------------------------------------------------------
def check_walk(nat, g, c):
    hp, keep = GA.host_params(nat, c.params)
    got = g.walk(c.seeds, hp)
    del keep
    for q, s in enumerate(c.seeds):
        exp = GA.walk_tuples(c.t, GA.walk_oracle(c.t, s, c.params, True))
        assert len(got[q]) == len(exp), (c.name, q, len(got[q]), len(exp))
        assert got[q] == exp, (c.name, q, next(i for i, (a, b) in enumerate(zip(got[q], exp)) if a != b))


def test_walk_at_the_lds_boundary_both_claim_slot_paths(nat):
    """12 288 interned ids: claim slots in LDS, with limit 4 096 and 1 024 seeds the 86 016-byte launch; 12 289: claim
    slots in the workspace.  One expectation for both."""
    t, t1 = GA.lds_boundary_tables()
    for tt in (t, t1):
        g = tt.index(nat)
        check_walk(nat, g, GA.lds_boundary_case(tt))
        g.close()


def test_walk_many_queries_per_claim_slot_set(nat):
    """300 queries in one call on the workspace path (256 claim-slot sets at most: blocks run a second query under a new
    epoch tag), then 300 others on the same handle."""
    _t, t1 = GA.lds_boundary_tables()
    g = t1.index(nat)
    for seed in (11, 12):
        check_walk(nat, g, GA.many_queries_case(t1, seed))
    g.close()


def test_walk_cuts_inside_a_hub_list(nat):
    t = GA.hub_tables()
    g = t.index(nat)
    for c in GA.hub_cases(t):
        check_walk(nat, g, c)
    g.close()


def test_walk_frontier_beyond_256_entries(nat):
    t = GA.fanout_tables()
    g = t.index(nat)
    check_walk(nat, g, GA.fanout_case(t))
    g.close()


# ---- 5. the limit-4096 launch of the score kernel ----------------------------------------------------------------------
def test_search_at_limit_4096(nat):
    """65 536 B of dynamic LDS plus the kernel's static words: the call must succeed and rank 4 096 found nodes."""
    d = 4
    w, _ = world_of(d)
    g, dense = w.t.index(nat), nat.DenseIndex(w.X)
    c = next(c for c in w.cases if c.name == "limit-4096")
    exp, walks, _ = expected_of(d, c)
    assert len(walks[0]) == 4096
    out = host_search(nat, g, dense, c.params, c.Q, c.seeds, c.seed_count, c.seed_n, 256)
    for q in range(len(c.seed_count)):
        GA.assert_outputs_equal(out, q, exp[256][q], (c.name, q))
    g.close()


# ---- 6. non-finite scores ----------------------------------------------------------------------------------------------
def assert_equal_nan_aware(got, qi, exp, what):
    """assert_outputs_equal, except that a NaN equals a NaN whatever its sign and payload."""
    g = {n: (v.copy() if n != "count" else v) for n, v in got.items()}
    e = dict(exp)
    for name in ("final", "semantic"):
        both = np.isnan(g[name][qi]) & np.isnan(e[name])
        assert np.array_equal(np.isnan(g[name][qi]), np.isnan(e[name])), (what, name)
        g[name][qi][both] = 0
        e[name] = np.where(both, 0, e[name]).astype(e[name].dtype)
    GA.assert_outputs_equal(g, qi, e, what)


def test_non_finite_scores_rank_last_and_every_hit_appears_once(nat):
    """A NaN final ranks behind every number (-inf included), NaN entries in walk order; +-inf order as numbers; every
    valid found node appears exactly once and count = min(valid, k)."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(17)
    d, k_grid = 8, (1, 10, 256)
    t = GA.make_tables(rng, 800, hubs={3: 300}, shared_rows=0, degrees=(0, 1, 2, 3))  # no two nodes on one row
    n_dense = t.n_rows
    seeds = np.array([[t.row_of(3)]], np.int64)
    X0 = GA.exact_rows(rng, n_dense, d, pool=40)
    q0 = np.zeros(d, np.float32)
    q0[[1, 3, 4, 7]] = [1, -1, 1, 1]
    g = t.index(nat)
    seeds_t, one_t = torch.from_numpy(seeds).to(dev), torch.ones(1, dtype=torch.int32, device=dev)
    seen_nan = seen_inf = 0
    for limit in (512, 200):  # more valid entries than the largest k, and fewer: the slots up to count - 1 are all written
        p = GA.make_params(limit, default_depth=2, rel_max_depth=[2] * GA.N_REL)
        found = GA.walk_oracle(t, seeds[0], p, False)
        rows = np.array([r for r in t.node_row[[f[0] for f in found]] if r >= 0])
        assert (len(rows) > 256) == (limit == 512) and len(rows) > 150
        cases = {}
        X = X0.copy()
        X[rows[5], 3] = np.nan                      # one NaN component in one walked row
        cases["nan-row"] = (X, q0)
        X = X0.copy()
        X[rows[::7], 3] = np.nan                    # NaN finals, and infinities of both signs among the numbers
        X[rows[1::7], 4] = np.inf
        X[rows[2::7], 4] = -np.inf
        cases["nan-and-inf-rows"] = (X, q0)
        q = q0.copy()
        q[4] = np.inf                               # <q, q> = inf: inf / inf
        cases["inf-query"] = (X0, q)
        q = q0.copy()
        q[0] = np.nan                               # every final is NaN: the list is the walk order
        cases["nan-query"] = (X0, q)
        for name, (X, q) in cases.items():
            dense = nat.DenseIndex(X)
            order, row, sem, final = GA.score_all(t, X, q, found, p, n_dense)
            seen_nan += int(np.isnan(final[order]).sum())
            seen_inf += int(np.isinf(final[order]).sum())
            if name == "nan-query":
                assert np.all(np.isnan(final[order])) and np.all(np.diff(order) > 0)
            for k in k_grid:
                out = host_search(nat, g, dense, p, q[None], seeds, np.array([1], np.int32), 1, k)
                assert_no_sentinel(out, (name, limit, k))
                c = int(out["count"][0])
                assert c == min(len(order), k), (name, limit, k, c)
                got_rows = out["rows"][0, :c].tolist()
                assert len(set(got_rows)) == c and min(got_rows) >= 0, (name, limit, k, "a hit twice")
                assert np.all(out["rows"][0, c:] == -1) and np.all(out["relation"][0, c:] == -1)
                exp = GA.cut_to_k(t, found, order, row, sem, final, k)
                assert_equal_nan_aware(out, 0, exp, (name, limit, k))
                # the host-pointer call copies an internal buffer out; the device call writes the caller's own,
                # sentinel-filled buffers: a slot the kernel skipped shows here
                dev_out, _ = device_search(nat, g, dense, p, torch.from_numpy(q[None].copy()).to(dev), None, seeds_t, one_t, 1, 1, k)
                assert_no_sentinel(dev_out, (name, limit, k, "device"))
                assert_equal_nan_aware(dev_out, 0, exp, (name, limit, k, "device"))
    assert seen_nan > 400 and seen_inf > 40
    g.close()


# ---- 7. the reserve contract -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("lds-claims", "workspace-claims"))
def test_reserved_handle_allocates_nothing(nat, which):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(23)
    t = GA.make_tables(rng, 3000, hubs={5: 1100}) if which == "lds-claims" else GA.lds_boundary_tables()[1]
    d, nq_max = 8, 64
    n_dense = t.n_rows - 3
    X, Q = GA.exact_rows(rng, n_dense, d), GA.exact_queries(rng, nq_max, d)
    seeds = rng.integers(0, t.n_rows, size=(nq_max, 6)).astype(np.int64)
    if t.hubs:
        seeds[::5, 0] = t.row_of(5)
    seed_count = rng.integers(0, 7, size=nq_max).astype(np.int32)
    seed_count[0] = 6
    g, dense = t.index(nat), nat.DenseIndex(X)
    g.reserve(nq_max=64, k_max=64, limit_max=1024)
    Q_t, seeds_t, cnt_t = (torch.from_numpy(x).to(dev) for x in (Q, seeds, seed_count))
    torch.cuda.synchronize()
    full = 0
    for ng in (1, 7, 64):
        for k in (1, 64):
            for limit in (1, 1000, 1024):
                p = GA.make_params(limit, default_depth=5, rel_max_depth=[5, 4, 5, 3, 5, 5])
                got, grew = device_search(nat, g, dense, p, Q_t, None, seeds_t, cnt_t, 6, ng, k)
                assert grew == 0, f"{which} ng={ng} k={k} limit={limit}: a call within the reserve (re)allocated {grew} buffer(s)"
                exp = host_search(nat, g, dense, p, Q[:ng], seeds[:ng], seed_count[:ng], 6, k)
                assert_same_outputs(got, exp, (which, ng, k, limit))
                full += int(limit >= 1000 and got["count"][0] == k)
    assert full >= 6  # the walks do fill the reserved lists
    g.close()

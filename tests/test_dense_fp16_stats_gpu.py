"""The statistics record behind both fp16 first passes of the dense channel (csrc/dense_fp16.hpp DenseFp16Stats): one
kernel computes it, the dense handle owns it and keeps it current across add(), the short-corpus first pass receives a
copy.  The per-query bound that DenseSmallApprox writes is the one public output that exposes the record (x_scale and
the largest row norm enter it), so it is compared with the fp64 restatement RA.dense_eps; the two readings of the
record — the large scan tolerates NaN rows, the short-corpus form does not — are checked through the routes."""
import numpy as np
import pytest

import rounding_adversary as RA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from legal_rag_amd import _native
    _native.load()
    return _native


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def _eps(nat, idx, n, Q):
    """The bounds of the short-corpus first pass over the handle's matrix as it is now."""
    import torch
    dev = torch.device("cuda", 0)
    nq = Q.shape[0]
    ap = nat.DenseSmallApprox(idx)
    try:
        ld = (n + 31) // 32 * 32
        S = torch.empty((nq, ld), dtype=torch.float32, device=dev)
        eps = torch.empty((nq,), dtype=torch.float32, device=dev)
        Qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
        ap.approx_device(Qd.data_ptr(), nq, S.data_ptr(), ld, eps.data_ptr(), int(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return eps.cpu().numpy().astype(np.float64)
    finally:
        ap.close()


def test_statistics_follow_add(nat):
    rng = np.random.default_rng(31)
    A, B = unit_rows(rng, 40, 128), unit_rows(rng, 24, 128) * np.float32(40.0)
    Q = unit_rows(rng, 8, 128)
    idx = nat.DenseIndex(A, device=0)
    idx.add(B)
    eps = _eps(nat, idx, 64, Q)
    idx.close()
    want, stale = RA.dense_eps(np.concatenate([A, B]), Q), RA.dense_eps(A, Q)
    print(f"OBS eps / expected {(eps / want).min():.8f}..{(eps / want).max():.8f}; expected / stale {(want / stale).min():.2f}")
    assert np.allclose(eps, want, rtol=1e-5, atol=0)


def test_second_grid_stride_round_and_last_row(nat):
    """8 200 rows: 8 more than one round of the statistics kernel's 2 048 blocks x 4 waves; the last row sets both maxima."""
    rng = np.random.default_rng(32)
    X, Q = unit_rows(rng, 8200, 128), unit_rows(rng, 8, 128)
    X[8199] *= np.float32(64.0)
    idx = nat.DenseIndex(X, device=0)
    eps = _eps(nat, idx, 8200, Q)
    idx.close()
    want = RA.dense_eps(X, Q)
    print(f"OBS eps / expected {(eps / want).min():.8f}..{(eps / want).max():.8f}")
    assert np.allclose(eps, want, rtol=1e-5, atol=0)


def test_one_record_two_readings(nat, monkeypatch):
    rng = np.random.default_rng(19)
    X, Q = unit_rows(rng, 9017, 128), unit_rows(rng, 33, 128)
    X[::7] = np.nan
    monkeypatch.setenv("AMDR_DENSE_HI", "1")
    monkeypatch.setenv("AMDR_DENSE_TWO_LEVEL", "1")
    idx = nat.DenseIndex(X, device=0)
    assert "dense_hi_tilemax_kernel" in idx.plan_info(33, 10), idx.plan_info(33, 10)  # NaN rows: the large scan takes them
    with pytest.raises(nat.NativeError):  # ... the short-corpus first pass does not
        _eps(nat, idx, 9017, Q)
    idx.close()
    monkeypatch.delenv("AMDR_DENSE_HI")
    monkeypatch.delenv("AMDR_DENSE_TWO_LEVEL")

    Q = unit_rows(rng, 96, 128)
    monkeypatch.setenv("AMDR_DENSE_SMALL_HI", "1")
    monkeypatch.setenv("AMDR_DENSE_SMALL_HI_MIN", "96")
    idx = nat.DenseIndex(unit_rows(rng, 64, 128), device=0)
    assert idx.plan_info(96, 5).startswith("dsh_scores_kernel"), idx.plan_info(96, 5)  # (a finite matrix of this shape does)
    idx.close()
    for bad in (np.nan, np.inf):
        Xs = unit_rows(rng, 64, 128)
        Xs[17, 5] = bad
        out = {}
        for small_hi in ("1", "0"):
            monkeypatch.setenv("AMDR_DENSE_SMALL_HI", small_hi)
            monkeypatch.setenv("AMDR_DENSE_SMALL_HI_MIN", "96")
            idx = nat.DenseIndex(Xs, device=0)
            plan = idx.plan_info(96, 5)  # before any search has run on the handle
            assert not plan.startswith("dsh_scores_kernel"), (bad, small_hi, plan)
            out[small_hi] = idx.search(Q, 5)
            idx.close()
        assert np.array_equal(out["1"][1], out["0"][1]), bad
        assert np.array_equal(out["1"][0].view(np.uint32), out["0"][0].view(np.uint32)), bad

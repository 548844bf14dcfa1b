"""-m gpu: the two device kernels that decode ANY slice through PsellSliceReader (csrc/psell_slice.hpp) -- psell_tile_body behind
polee_debug_loglik_force_mixed, em_g64_tiles_kernel behind the EM residual -- on one small matrix that fills every sliced stream,
against f64 NumPy on the dense matrix; without and with multiplicities, on the device-built and on the host-built layout.

The builder reads POLEE_DEVICE_BUILD once per process, so the host-built layout is checked by a child (this file run as a script:
one child for both of its cases)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 96
A1, A1M, A2, A2M, BN, B = range(6)


def make_matrix():
    """Rows in blocks, one per stream the builder is meant to choose for them (it chooses by cost: test_streams_are_populated).
    The mixed blocks are small against the rest: the device builder leaves a matrix whose mixed rows hold a tenth of the non-zeros
    to the host builder."""
    rng = np.random.default_rng(20)
    rows = []
    rows += [np.arange(0, 5)] * 128                                                    # A1: two full slices of one 5-set
    s12 = np.arange(12, 24)
    rows += [np.sort(rng.choice(s12, int(rng.integers(3, 7)), replace=False)) for _ in range(128)]      # A1M: subsets of a 12-set
    rows += [np.arange(24, 48)] * 512                                                  # A2: one 24-set
    s28 = np.arange(48, 76)
    rows += [np.sort(rng.choice(s28, int(rng.integers(4, 11)), replace=False)) for _ in range(64)]      # A2M: subsets of a 28-set
    assert np.unique(np.concatenate(rows[-64:])).size >= 17
    rows += [np.sort(rng.choice(N, int(rng.integers(3, 16)), replace=False)) for _ in range(70)]        # BN: unrelated rows
    rows += [np.sort(rng.choice(N, 40, replace=False)) for _ in range(6)]              # B: rows too long for any uniform slice
    rows += [np.array([int(rng.integers(0, N))]) for _ in range(200)]                  # S: one transcript
    rows += [np.zeros(0, np.int64)] * 3                                                # empty
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    m = len(rows)
    X = np.zeros((m, N), np.float32)
    for i, r in enumerate(rows):
        X[i, r] = np.exp(rng.normal(-9, 1.5, r.size)).astype(np.float32)
    colptr = np.concatenate([[0], np.cumsum((X != 0).sum(axis=0))]).astype(np.uint32) + np.uint32(1)
    ri, ci = np.nonzero(X.T)  # (by transcript, fragments ascending)
    return dict(m=m, n=N, X=X, colptr=colptr, rowval=(ci + 1).astype(np.uint32), nzval=X.T[ri, ci].astype(np.float32),
                ks=(1 + np.arange(m) % 5).astype(np.int64))


def truth(X, ks, x):
    """lp = sum_i ks_i log (X x)_i, g = X^T (ks / (X x)) in f64, empty rows aside."""
    X = X.astype(np.float64)
    p = X @ x.astype(np.float64)
    live = p > 0
    w = np.where(live, ks / np.where(live, p, 1.0), 0.0)
    return float((ks[live] * np.log(p[live])).sum()), X.T @ w


def check_decoders(P, ctx, mat, with_ks, device_built):
    from polee_amd import _lib as L
    from polee_amd.em import EM
    ks = mat["ks"] if with_ks else None
    ksf = mat["ks"].astype(np.float64) if with_ks else np.ones(mat["m"])
    s = P.RNASeqSample(mat["m"], mat["n"], mat["colptr"], mat["rowval"], mat["nzval"], ks=ks, ctx=ctx)
    assert bool(s.built_on_device) == device_built
    nnz = s.info["stream_nnz"]
    assert all(nnz[q] > 0 for q in (A1, A1M, A2, A2M, BN, B)), nnz
    rng = np.random.default_rng(5)
    # psell_tile_body over every slice; tolerances: tests/test_gpu_parity.py's against f64 NumPy (lp 1e-6, gradient rtol 3e-5 +
    # 1e-7 of its maximum)
    L.check(L.lib().polee_debug_loglik_force_mixed(s._h, 1))
    try:
        for K in (1, 6):
            x = np.clip(rng.dirichlet(np.ones(N), size=K), 1e-10, 1).astype(np.float32)
            lp, g = s.log_likelihood(x) if ks is None else P.factored_log_likelihood(s, x)
            for k in range(K):
                lp0, g0 = truth(mat["X"], ksf, x[k])
                print("ks %d K %d draw %d: lp rel. error %.3g, gradient max rel. error %.3g" % (
                    with_ks, K, k, abs(lp[k] - lp0) / abs(lp0), np.max(np.abs(g[k] - g0) / np.maximum(np.abs(g0), 1e-7 * g0.max()))))
                assert abs(lp[k] - lp0) <= 1e-6 * abs(lp0), (K, k, lp[k], lp0)
                np.testing.assert_allclose(g[k], g0, rtol=3e-5, atol=1e-7 * g0.max())
    finally:
        L.check(L.lib().polee_debug_loglik_force_mixed(s._h, 0))
    # em_g64_tiles_kernel: the fixed-point residual at the uniform start, as tests/test_gpu_em.py test_residual_of_early_iterates
    em = EM(s)
    got = em.info(kkt=True)["kkt_max"]
    y = em.mixture().astype(np.float64)
    y /= y.sum()
    want = float(np.max(y * np.abs(truth(mat["X"], ksf, y)[1] / ksf[(mat["X"] != 0).any(axis=1)].sum() - 1)))
    print("ks %d: kkt_max device %.9g, NumPy %.9g" % (with_ks, got, want))
    assert abs(got - want) <= 1e-3 * want, (got, want)


def test_streams_are_populated():
    """The builder chooses streams by cost: the matrix above must put non-zeros into all six sliced streams (no GPU needed)."""
    from test_layouts import _psell
    mat = make_matrix()
    for ks in (None, mat["ks"]):
        nnz = _psell(mat["m"], mat["n"], mat["colptr"], mat["rowval"], mat["nzval"], ks=ks)["stream_nnz"]
        assert all(nnz[q] > 0 for q in (A1, A1M, A2, A2M, BN, B)), nnz
        assert nnz[BN] + nnz[B] < 0.08 * sum(nnz), nnz  # (the device builder takes it)


@pytest.fixture(scope="module")
def host_child():
    """Both cases on the host-built layout, in one child process."""
    return subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, POLEE_DEVICE_BUILD="0"), cwd=ROOT,
                          capture_output=True, text=True, timeout=300)


@pytest.mark.gpu
@pytest.mark.parametrize("with_ks", [0, 1])
def test_decoders_on_the_device_built_layout(with_ks):
    import polee_amd as P
    check_decoders(P, P.Context(0), make_matrix(), with_ks, True)


@pytest.mark.gpu
@pytest.mark.parametrize("with_ks", [0, 1])
def test_decoders_on_the_host_built_layout(host_child, with_ks):
    print(host_child.stdout)
    assert "host-built, ks %d: ok" % with_ks in host_child.stdout, host_child.stdout[-2000:] + host_child.stderr[-4000:]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import polee_amd as P
    ctx = P.Context(0)
    for with_ks in (0, 1):
        try:
            check_decoders(P, ctx, make_matrix(), with_ks, False)
            print("host-built, ks %d: ok" % with_ks)
        except AssertionError:
            import traceback
            traceback.print_exc()

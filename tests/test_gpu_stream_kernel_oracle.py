"""-m gpu: the streaming kernel in its DEFAULT mode (float atomics, dynamic schedule) against the float64 oracle: the
reference's fixture at every number of draws K = 1 .. 8 (each K is its own kernel instance), and a synthetic sample of
several hundred tiles that holds all five kinds of stream the persistent launch walks -- dense narrow (A1), masked narrow
(A1M), dense wide (A2), masked wide (A2M) and mixed narrow (BN) -- so that every slice loop, its ring refills and its
counted waits are exercised.  Tolerances of tests/test_gpu_configs.py: lp 1e-6 relative; gradient 1e-4 relative + 1e-6 of
the largest entry."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


def check(lp, g, so, x, what, ks=None):
    worst = 0.0
    for k in range(x.shape[0]):
        lpo, go = so.log_likelihood(x[k]) if ks is None else so.factored_log_likelihood(ks, x[k])
        scale = np.abs(go).max()
        err_lp = abs(lp[k] - lpo) / abs(lpo)
        err_g = float((np.abs(g[k] - go) / (np.abs(go) + 1e-2 * scale)).max())
        worst = max(worst, err_g)
        print("%s draw %d: lp rel err %.3g, worst weighted gradient err %.3g" % (what, k, err_lp, err_g))
        assert err_lp <= 1e-6, (what, k, lp[k], lpo)
        np.testing.assert_allclose(g[k], go, rtol=1e-4, atol=1e-6 * scale)
    return worst


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_fixture_matches_oracle_at_every_number_of_draws(P, lm_fixture, K):
    f = lm_fixture
    m, n = f["m"], f["n"]
    ctx = P.Context(0)
    s = P.RNASeqSample(m, n, f["colptr"], f["rowval"], f["nzval"], f["effective_lengths"], ctx=ctx)
    so = O.Sample(m, n, f["colptr"], f["rowval"], f["nzval"])
    x = np.random.default_rng(K).dirichlet(np.ones(n), size=K).astype(np.float32)
    x = np.clip(x, np.float32(1e-10), 1)
    lp, g = s.log_likelihood(x)
    check(lp, g, so, x, "fixture K=%d" % K)
    lp2, g2 = s.log_likelihood(x)  # a second launch on the same handle (the ticket counter runs on)
    check(lp2, g2, so, x, "fixture K=%d again" % K)


# The small sample: the smallest of synth.make_sample(n, 75 n, 14.0, seed=7, dropout=0.3), n = 200, 250, .. (the large one's
# proportions), whose layout has a tile of every one of the five kinds, with and without multiplicities.  It was FOUND with the
# host builder (the layout view of tests/test_layouts.py: tiles per kind 4, 3, 1, 1, 1; with multiplicities 5, 2, 1, 1, 1); the
# test itself builds through the default path, the device builder, which makes the same layout byte for byte
# (tests/test_gpu_device_build.py) -- the assertion on the tiles per kind below holds for whichever builder ran.  The cases beside
# the large one cover what the slice loops' shared blocks are templated over: one and two draw groups (K <= 4, K > 4), both
# forms of lp (the mantissa product; with multiplicities the sum of ks log2 s) and both targets of a tile's flush (float atomics;
# the deterministic mode's windows).
SMALL = (300, 22500)


@pytest.mark.parametrize("n,m,K,with_ks,deterministic,min_tiles", [
    pytest.param(20000, 1500000, 6, False, False, 200, id="K6"),
    pytest.param(*SMALL, 3, True, False, 5, id="K3-multiplicities"),
    pytest.param(*SMALL, 8, False, True, 5, id="K8-deterministic"),
    pytest.param(*SMALL, 4, True, True, 5, id="K4-multiplicities-deterministic"),
])
def test_sample_with_all_five_stream_kinds_matches_oracle(P, n, m, K, with_ks, deterministic, min_tiles):
    from tools import synth
    smp = synth.make_sample(n, m, 14.0, seed=7, dropout=0.3)
    ks = np.random.default_rng(5).integers(1, 6, m).astype(np.int64) if with_ks else None
    ctx = P.Context(0)
    s = P.RNASeqSample(m, n, None, None, None, smp["effective_lengths"], ks=ks, ctx=ctx,
                       xt=(smp["tcolptr"], smp["trowval"], smp["tnzval"]))
    tiles = list(s.info["stream_tiles"])[:6]
    print("tiles per stream (A1, A1M, A2, A2M, BN, B):", tiles)
    assert all(t > 0 for t in tiles[:5]), tiles
    assert sum(tiles[:5]) >= min_tiles, tiles
    colptr, rowval, nzval = synth.to_csc(smp)
    so = O.Sample(m, n, colptr, rowval, nzval)
    O.set_num_threads(O.physical_cores())
    x = np.random.default_rng(2).gamma(0.3, size=(K, n)).astype(np.float32) + np.float32(1e-7)
    x /= x.sum(axis=1, keepdims=True)
    x = np.clip(x, np.float32(1e-10), 1)
    if deterministic:
        s.set_deterministic(True)
    lp, g = s.log_likelihood(x)
    check(lp, g, so, x, "five kinds", ks=ks)
    if deterministic:  # fixed-order sums: a second evaluation agrees bit for bit
        lp2, g2 = s.log_likelihood(x)
        assert np.array_equal(lp, lp2) and np.array_equal(g, g2)

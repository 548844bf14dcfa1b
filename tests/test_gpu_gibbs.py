"""The Gibbs sampler on the GPU (csrc/gibbs.hip, polee_amd.gibbs; `polee debug-sample`, src/gibbs.jl): the conjugate case
against Dirichlet marginals, tiny problems against their exact posteriors, the assignment kernel against the NumPy restatement
of tests/test_gibbs_host.py draw for draw, bitwise reproducibility, the real fixture against the restatement and against fitted
approximations, a C2-sized run, and the argument checks."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT  # noqa: F401
from test_gibbs_host import (Layout, NumpyGibbs, assign, batch_means_se, exact_moments, rows_of, tiny_problem)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def ctx(P):
    return P.Context(0)


def _sampler(P, ctx, lm, C=8, seed=11, efflen=True, **kw):
    from polee_amd.gibbs import GibbsSampler
    return GibbsSampler(lm["m"], lm["n"], lm["colptr"], lm["rowval"], lm["nzval"], lm["effective_lengths"] if efflen else None,
                        C, seed, ctx=ctx, **kw)


def _xt(lm):
    indptr, col, val = rows_of(lm["m"], lm["n"], lm["colptr"], lm["rowval"], lm["nzval"])
    return indptr.astype(np.uint64) + 1, (col + 1).astype(np.uint32), val


# ---- 1. conjugate case -----------------------------------------------------------------------------------------------------------
def test_conjugate_dirichlet_marginals(P, ctx):
    from scipy import stats
    from polee_amd.gibbs import GibbsSampler
    cs = np.array([0, 50, 1_000_000, 3, 20_000, 0, 700], np.int64)
    n, m = cs.size, int(cs.sum())
    colptr = np.concatenate([[1], 1 + np.cumsum(cs)]).astype(np.uint64)
    rowval = np.arange(1, m + 1, dtype=np.uint32)
    C, S = 32, 640
    g = GibbsSampler(m, n, colptr, rowval, np.ones(m, np.float32), None, C, 5, ctx=ctx)
    g.reserve(S)
    g.run(S, 1)
    g.sync()
    counts = g.get_counts()
    assert (counts == cs[None, :].astype(np.uint32)).all()
    x = g.get_draws().reshape(C * S, n).astype(np.float64)
    assert np.allclose(x.sum(axis=1), 1, atol=1e-5)
    a = 1.0 + cs
    A = a.sum()
    mean = a / A
    var = a * (A - a) / (A * A * (A + 1))
    N = x.shape[0]
    for j in range(n):
        se_m = np.sqrt(var[j] / N)
        assert abs(x[:, j].mean() - mean[j]) < 5 * se_m, (j, x[:, j].mean(), mean[j])
        d2 = (x[:, j] - mean[j]) ** 2
        assert abs(d2.mean() - var[j]) < 5 * d2.std() / np.sqrt(N), (j, d2.mean(), var[j])
    for j in (0, 1, 2):  # c = 0, 50, 1e6 (the f64 acceptance test's guard)
        p = stats.kstest(x[:, j], stats.beta(a[j], A - a[j]).cdf).pvalue
        assert p > 1e-3, (j, p)


# ---- 2. exact posterior, non-conjugate -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(2, 300), (3, 200)])
def test_exact_posterior_non_conjugate(P, ctx, n, m):
    from polee_amd.gibbs import GibbsSampler
    Xd, colptr, rowval, nzval = tiny_problem(n, m, seed=10 + n)
    C, S, thin = 32, 100, 50
    g = GibbsSampler(m, n, colptr, rowval, nzval, None, C, 17, ctx=ctx)
    g.reserve(S)
    g.run(500, 0)
    g.run(S * thin, thin)
    x = g.get_draws().astype(np.float64)  # [C, S, n]
    mean, var = exact_moments(Xd, n, grid=400 if n == 2 else 600)
    for j in range(n):
        se_m = batch_means_se(x[:, :, j], 10)
        d2 = (x[:, :, j] - mean[j]) ** 2
        se_v = batch_means_se(d2, 10)
        assert abs(x[:, :, j].mean() - mean[j]) < 5 * se_m, (j, x[:, :, j].mean(), mean[j], se_m)
        assert abs(d2.mean() - var[j]) < 5 * se_v, (j, d2.mean(), var[j], se_v)


# ---- 3. assignment kernel against the restatement ------------------------------------------------------------------------------
def test_assignments_match_restatement_draw_for_draw(P, ctx, lm_fixture):
    lm = lm_fixture
    m, n = lm["m"], lm["n"]
    lay = Layout(m, n, *rows_of(m, n, lm["colptr"], lm["rowval"], lm["nzval"]))
    C, seed = 8, 2024
    g = _sampler(P, ctx, lm, C=C, seed=seed)
    rng = np.random.default_rng(1)
    g0 = rng.gamma(0.5, size=(C, n)).astype(np.float32) * np.float32(100)
    g0[:, ::17] = 0  # (rows whose weights are all zero pick their first entry)
    g.set_state(g0)
    g.run(1, 0)
    g.sync()
    assert g.info["sweeps_done"] == 1
    picks, margin = assign(lay, g0, seed, 1)
    empty = np.ones(m, bool)
    empty[lay.rows] = False
    empty[lay.single_rows] = False
    for c in range(C):
        z = g.debug_assignments(c)
        assert (z[lay.single_rows] == lay.single_col + 1).all()
        assert (z[empty] == 0).all()
        bad = np.flatnonzero(z[lay.rows] != picks[c] + 1)
        assert bad.size <= 1e-4 * lay.rows.size, (c, bad.size)
        assert (margin[c, bad] <= 1e-5).all(), margin[c, bad]
    counts = g.get_counts().astype(np.int64)
    assert (counts.sum(axis=1) == lay.num_nonempty).all()
    assert (counts >= lay.base[None, :]).all()


# ---- 4. reproducibility -------------------------------------------------------------------------------------------------------
def _run(g, S=4, stride=7):
    g.reserve(S)
    g.run(30, 0)
    g.run(S * stride, stride)
    g.sync()
    return g.get_draws()


def test_bitwise_reproducible(P, ctx, lm_fixture):
    lm = lm_fixture
    a = _run(_sampler(P, ctx, lm, C=8, seed=99))
    b = _run(_sampler(P, ctx, lm, C=8, seed=99))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    c = _run(_sampler(P, ctx, lm, C=8, seed=100))
    assert not np.array_equal(a, c)
    one = _run(_sampler(P, ctx, lm, C=1, seed=99))
    assert np.array_equal(one[0].view(np.uint32), a[0].view(np.uint32))
    xt = _run(_sampler(P, ctx, lm, C=8, seed=99, xt=_xt(lm)))
    assert np.array_equal(xt.view(np.uint32), a.view(np.uint32))
    # rows out of order in the fragment-major input give the same layout
    tp, tr, tv = _xt(lm)
    tr2, tv2 = tr.copy(), tv.copy()
    for i in range(0, lm["m"], 3):
        s0, s1 = int(tp[i]) - 1, int(tp[i + 1]) - 1
        tr2[s0:s1], tv2[s0:s1] = tr[s0:s1][::-1], tv[s0:s1][::-1]
    rev = _run(_sampler(P, ctx, lm, C=8, seed=99, xt=(tp, tr2, tv2)))
    assert np.array_equal(rev.view(np.uint32), a.view(np.uint32))


# ---- 5. against the restatement, statistically --------------------------------------------------------------------------------
def test_fixture_posterior_matches_restatement(P, ctx, lm_fixture):
    lm = lm_fixture
    m, n = lm["m"], lm["n"]
    lay = Layout(m, n, *rows_of(m, n, lm["colptr"], lm["rowval"], lm["nzval"]))
    C, thin = 8, 5
    g = _sampler(P, ctx, lm, C=C, seed=7, efflen=False)
    g.reserve(400)
    g.run(500, 0)
    g.run(400 * thin, thin)
    xg = g.get_draws().astype(np.float64)  # [C, 400, n]
    s = NumpyGibbs(lay, C, seed=12345)
    burn, keep = 200, 800
    xn = np.empty((C, keep // thin, n))
    for t in range(burn + keep):
        s.step()
        if t >= burn and (t - burn) % thin == thin - 1:
            xn[:, (t - burn) // thin] = s.x()
    mg, mn = xg.mean(axis=(0, 1)), xn.mean(axis=(0, 1))
    vg, vn = xg.var(axis=(0, 1)), xn.var(axis=(0, 1))
    sel = np.flatnonzero(np.maximum(mg, mn) >= 1e-4)
    assert sel.size > 100
    bad = []
    for j in sel:
        se = np.hypot(batch_means_se(xg[:, :, j], 10), batch_means_se(xn[:, :, j], 8))
        sev = np.hypot(batch_means_se((xg[:, :, j] - mg[j]) ** 2, 10), batch_means_se((xn[:, :, j] - mn[j]) ** 2, 8))
        if abs(mg[j] - mn[j]) > 5 * se or abs(vg[j] - vn[j]) > 5 * sev:
            bad.append((int(j), mg[j], mn[j], vg[j], vn[j]))
    assert not bad, bad


# ---- 6. against the fitted approximations ----------------------------------------------------------------------------------------
def _agreement(gibbs_mean, approx_mean, band, floor=1e-4):
    from scipy import stats
    sel = gibbs_mean >= floor
    rho = stats.spearmanr(np.log(gibbs_mean[sel]), np.log(approx_mean[sel])).correlation
    inside = ((gibbs_mean[sel] >= band[0][sel]) & (gibbs_mean[sel] <= band[1][sel])).mean()
    return rho, inside, int(sel.sum())


def test_gibbs_posterior_against_fitted_approximations(P, ctx, lm_fixture, prep_fixture):
    lm, pr = lm_fixture, prep_fixture
    g = _sampler(P, ctx, lm, C=16, seed=3, efflen=False)
    g.reserve(300)
    g.run(1000, 0)
    g.run(300 * 5, 5)
    gm = g.get_draws().astype(np.float64).mean(axis=(0, 1))
    t = P.PolyaTreeTransform(pr["node_parent_idxs"], pr["node_js"], ctx=ctx)
    fits = {"reference": (pr["mu"], pr["omega"], pr["alpha"])}
    s = P.RNASeqSample(lm["m"], lm["n"], lm["colptr"], lm["rowval"], lm["nzval"], lm["effective_lengths"], ctx=ctx)
    own = P.approximate_likelihood(P.LogitSkewNormalPTTApprox(), s, t)
    fits["own"] = (own["mu"], own["omega"], own["alpha"])
    lines = []
    for name, (mu, omega, alpha) in fits.items():
        als = P.ApproxLikelihoodSampler()
        als.set_transform(t, mu, np.exp(np.asarray(omega, np.float64)).astype(np.float32), alpha)
        band = als.quantile((0.01, 0.99), N=4000).astype(np.float64)
        pm = als.posterior_mean(N=4000).astype(np.float64)
        rho, inside, k = _agreement(gm, pm, band)
        lines.append("%s: spearman %.4f, inside 1-99%% band %.4f over %d transcripts" % (name, rho, inside, k))
        assert rho >= 0.98 and inside >= 0.95, lines
    print("\n".join(lines))


# ---- 7. full size ----------------------------------------------------------------------------------------------------------------
def test_c2_full_size(P, ctx):
    from tools import synth
    from polee_amd.gibbs import GibbsSampler
    N, M = 200_000, 30_000_000
    smp = synth.make_sample(N, M, 8.0, seed=123456789, literal=True)
    g = GibbsSampler(M, N, None, None, None, smp["effective_lengths"], 8, 1, ctx=ctx,
                     xt=(smp["tcolptr"], smp["trowval"], smp["tnzval"]))
    info = g.info
    nonempty = M - info["num_empty_rows"]
    assert info["num_multi_rows"] + info["num_single_rows"] == nonempty
    g.reserve(2)
    g.run(20, 10)
    g.sync()  # (no POLEE_ERR_NONFINITE)
    counts = g.get_counts().astype(np.int64)
    assert (counts.sum(axis=1) == nonempty).all()
    x = g.get_draws()
    assert x.shape == (8, 2, N) and np.isfinite(x).all() and (x >= 0).all()
    assert np.allclose(x.astype(np.float64).sum(axis=2), 1, atol=1e-5)


# ---- 8. argument rejection -------------------------------------------------------------------------------------------------------
def test_argument_rejection(P, ctx, lm_fixture):
    from polee_amd import PoleeError
    lm = lm_fixture
    for C in (0, 33):
        with pytest.raises(PoleeError, match="num_chains") as e:
            _sampler(P, ctx, lm, C=C)
        assert e.value.status == 1
    for bad in (0.0, -1.0, np.inf):
        el = lm["effective_lengths"].astype(np.float32).copy()
        el[5] = bad
        with pytest.raises(PoleeError, match="effective length") as e:
            _sampler(P, ctx, dict(lm, effective_lengths=el))
        assert e.value.status == 1
    g = _sampler(P, ctx, lm, C=2)
    with pytest.raises(PoleeError, match="stride < 0") as e:
        g.run(3, -1)
    assert e.value.status == 1
    with pytest.raises(PoleeError, match="no store reserved") as e:
        g.run(3, 1)
    assert e.value.status == 1
    g.reserve(2)
    with pytest.raises(PoleeError, match="do not fit") as e:
        g.run(3, 1)
    assert e.value.status == 1
    g.run(2, 1)
    assert g.num_stored == 2


# ---- CLI ---------------------------------------------------------------------------------------------------------------------
def test_cli_writes_kallisto_file_and_convergence_csv(P, tmp_path):
    import subprocess
    import sys
    from polee_amd import h5io
    out = str(tmp_path / "g.h5")
    lm = os.path.join(GOLDEN, "mBr_M_6w_1.likelihood-matrix.h5")
    subprocess.check_call([sys.executable, "-m", "polee_amd.gibbs", lm, "-o", out, "--kallisto", "--num-samples", "64",
                           "--burnin", "100", "--stride", "10", "--chains", "8"], cwd=ROOT, timeout=300)
    with h5io.File(out) as f:
        n = f.dataset_kind("est_counts")[2][0]
        assert n == 313
        assert f.read("aux/num_bootstrap", np.int64)[0] == 64
        assert f.read_strings("aux/ids") == [str(j) for j in range(1, n + 1)]
        assert (f.read("aux/lengths", np.int64) == -1).all()
        assert f.read_strings("aux/kallisto_version") == "polee debug-sample"
        assert f.exists("bootstrap/bs63") and not f.exists("bootstrap/bs64")
        assert abs(f.read("est_counts", np.float64).sum() - 19743) < 1e-6 * 19743
    lines = open(out + ".convergence.csv").read().splitlines()
    assert len(lines) == 1  # 10 * 8 = 80 sweeps: one (partial) checkpoint of 125
    r = np.array([float(v) for v in lines[0].split(",")])
    assert r.size == 313 and np.isfinite(r).mean() > 0.9

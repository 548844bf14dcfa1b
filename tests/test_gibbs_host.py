"""CPU tests of the Gibbs sampler's host side (no GPU): a NumPy restatement of generate_gibbs_sample, rand_gamma and
convergence_stats (src/gibbs.jl:180-319) with the device's Philox4x32-10 keying (csrc/rng.hpp, csrc/gibbs.hip),
validated against exact posteriors of tiny problems; the kallisto and CSV writers of polee_amd.gibbs read back through h5io.
tests/test_gpu_gibbs.py compares the GPU sampler with this restatement."""
import os

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401

MASK = np.uint64(0xFFFFFFFF)
TAG_ASSIGN, TAG_GAMMA, TAG_INIT = 1 << 24, 2 << 24, 3 << 24


# ---- restatement -------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, seed):
    """rng.hpp philox4x32_10, vectorised: four uint32 counter words (broadcast) -> four uint32 arrays."""
    c = [np.asarray(x).astype(np.uint64) & MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def u01f(w):
    return ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def u01d(w):
    return ((w >> np.uint32(8)).astype(np.float64) + 0.5) * (1.0 / 16777216.0)


def rows_of(m, n, colptr, rowval, nzval):
    """X by columns (1-based, the HDF5 form) -> fragment-major rows with ascending transcripts: (indptr, col 0-based, val f32)."""
    colptr = np.asarray(colptr, np.int64) - 1
    rowval = np.asarray(rowval, np.int64) - 1
    col = np.repeat(np.arange(n, dtype=np.int64), np.diff(colptr))
    order = np.lexsort((col, rowval))
    indptr = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(rowval, minlength=m), out=indptr[1:])
    return indptr, col[order], np.asarray(nzval, np.float32)[order]


class Layout:
    """The sampler's split of X (gibbs.hip gb_build): single-transcript fragments -> base counts, empty ones dropped, the rest
    padded to the longest row for vectorised sequential f32 sums."""

    def __init__(self, m, n, indptr, col, val):
        self.m, self.n = m, n
        lens = np.diff(indptr)
        single = np.flatnonzero(lens == 1)
        self.base = np.bincount(col[indptr[single]], minlength=n).astype(np.int64)
        self.num_nonempty = int((lens > 0).sum())
        self.single_rows, self.single_col = single, col[indptr[single]]
        self.rows = np.flatnonzero(lens >= 2)
        L = int(lens[self.rows].max()) if self.rows.size else 0
        self.L = L
        R = self.rows.size
        self.len = lens[self.rows]
        self.pcol = np.zeros((R, L), np.int64)
        self.pval = np.zeros((R, L), np.float32)
        for l in range(L):
            has = self.len > l
            self.pcol[has, l] = col[indptr[self.rows[has]] + l]
            self.pval[has, l] = val[indptr[self.rows[has]] + l]


def assign(lay, g, seed, sweep, chains=None):
    """The assignment step of generate_gibbs_sample (gibbs.jl:182-210) as gb_assign_kernel computes it: w_l = X_il g_j in f32,
    sequential f32 running sums, r = u sum w with u from Philox (original fragment, chain, sweep, TAG_ASSIGN), the first l with
    r <= running sum (the first entry when every weight is 0).  g [C, n] -> picks [C, R] (0-based transcripts), and the
    margins |r - running sum| / sum w of every pick (how close to a tie it was)."""
    C = g.shape[0]
    chains = np.arange(C) if chains is None else np.asarray(chains)
    R, L = lay.pcol.shape
    picks = np.empty((C, R), np.int64)
    margin = np.empty((C, R), np.float64)
    if R == 0:
        return picks, margin
    for ci, c in enumerate(chains):
        w = lay.pval * g[ci][lay.pcol]  # f32 products
        w[np.arange(L)[None, :] >= lay.len[:, None]] = 0
        s = np.zeros(R, np.float32)
        for l in range(L):
            s = s + w[:, l]
        u = u01f(philox4x32_10(lay.rows.astype(np.uint32), np.uint32(c), np.uint32(sweep), np.uint32(TAG_ASSIGN), seed)[0])
        rr = u * s
        cs = np.zeros(R, np.float32)
        pick = lay.pcol[:, 0].copy()
        mg = np.full(R, np.inf)
        done = np.zeros(R, bool)
        for l in range(L):
            cs = cs + w[:, l]
            valid = lay.len > l
            hit = valid & ~done & (rr <= cs)
            pick[hit] = lay.pcol[hit, l]
            done |= hit
            near = valid & (s > 0)
            mg[near] = np.minimum(mg[near], np.abs(rr[near].astype(np.float64) - cs[near]) / s[near])
        picks[ci] = pick
        margin[ci] = mg
    return picks, margin


def rand_gamma(a, seed, js, chains, sweep, tag):
    """rand_gamma (gibbs.jl:245-280) for shapes a >= 1 as gb_gamma draws it: one Philox block (j, chain, sweep, tag | attempt)
    per attempt, a Box-Muller normal from words 0-1, the acceptance uniform from word 2, shape constants and the test in f64."""
    a = np.asarray(a, np.float64)
    d = a - 1.0 / 3.0
    cc = 1.0 / np.sqrt(9.0 * d)
    out = np.full(a.shape, np.nan)
    pending = np.ones(a.shape, bool)
    js, chains = np.broadcast_to(js, a.shape), np.broadcast_to(chains, a.shape)
    attempt = 0
    while pending.any():
        idx = np.nonzero(pending)
        w = philox4x32_10(js[idx], chains[idx], np.uint32(sweep), np.uint32(tag | attempt), seed)
        u1, u2, u = u01d(w[0]), u01d(w[1]), u01d(w[2])
        x = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
        v = 1.0 + cc[idx] * x
        ok = v > 0
        v3 = np.where(ok, v, 1.0) ** 3
        xsq = x * x
        acc = ok & ((u < 1.0 - 0.0331 * xsq * xsq) | (np.log(u) < 0.5 * xsq + d[idx] * (1.0 - v3 + np.log(v3))))
        sel = tuple(i[acc] for i in idx)
        out[sel] = d[sel] * v3[acc]
        pending[sel] = False
        attempt += 1
    return out.astype(np.float32)


class NumpyGibbs:
    """generate_gibbs_sample (gibbs.jl:180-240) for C chains with the device's keying: a chain's state g [n] stays
    unnormalised, as on the device."""

    def __init__(self, lay, C, seed, chains=None):
        self.lay, self.C, self.seed = lay, C, seed
        self.chains = np.arange(C) if chains is None else np.asarray(chains)
        n = lay.n
        self.g = rand_gamma(np.ones((C, n)), seed, np.arange(n)[None, :], self.chains[:, None], 0, TAG_INIT)
        self.sweep = 0
        self.counts = np.zeros((C, n), np.int64)

    def step(self):
        self.sweep += 1
        lay = self.lay
        picks, _ = assign(lay, self.g, self.seed, self.sweep, self.chains)
        counts = np.stack([np.bincount(p, minlength=lay.n) for p in picks]) if picks.shape[1] else np.zeros((self.C, lay.n), np.int64)
        self.counts = counts + lay.base[None, :]
        self.g = rand_gamma(1.0 + self.counts, self.seed, np.arange(lay.n)[None, :], self.chains[:, None], self.sweep, TAG_GAMMA)

    def x(self, efflens=None):
        g = self.g.astype(np.float64)
        if efflens is not None:
            g = g / np.asarray(efflens, np.float64)[None, :]
        return g / g.sum(axis=1, keepdims=True)


def convergence_stats(samples, sample_count):
    """convergence_stats (gibbs.jl:283-319) as written: samples [C, S, n] -> R [n] over the first sample_count draws."""
    C = samples.shape[0]
    k = sample_count // 2
    mid = (sample_count + 1) // 2
    halves = [samples[:, :mid, :].astype(np.float64), samples[:, mid:sample_count, :].astype(np.float64)]
    means = np.concatenate([h.mean(axis=1) for h in halves])  # [2C, n]
    total = means.mean(axis=0)
    B = (k / (2 * C - 1)) * ((means - total) ** 2).sum(axis=0)
    variances = np.concatenate([((h - h.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / k for h in halves])
    W = variances.sum(axis=0) / (2 * C)
    var = ((k - 1) / k) * W + (1 / k) * B
    return np.sqrt(var / W)


def batch_means_se(draws, nbatch=20):
    """draws [C, S] (independent chains) -> standard error of the overall mean by batch means within each chain."""
    C, S = draws.shape
    b = S // nbatch
    bm = draws[:, :b * nbatch].reshape(C, nbatch, b).mean(axis=2).ravel()
    return bm.std(ddof=1) / np.sqrt(bm.size)


def exact_moments(Xrows, n, grid=400):
    """E[y], Var[y] of p(y | X) ∝ prod_i (X_i . y) on the simplex (n = 2 or 3) by f64 quadrature (midpoint rule)."""
    t = (np.arange(grid) + 0.5) / grid
    if n == 2:
        Y = np.stack([t, 1 - t], axis=1)
        wq = np.full(grid, 1.0 / grid)
    else:
        a, b = np.meshgrid(t, t, indexing="ij")
        y1 = a
        y2 = (1 - a) * b
        Y = np.stack([y1.ravel(), y2.ravel(), (1 - y1 - y2).ravel()], axis=1)
        wq = ((1 - a) / grid ** 2).ravel()  # Jacobian of (a, b) -> simplex
    logp = np.log(Y @ Xrows.T.astype(np.float64)).sum(axis=1)
    p = np.exp(logp - logp.max()) * wq
    p /= p.sum()
    mean = p @ Y
    var = p @ (Y - mean) ** 2
    return mean, var


def tiny_problem(n, m, seed):
    """m multi-transcript fragments over n transcripts (dense rows, random weights) in the HDF5's CSC form."""
    rng = np.random.default_rng(seed)
    Xd = rng.uniform(0.05, 1.0, size=(m, n)).astype(np.float32) * rng.uniform(0.2, 3.0, size=n).astype(np.float32)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.full(n, m))]).astype(np.uint64)
    rowval = np.tile(np.arange(1, m + 1, dtype=np.uint32), n)
    nzval = Xd.T.ravel().astype(np.float32)
    return Xd, colptr, rowval, nzval


# ---- tests --------------------------------------------------------------------------------------------------------------------
def test_philox_matches_the_published_known_answer():
    """Random123's known-answer vector for Philox4x32-10 (counter = key = 0) and the device's key schedule."""
    w = philox4x32_10(np.uint32(0), np.uint32(0), np.uint32(0), np.uint32(0), 0)
    assert [int(x) for x in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    w = philox4x32_10(np.uint32(0x243F6A88), np.uint32(0x85A308D3), np.uint32(0x13198A2E), np.uint32(0x03707344),
                      (0x299F31D0 << 32) | 0xA4093822)
    assert [int(x) for x in w] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    u = u01f(np.array([0, 0xFFFFFFFF], np.uint32))
    assert 0 < u[0] < u[1] <= 1  # (f32: 2^24 - 0.5 rounds to 2^24 -- r = sum w then picks the last positive weight)
    assert u01d(np.array([0xFFFFFFFF], np.uint32))[0] < 1


def test_rand_gamma_moments_including_large_shapes():
    """Marsaglia-Tsang with the f64 test: mean a and variance a at a = 1, 51 and 1e6 + 1 (the f32 cancellation case)."""
    N = 40000
    for a in (1.0, 51.0, 1e6 + 1):
        x = rand_gamma(np.full(N, a), 99, np.arange(N), 0, 1, TAG_GAMMA).astype(np.float64)
        assert abs(x.mean() - a) < 5 * np.sqrt(a / N), (a, x.mean())
        assert abs(x.var() / a - 1) < 5 * np.sqrt(2.0 / N) + 2e-3 * (a > 1e5), (a, x.var() / a)


def test_assignment_every_weight_zero_picks_the_first_entry():
    indptr = np.array([0, 3])
    lay = Layout(1, 3, indptr, np.array([0, 1, 2]), np.array([1.0, 1.0, 1.0], np.float32))
    picks, _ = assign(lay, np.zeros((2, 3), np.float32), 1, 1)
    assert (picks == 0).all()


@pytest.mark.parametrize("n,m", [(2, 40), (3, 25)])
def test_restatement_matches_exact_posterior(n, m):
    Xd, colptr, rowval, nzval = tiny_problem(n, m, seed=n)
    lay = Layout(m, n, *rows_of(m, n, colptr, rowval, nzval))
    C, burn, S = 64, 100, 600
    s = NumpyGibbs(lay, C, seed=7)
    draws = np.empty((C, S, n))
    for t in range(burn + S):
        s.step()
        if t >= burn:
            draws[:, t - burn] = s.x()
    mean, var = exact_moments(Xd, n)
    for j in range(n):
        se_m = batch_means_se(draws[:, :, j])
        se_v = batch_means_se((draws[:, :, j] - mean[j]) ** 2)
        assert abs(draws[:, :, j].mean() - mean[j]) < 5 * se_m, (j, draws[:, :, j].mean(), mean[j], se_m)
        assert abs(((draws[:, :, j] - mean[j]) ** 2).mean() - var[j]) < 5 * se_v, (j, var[j])


def test_conjugate_counts_are_base_counts():
    """Single-transcript fragments only: the counts are the base counts, and the draws Dirichlet(1 + c)."""
    n, cs = 4, np.array([0, 3, 50, 1000])
    m = int(cs.sum())
    rowval = np.arange(1, m + 1, dtype=np.uint32)
    colptr = np.concatenate([[1], 1 + np.cumsum(cs)]).astype(np.uint64)
    lay = Layout(m, n, *rows_of(m, n, colptr, rowval, np.ones(m, np.float32)))
    assert (lay.base == cs).all() and lay.rows.size == 0
    s = NumpyGibbs(lay, 16, seed=3)
    xs = []
    for _ in range(300):
        s.step()
        assert (s.counts == cs[None, :]).all()
        xs.append(s.x())
    xs = np.concatenate(xs)
    a = 1.0 + cs
    mean = a / a.sum()
    assert np.all(np.abs(xs.mean(axis=0) - mean) < 5 * np.sqrt(mean * (1 - mean) / (a.sum() + 1) / xs.shape[0]))


def test_convergence_stats_formula():
    """The integer split and the variance terms of gibbs.jl:283-319 on a hand-sized case; ~1 for iid draws."""
    rng = np.random.default_rng(0)
    x = rng.normal(size=(4, 101, 3)).astype(np.float32)
    R = convergence_stats(x, 101)
    assert np.all(np.abs(R - 1) < 0.05)
    # a chain offset from the others inflates R
    x[0] += 3
    assert np.all(convergence_stats(x, 101) > 1.5)
    # count = 5: k = 2, halves of 3 and 2 draws, variances over 1/k
    y = np.arange(2 * 5, dtype=np.float64).reshape(2, 5, 1)
    k, C = 2, 2
    means = np.array([1.0, 6.0, 3.5, 8.5])
    B = k / (2 * C - 1) * ((means - means.mean()) ** 2).sum()
    W = (2 * 2.0 + 2 * 0.5) / k / (2 * C)
    assert np.isclose(convergence_stats(y, 5)[0], np.sqrt(((k - 1) / k * W + B / k) / W))


def _fake_draws(C=2, S=3, n=5, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.gamma(1.0, size=(C, S, n)).astype(np.float32)
    return x / x.sum(axis=2, keepdims=True)


def test_kallisto_writer_layout(tmp_path):
    from polee_amd import h5io
    from polee_amd.gibbs import write_kallisto
    x = _fake_draws()
    C, S, n = x.shape
    els = np.array([100, 200, 50, 400, 1000], np.float32)
    ids = ["ENST%d" % j for j in range(n)]
    lens = np.array([300, 400, 150, 800, 1500])
    fn = str(tmp_path / "g.h5")
    write_kallisto(fn, x, els, 1234, ids, lens, use_efflen=True, call="-o g.h5 --kallisto lm.h5")
    with h5io.File(fn) as f:
        assert f.dataset_kind("est_counts") == ("float", 8, (n,))
        est = f.read("est_counts", np.float64)
        pm = x.astype(np.float64).mean(axis=(0, 1)) * els
        assert np.allclose(est, pm / pm.sum() * 1234, rtol=1e-12)
        assert np.isclose(est.sum(), 1234)
        assert f.dataset_kind("aux/num_bootstrap") == ("integer", 8, (1,)) and f.read("aux/num_bootstrap", np.int64)[0] == C * S
        assert np.allclose(f.read("aux/eff_lengths", np.float64), els)
        assert (f.read("aux/lengths", np.int64) == lens).all()
        assert f.read_strings("aux/ids") == ids
        assert f.read_strings("aux/call") == ["-o g.h5 --kallisto lm.h5"]
        assert f.read("aux/index_version", np.int64)[0] == -1
        assert f.read_strings("aux/kallisto_version") == "polee debug-sample"
        assert len(f.read_strings("aux/start_time")) >= 19
        for k in range(C * S):
            c, s = divmod(k, S)
            bs = f.read("bootstrap/bs%d" % k, np.float64)
            v = x[c, s].astype(np.float64) * els
            assert np.allclose(bs, v / v.sum() * 1234, rtol=1e-12)
        assert not f.exists("bootstrap/bs%d" % (C * S))


def test_kallisto_writer_without_efflen(tmp_path):
    from polee_amd import h5io
    from polee_amd.gibbs import write_kallisto
    x = _fake_draws(1, 2, 4)
    fn = str(tmp_path / "g.h5")
    write_kallisto(fn, x, np.ones(4, np.float32) * 7, 10, ["a", "b", "c", "d"], -np.ones(4), use_efflen=False)
    with h5io.File(fn) as f:
        assert np.allclose(f.read("est_counts", np.float64), x.astype(np.float64).mean(axis=(0, 1)) * 10)
        assert np.allclose(f.read("bootstrap/bs1", np.float64), x[0, 1].astype(np.float64) * 10)


def test_csv_writer(tmp_path):
    from polee_amd.gibbs import write_csv
    x = _fake_draws(2, 2, 3)
    fn = str(tmp_path / "g.csv")
    write_csv(fn, x, ["t1", "t2", "t3"])
    lines = open(fn).read().splitlines()
    assert lines[0] == "t1,t2,t3" and len(lines) == 5
    back = np.array([[float(v) for v in l.split(",")] for l in lines[1:]])
    assert np.allclose(back, x.reshape(4, 3), rtol=1e-6)
    assert all("e" in v for v in lines[1].split(","))


def test_cli_rejects_ids_of_the_wrong_length(tmp_path):
    from polee_amd.gibbs import gibbs_sampler
    lm = os.path.join(ROOT, "tests", "golden", "mBr_M_6w_1.likelihood-matrix.h5")
    with pytest.raises(ValueError, match="different number of transcripts"):
        gibbs_sampler(lm, str(tmp_path / "g.csv"), transcript_ids=["a", "b"])

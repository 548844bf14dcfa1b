"""-m gpu: RNASeqTSNE (polee_amd/tsne.py, csrc/tsne.hip; models/polee_tsne.py:17-185, :213-398) against the NumPy float64 restatement
tests/tsne_restatement.py.

The restatement is fed the DEVICE'S OWN draws (polee_approx_sample with the same z0 slice; the sampler's parity with the oracle is
covered by tests/test_gpu_parity.py), so a wrong z0 slice, draw index or seed rule is an O(1) error.  The bandwidths are set
explicitly, sqrt(median delta) f U(0.5, 1.5) (_sigmas): find_sigmas at S <= 51 ends at the top of its bracket and P is uniform whatever x is.  The
problems are built as _problem of tests/test_gpu_classify.py builds them, but with ONE tree for all samples and la_mu = a shared
profile + a group effect (two groups) + noise of graded size: independent parameters per sample give all pairs the same distance and
a P that no bandwidth spreads.  Every case with B >= 3 asserts that P spans a factor 3 off the diagonal; at B = 2 the one
off-diagonal entry is 1 / S + eps exactly, whatever the distance.

Tolerances.  With L = max |lx|, c = lx - (row mean) (L2: c = lx), dc_j = c_aj - c_bj:
  delta   a staged value is fl(logf(x) - mhat): one ulp of logf, 1.2e-7 L, plus the subtraction's half ulp, 6e-8 max |c|; a difference
          of two adds its own half ulp: e = 2 (1.2e-7 L + 6e-8 max |c|) + 6e-8 max |dc|.  The squares are summed by an f32 FMA chain
          of at most 512 terms per chunk (512 2^-24 = 3.1e-5 relative to the sum of the terms, which are all positive); the chunk
          partials are combined in f64 and the residue of the rounded row mean is taken out exactly.  So
              |delta_dev - delta_ref| <= (2 e sum_j |dc_j| + 3.1e-5 sum_j dc_j^2) / n       (L2: without the / n)
  z       a chunk of 128 transcripts is one product, one FMA and six shuffle-tree additions per lane, 8 roundings of 2^-24, plus the
          ulp of logf: B_z = 6e-7 max_{s,c} sum_j |lx_sj W_jc|; the chunks are combined in f64.  The embedding: B_z + 6e-8 |z|.
  loss    first order in r_E = max_ab expm1(tol_delta_ab / (2 sigma_b^2)), the relative error of E_ab (twice that for the
          column-normalised pc and for P), and r_k = ((alpha + 1) / sqrt(alpha)) sqrt(C) B_z, the relative error of a Student kernel
          whose arguments are off by 2 B_z per component (d log k = ((alpha + 1) / (2 alpha)) dD / (1 + D / alpha), dD <= 4 B_z
          sqrt(C D), and sqrt(D) / (1 + D / alpha) <= sqrt(alpha) / 2; twice that for Q):
              |loss_dev - loss_ref| <= 1e-6 |loss| + sum_ab P_ab ((|log(P_ab / Q_ab)| + 1) 2 r_E + 2 r_k)
          (dL/dP = log(P / Q) + 1, dL/dQ = -P / Q); 1e-6 |loss| is the f32 result.
  g_W     the convention of tests/test_gpu_regression.py: an entry within 1e-2 relative to |ref| + 2e-3 max |g|.
  Adam    against the device's own gradients, |p_dev - p_host| <= 1e-5 lr_t + 6e-8 |p|.  No multi-step trajectory is compared with a
          float64 one: m / (sqrt(v) + eps) is the same +-(1 - b1) / sqrt(1 - b2) on the first step whatever the gradient's size, so
          rounding-level gradient differences grow into O(lr) parameter differences (as tests/test_gpu_classify.py explains).

Worst observed ratios (MI355X): profiles/tsne_parity_margins.txt -- delta 0.002 to 0.022 of its bound, z 0.013 to 0.027, g_W at most
0.10, Adam 0.07.  The loss uses 1e-6 to 1.2e-3 of its bound, a headroom ABOVE the factor 1000 within which a derived bound counts as
sharp; written down, not tuned: the bound charges the worst relative error of any E_ab to every entry of P with one sign, while pc is
a ratio in which the error a column shares cancels and the B^2 terms' errors are of either sign.  A wrong distance is not hidden by
it: delta is held to its own bound and P is asserted to be far from uniform.
"""
import ctypes as C

import numpy as np
import pytest

import tsne_restatement as T
from conftest import random_tree
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def ctx(P):
    return P.Context(0)


_PROBLEMS = {}


def _problem(P, ctx, S, n):
    """one random tree, per-sample parameters; built once per shape"""
    if (S, n) not in _PROBLEMS:
        rng = np.random.default_rng(2000 * S + n)
        li, ri, fi = O.make_inverse_ptt_params(*random_tree(n, rng))
        group = (np.arange(S) % 2)[:, None] * rng.normal(0, 0.7, size=(1, n - 1))
        mu = rng.normal(0, 1, size=(1, n - 1)) + group + rng.uniform(0.1, 0.5, size=(S, 1)) * rng.normal(0, 1, size=(S, n - 1))
        vars_ = dict(efflen=rng.uniform(200, 3000, size=(S, n)).astype(np.float32), la_mu=mu.astype(np.float32),
                     la_sigma=np.exp(rng.normal(-2.5, 0.3, size=(S, n - 1))).astype(np.float32),
                     la_alpha=rng.normal(0, 0.3, size=(S, n - 1)).astype(np.float32), left_index=li[None], right_index=ri[None],
                     leaf_index=fi[None])
        _PROBLEMS[(S, n)] = P.RNASeqApproxLikelihood(vars_, ctx=ctx)
    return _PROBLEMS[(S, n)]


def _points(S, n):
    rng = np.random.default_rng(3000 * S + n)
    group = (np.arange(S) % 2)[:, None] * rng.normal(0, 0.7, size=(1, n))
    x = rng.normal(-np.log(n), 1.5, size=(1, n)) + group + rng.uniform(0.1, 0.5, size=(S, 1)) * rng.normal(0, 1, size=(S, n))
    return x.astype(np.float32)


def _draw(ap, z0):
    """the device's own draw for z0 [S][n-1], as log expression in float64"""
    return np.log(ap.sample(z0=z0.copy()).astype(np.float64))


def _batch(rng, S, B):
    return rng.permutation(S)[:B].astype(np.int32)  # (unsorted)


def _sigmas(rng, lx, use_vlr, batch=None):
    """explicit bandwidths sqrt(median delta) f U(0.5, 1.5), f32 [S]: f = 0.5, or with a batch of 3 or more the largest of 1, 0.7, 0.5,
    ... at which the restatement's P on that batch spans a factor 4 off the diagonal (the tests then assert a factor 3)"""
    d = T.pairwise_delta(lx, use_vlr)
    base = np.sqrt(np.median(d[d > 0])) * rng.uniform(0.5, 1.5, size=lx.shape[0])
    if batch is None or len(batch) < 3:
        return (0.5 * base).astype(np.float32)
    for f in (1.0, 0.7, 0.5, 0.35, 0.25, 0.18, 0.12):
        sig = (f * base).astype(np.float32)
        off = T.p_matrix(d[np.ix_(batch, batch)], sig[batch].astype(np.float64), lx.shape[0])[~np.eye(len(batch), dtype=bool)]
        if off.max() >= 4.0 * off.min():
            break
    return sig


def _delta_tol(lx, use_vlr):
    """the bound of the docstring for every pair of rows of lx [B][n]"""
    c = lx - lx.mean(axis=1, keepdims=True) if use_vlr else lx
    L, cmax = np.abs(lx).max(), np.abs(c).max()
    tol = np.zeros((lx.shape[0], lx.shape[0]))
    for a in range(lx.shape[0]):
        dc = c[a][None, :] - c
        e = 2.0 * (1.2e-7 * L + 6e-8 * cmax) + 6e-8 * np.abs(dc).max()
        tol[a] = 2.0 * e * np.abs(dc).sum(axis=1) + 3.1e-5 * (dc * dc).sum(axis=1)
    return tol / lx.shape[1] if use_vlr else tol


def _B_z(lx, W):
    return 6e-7 * (np.abs(lx) @ np.abs(W.astype(np.float64))).max()


def _model(P, ctx, n, S, C, use_vlr=True, **kw):
    return P.RNASeqTSNE(n, S, ctx=ctx, num_components=C, use_vlr=int(use_vlr), **kw)


# ---- distances
@pytest.mark.parametrize("n,S", [(130, 3), (150, 5), (1100, 5), (130, 70), (1100, 70)])
@pytest.mark.parametrize("use_vlr", [True, False])
def test_distances_match_restatement(P, ctx, n, S, use_vlr):
    """n = 130, 150: one chunk of the pairwise kernel, the last staged block ragged; 1100: three chunks, the last of 76 transcripts;
    S = 70: two row tiles, three tile pairs, the second tile of 6 rows.  Both paths."""
    rng = np.random.default_rng(101)
    ap = _problem(P, ctx, S, n)
    ts = _model(P, ctx, n, S, 2, use_vlr)
    z0 = rng.normal(size=(S, n - 1)).astype(np.float32)
    x = _points(S, n)
    for tag, got, lx in (("draws", ts.distances(ap, z0=z0), _draw(ap, z0)), ("points", ts.distances(x=x), x.astype(np.float64))):
        ref, tol = T.pairwise_delta(lx, use_vlr), _delta_tol(lx, use_vlr)
        np.testing.assert_array_equal(got, got.T)
        assert not np.diag(got).any() and got.shape == (S, S) and (got >= 0).all()
        off = ~np.eye(S, dtype=bool)
        used = float((np.abs(got - ref)[off] / tol[off]).max())
        print("MARGIN delta %s n=%d S=%d vlr=%d: delta %.3g .. %.3g, used %.3g" % (tag, n, S, use_vlr, ref[off].min(), ref[off].max(),
                                                                                   used))
        assert used <= 1.0


# ---- loss and gradient
# (n, S, B, C, use_vlr, alpha): C = 1, 2 / 3 / 6 / 16 run the kernels' four widths (2, 4, 8, 16), C = 1, 3 and 6 with padding; B < S
# leaves samples whose gradient comes through the normaliser of Q alone
CASES = [(130, 3, 2, 1, True, 1.0), (130, 3, 3, 2, True, 1.0), (150, 5, 2, 3, True, 1.0), (150, 5, 5, 16, True, 1.0),
         (150, 5, 3, 6, True, 1.0),
         (1100, 5, 5, 2, True, 1.0), (130, 70, 37, 2, True, 1.0), (150, 70, 70, 3, True, 1.0), (1100, 70, 37, 16, True, 1.0),
         (1100, 3, 3, 1, False, 1.0), (150, 70, 37, 2, False, 2.5)]


def _check(tag, lx, W, batch, sig, use_vlr, alpha, loss, g_W):
    S, C = lx.shape[0], W.shape[1]
    loss_o, g_o, _, Pm, Qm = T.loss_and_gradient(W, lx, batch, sig, use_vlr, alpha)
    off = Pm[~np.eye(len(batch), dtype=bool)]
    spread = off.max() / off.min()
    if len(batch) >= 3:
        assert spread >= 3.0, spread  # (a test on a uniform P could not see a wrong distance)
    r_E = np.expm1(_delta_tol(lx[batch], use_vlr) / (2.0 * sig[batch].astype(np.float64)[None, :] ** 2)).max()
    r_k = (alpha + 1.0) / np.sqrt(alpha) * np.sqrt(C) * _B_z(lx, W)
    tol = 1e-6 * abs(loss_o) + (Pm * ((np.abs(np.log(Pm / Qm)) + 1.0) * 2.0 * r_E + 2.0 * r_k)).sum()
    used_l = abs(loss - loss_o) / tol
    used_g = float((np.abs(g_W - g_o) / (np.abs(g_o) + 2e-3 * np.abs(g_o).max())).max()) / 1e-2
    print("MARGIN %s loss %.6g ref %.6g  P spread %.3g  used: loss %.3g g_W %.3g" % (tag, loss, loss_o, spread, used_l, used_g))
    assert used_l <= 1.0, (loss, loss_o, tol)
    assert used_g < 1.0


@pytest.mark.parametrize("n,S,B,C,use_vlr,alpha", CASES)
def test_loss_and_gradient_match_restatement(P, ctx, n, S, B, C, use_vlr, alpha):
    rng = np.random.default_rng(102)
    ap = _problem(P, ctx, S, n)
    z0 = rng.normal(size=(S, n - 1)).astype(np.float32)
    lx = _draw(ap, z0)
    W = rng.normal(0, 0.1, size=(n, C)).astype(np.float32)
    batch = _batch(rng, S, B)
    sig = _sigmas(rng, lx, use_vlr, batch)
    ts = _model(P, ctx, n, S, C, use_vlr, alpha=alpha)
    ts.set_params(W)
    np.testing.assert_array_equal(ts.get_params(), W)
    ts.set_sigmas(sig)
    loss, g_W = ts.loss_and_gradient(batch, ap, z0=z0)
    _check("draws n=%d S=%d B=%d C=%d vlr=%d" % (n, S, B, C, use_vlr), lx, W, batch, sig, use_vlr, alpha, loss, g_W)


@pytest.mark.parametrize("n,S,B,C,use_vlr", [(150, 70, 70, 2, True), (130, 5, 3, 16, False), (1100, 70, 37, 3, True)])
def test_point_path_matches_restatement(P, ctx, n, S, B, C, use_vlr):
    rng = np.random.default_rng(103)
    x = _points(S, n)
    lx = x.astype(np.float64)
    W = rng.normal(0, 0.1, size=(n, C)).astype(np.float32)
    batch = _batch(rng, S, B)
    sig = _sigmas(rng, lx, use_vlr, batch)
    ts = _model(P, ctx, n, S, C, use_vlr)
    ts.set_params(W)
    ts.set_sigmas(sig)
    loss, g_W = ts.loss_and_gradient(batch, x=x)
    _check("points n=%d S=%d B=%d C=%d vlr=%d" % (n, S, B, C, use_vlr), lx, W, batch, sig, use_vlr, 1.0, loss, g_W)
    z = ts.embed(x=x)
    used = float((np.abs(z - lx @ W) / (_B_z(lx, W) + 6e-8 * np.abs(lx @ W))).max())
    print("MARGIN embed points n=%d S=%d C=%d used %.3g" % (n, S, C, used))
    assert z.shape == (S, C) and used <= 1.0


# ---- Adam
@pytest.mark.parametrize("n,S,B,C", [(150, 5, 3, 8), (1100, 70, 37, 2)])
def test_adam_against_the_devices_own_gradients(P, ctx, n, S, B, C):
    """three single steps: Adam's form (TF1: beta1 0.99, epsilon 1e-8) and the step clock, without any sensitivity to the rounding of
    the gradients"""
    rng = np.random.default_rng(104)
    lr, steps = 1e-2, 3
    b1, b2, eps = (float(np.float32(v)) for v in (0.99, 0.999, 1e-8))  # (the options are f32)
    ap = _problem(P, ctx, S, n)
    z0 = rng.normal(size=(steps, S, n - 1)).astype(np.float32)
    W = rng.normal(0, 0.1, size=(n, C)).astype(np.float32)
    ts = _model(P, ctx, n, S, C, learning_rate=lr)
    ts.set_params(W)
    ts.set_sigmas(_sigmas(rng, _draw(ap, z0[0]), True))
    m = v = 0.0
    worst = 0.0
    for t in range(1, steps + 1):
        batch = _batch(rng, S, B)
        before = ts.get_params()
        loss, g = ts.loss_and_gradient(batch, ap, z0=z0[t - 1])
        trace = ts.fit(1, ap, batches=batch[None], z0=z0[t - 1])
        assert trace[0] == np.float32(loss)  # (the same kernels in the same order)
        after = ts.get_params()
        lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        host, m, v = T.adam_step(before, g, m, v, t, lr, b1, b2, eps)
        err = np.abs(after.astype(np.float64) - host)
        tol = 1e-5 * lr_t + 6e-8 * np.abs(host)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (t, float((err / tol).max()))
        assert np.abs(after - before).max() > 0.1 * lr_t  # (the step is far above the rounding of p)
    print("MARGIN adam n=%d S=%d B=%d C=%d used %.3g of the bound" % (n, S, B, C, worst))


# ---- clock and reproducibility
def test_clock_and_reproducibility_are_bitwise(P, ctx):
    rng = np.random.default_rng(105)
    n, S, B, C = 150, 5, 3, 2
    ap = _problem(P, ctx, S, n)
    W = rng.normal(0, 0.1, size=(n, C)).astype(np.float32)
    sig = _sigmas(rng, np.log(ap.sample(seed=1).astype(np.float64)), True)

    def fresh():
        ts = _model(P, ctx, n, S, C, learning_rate=1e-2)
        ts.set_params(W)
        ts.set_sigmas(sig)
        return ts
    a = fresh()
    batch = _batch(rng, S, B)
    e1, e2 = a.loss_and_gradient(batch, ap, seed=11), a.loss_and_gradient(batch, ap, seed=11)
    assert e1[0] == e2[0]
    np.testing.assert_array_equal(e1[1], e2[1])
    assert a.loss_and_gradient(batch, ap, seed=12)[0] != e1[0]  # (other draws)
    np.testing.assert_array_equal(a.distances(ap, seed=11), a.distances(ap, seed=11))
    z0 = rng.normal(size=(5, S, n - 1)).astype(np.float32)
    for kw_split, kw_whole in ((lambda lo, hi: dict(seed=21), dict(seed=21)), (lambda lo, hi: dict(z0=z0[lo:hi]), dict(z0=z0))):
        a, b = fresh(), fresh()
        ta = np.concatenate([a.fit(2, ap, batch_size=B, **kw_split(0, 2)), a.fit(3, ap, batch_size=B, **kw_split(2, 5))])
        tb = b.fit(5, ap, batch_size=B, **kw_whole)
        np.testing.assert_array_equal(ta, tb)
        np.testing.assert_array_equal(a.get_params(), b.get_params())
        assert not np.array_equal(a.get_params(), W) and a.t == b.t == 5
    c = fresh()
    assert not np.array_equal(c.fit(5, ap, batch_size=B, seed=22), tb)  # (another seed: other batches and other draws)
    assert not np.array_equal(c.get_params(), b.get_params())
    c.reset()
    assert c.t == 0
    z1, z2 = a.embed(ap, ndraws=4, seed=31), a.embed(ap, ndraws=4, seed=31)
    np.testing.assert_array_equal(z1, z2)
    assert not np.array_equal(z1, a.embed(ap, ndraws=4, seed=32))


# ---- the embedding
@pytest.mark.parametrize("n,S,C,ndraws", [(150, 5, 3, 4), (1100, 70, 16, 2), (130, 3, 1, 3)])
def test_embedding_matches_restatement(P, ctx, n, S, C, ndraws):
    rng = np.random.default_rng(106)
    ap = _problem(P, ctx, S, n)
    z0 = rng.normal(size=(ndraws, S, n - 1)).astype(np.float32)
    lx = np.stack([_draw(ap, z) for z in z0])
    W = rng.normal(0, 0.1, size=(n, C)).astype(np.float32)
    ts = _model(P, ctx, n, S, C)
    ts.set_params(W)
    z = ts.embed(ap, ndraws=ndraws, z0=z0)
    ref = T.embed(W, lx)
    used = float((np.abs(z - ref) / (max(_B_z(l, W) for l in lx) + 6e-8 * np.abs(ref))).max())
    print("MARGIN embed n=%d S=%d C=%d draws=%d used %.3g" % (n, S, C, ndraws, used))
    assert z.shape == (S, C) and used <= 1.0


def test_find_sigmas_runs_on_the_devices_distances_of_draw_minus_one(P, ctx):
    from polee_amd import tsne
    n, S = 150, 70
    ap = _problem(P, ctx, S, n)
    ts = _model(P, ctx, n, S, 2)
    sig = ts.find_sigmas(ap, seed=77)
    delta = ts.distances(ap, seed=(77 - 0x9E3779B97F4A7C15) % (1 << 64))
    np.testing.assert_array_equal(sig, tsne.find_sigmas(delta, 50.0))
    np.testing.assert_array_equal(sig, T.find_sigmas(delta, 50.0)[0].astype(np.float32))
    assert sig.dtype == np.float32 and (sig > 1e-2).all()


# ---- planted groups, on the point path
def _planted():
    """S = 12 as two groups of 6, n = 150 of which 40 transcripts are shifted by N(0, 2) between the groups, replicate noise 0.2"""
    rng = np.random.default_rng(107)
    S, n = 12, 150
    group = np.arange(S) // 6
    shift = np.zeros(n)
    shift[rng.choice(n, 40, replace=False)] = rng.normal(0, 2, size=40)
    x = rng.normal(-np.log(n), 1.5, size=(1, n)) + group[:, None] * shift[None, :] + rng.normal(0, 0.2, size=(S, n))
    return x.astype(np.float32), group


def _separation(z, group):
    d = np.sqrt(((z[:, None, :] - z[None, :, :]) ** 2).sum(axis=2))
    same = group[:, None] == group[None, :]
    return d[~same].mean() / d[same & ~np.eye(len(z), dtype=bool)].mean()


def test_planted_groups_separate(P, ctx):
    """perplexity 4, B = 8, learning rate 1e-3 (the reference's 1e-6 moves W by less than 5e-4 in 500 steps), 300 steps.  A float64
    NumPy run of the restatement on these very inputs (same W0, batches and bandwidths) takes the loss to 0.50 of its start and the
    between / within distance ratio to 15.9, so the thresholds 0.8 and 3 leave room."""
    from polee_amd import tsne
    x, group = _planted()
    S, n = x.shape
    ts = _model(P, ctx, n, S, 2, learning_rate=1e-3)
    ts.find_sigmas(x=x, target_perplexity=4.0)
    ts.set_params(tsne.initial_weights(5, n, 2))
    trace = ts.fit(300, x=x, batch_size=8, seed=5)
    z = ts.embed(x=x)
    ratio, sep = trace[-10:].mean() / trace[:10].mean(), _separation(z.astype(np.float64), group)
    print("planted groups: loss %.4g -> %.4g (ratio %.3g), between / within %.3g" % (trace[:10].mean(), trace[-10:].mean(), ratio, sep))
    assert np.all(np.isfinite(trace)) and ratio < 0.8
    assert sep > 3.0


def test_estimate_tsne_on_draws_and_on_posterior_means(P, ctx):
    """the whole of estimate_tsne, both paths, a few steps: shapes, finiteness, and the draw path's seed rule"""
    n, S = 150, 5
    ap = _problem(P, ctx, S, n)
    z1, tr1 = P.estimate_tsne(ap, 3, 4, num_steps=6, seed=9, ctx=ctx, return_trace=True)
    z2 = P.estimate_tsne({"approx": ap}, 3, 4, num_steps=6, seed=9, ctx=ctx)
    np.testing.assert_array_equal(z1, z2)
    assert z1.shape == (S, 3) and z1.dtype == np.float32 and tr1.shape == (6,) and np.isfinite(z1).all() and np.isfinite(tr1).all()
    assert not np.array_equal(z1, P.estimate_tsne(ap, 3, 4, num_steps=6, seed=10, ctx=ctx))
    zp = P.estimate_tsne(None, 2, 100, x0_log=_points(S, n), use_posterior_mean=True, num_steps=6, ctx=ctx)
    assert zp.shape == (S, 2) and np.isfinite(zp).all()


# ---- argument errors
def test_errors(P, ctx):
    n, S = 130, 3
    ap = _problem(P, ctx, S, n)
    for bad in (0, 17):
        with pytest.raises(P.PoleeError) as ei:
            _model(P, ctx, n, S, bad)
        assert ei.value.status == 5 and "components" in str(ei.value)
    ts = _model(P, ctx, n, S, 2)
    ok = np.array([2, 0], np.int32)
    with pytest.raises(P.PoleeError) as ei:  # (bandwidths not set)
        ts.loss_and_gradient(ok, ap)
    assert ei.value.status == 1 and "bandwidths" in str(ei.value)
    for bad in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, np.nan, 1.0], [1.0, np.inf, 1.0]):
        with pytest.raises(P.PoleeError) as ei:
            ts.set_sigmas(bad)
        assert ei.value.status == 1 and "sigma[1]" in str(ei.value)
    with pytest.raises(P.PoleeError):  # (a refused set_sigmas sets nothing)
        ts.loss_and_gradient(ok, ap)
    ts.set_sigmas([1.0, 2.0, 0.5])
    for bad, needle in (([0, 3], "index 3"), ([-1, 0], "index -1"), ([1, 1], "twice"), ([0, 2, 0], "twice"), ([1], "batch size 1"),
                        ([0, 1, 2, 0], "batch size 4")):
        with pytest.raises(P.PoleeError) as ei:
            ts.loss_and_gradient(np.array(bad, np.int32), ap)
        assert ei.value.status == 1 and needle in str(ei.value), (bad, str(ei.value))
        with pytest.raises(P.PoleeError) as ei:  # (in the second batch of a fit: nothing is run)
            ts.fit(2, x=_points(S, n), batches=np.array([[0, 1, 2, 0][:len(bad)], bad], np.int32))
        assert ei.value.status == 1
    assert ts.t == 0
    other_n, other_S = _model(P, ctx, 150, S, 2), _model(P, ctx, n, 5, 2)
    for m in (other_n, other_S):  # (past the wrapper's own check: the library refuses an approximation of another n or S)
        delta = np.empty((m.S, m.S))
        with pytest.raises(P.PoleeError) as ei:
            P._lib.check(P.lib().polee_tsne_distances(m._h, ap._h, None, C.c_uint64(0), delta.ctypes.data_as(P._lib.f64p)), ctx._h)
        assert ei.value.status == 1 and "S = 3, n = 130" in str(ei.value)
    elsewhere = _model(P, P.Context(0), n, S, 2)  # (another context on the same device)
    with pytest.raises(P.PoleeError) as ei:
        elsewhere.distances(ap)
    assert ei.value.status == 1 and "another context" in str(ei.value)
    x = _points(S, n)
    x[1, 7] = -np.inf
    for call in (lambda: ts.distances(x=x), lambda: ts.loss_and_gradient(ok, x=x), lambda: ts.fit(1, x=x, batches=ok[None]),
                 lambda: ts.embed(x=x)):
        with pytest.raises(P.NonFiniteError) as ei:
            call()
        assert ei.value.status == 4 and "x[1][7]" in str(ei.value)
    assert ts.loss_and_gradient(ok, ap)[0] > 0  # (the handle still works)

"""-m gpu: the latent-design mode of the regression handle (csrc/regression.hip, polee_regression_set_latent_design) and RNASeqPCA
(polee_amd/pca.py; models/polee_pca.py:14-92) against the NumPy float64 restatement

    pca_loss(z) = oracle.regression_ref.regression_loss(..., design=z) + sum( z^2 / (2 sigma^2) + log sigma + log(2 pi) / 2 )

whose z-gradient is -a w_eff^T + z / sigma^2 with a = (x - mu) / x_scale^2 from the draws regression_loss returns.

Tolerances are those of tests/test_gpu_regression.py: the loss 1e-4 |loss| + 1e-2, a gradient entry 1e-2 relative to |reference| +
2e-3 of the gradient's scale.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import random_tree
from oracle import oracle as O
from oracle import regression_ref as RR
from pca_restatement import pca_loss, pca_z_gradient, prior_nlp, weights

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def ctx(P):
    return P.Context(0)


def _problem(rng, S, n):
    trees = [random_tree(n, rng) for _ in range(S)]
    idx = [O.make_inverse_ptt_params(*tr) for tr in trees]
    L_, R_, F_ = (np.stack([i[j] for i in idx]) for j in range(3))
    eff = rng.uniform(200, 3000, size=(S, n)).astype(np.float32)
    mu = rng.normal(0, 1, size=(S, n - 1)).astype(np.float32)
    sigma = np.exp(rng.normal(-1, 0.3, size=(S, n - 1))).astype(np.float32)
    alpha = rng.normal(0, 0.3, size=(S, n - 1)).astype(np.float32)
    vars_ = dict(efflen=eff, la_mu=mu, la_sigma=sigma, la_alpha=alpha, left_index=L_, right_index=R_, leaf_index=F_)
    x_init = (rng.normal(-np.log(n), 1.5, size=(1, n)) + rng.normal(0, 0.4, size=(S, n))).astype(np.float32)
    return vars_, x_init


def _lik(vars_):
    a = (vars_["efflen"], vars_["la_mu"], vars_["la_sigma"], vars_["la_alpha"], vars_["left_index"],
         vars_["right_index"], vars_["leaf_index"])
    return lambda x: O.approx_log_prob(x.astype(np.float32), *a).astype(np.float64)


def _set_lr(P, reg, lr):
    P._lib.check(P.lib().polee_regression_set_learning_rate(reg._h, C.c_float(lr)), reg.ctx._h)


# (distortion, point estimates, C, deg): run-time shapes, point estimates, F above the fixed-trip-count instances with 15 hinges, the
# REG_MAXF edge; and (2, 15), which the handle's data and column kernels run with fixed trip counts (deg = 15, F <= 4)
CASES = [(True, False, 2, 5), (False, True, 3, 5), (True, False, 5, 15), (True, False, 16, 5), (True, False, 2, 15)]


@pytest.mark.parametrize("n", [150, 130])  # neither a multiple of the block (128) nor of 64: dead lanes must add nothing
@pytest.mark.parametrize("use_distortion,point,Cdim,deg", CASES)
def test_loss_and_z_gradient_match_restatement(P, ctx, use_distortion, point, Cdim, deg, n):
    rng = np.random.default_rng(51)
    S, pen, bw = 4, 0.7, 1.3
    vars_, x_init = _problem(rng, S, n)
    ss = P.estimate_sample_scales(x_init, upper_quantile=0.8)
    z = rng.normal(0, 0.7, size=(S, Cdim)).astype(np.float32)
    kw = dict(kernel_regression_degree=deg, kernel_regression_bandwidth=bw, ctx=ctx)
    reg = P.RNASeqTranscriptLinearRegression(None if point else vars_, x_init, np.zeros_like(z), ss, use_distortion, pen, point, **kw)
    reg.set_latent_design(z, 1.0)
    np.testing.assert_array_equal(reg.get_design(), z)
    W = weights(x_init, deg, bw)
    p0 = RR.flatten(RR.initial_params(x_init, Cdim, deg), RR.PARAMS)
    theta = (p0 + rng.normal(0, 0.3, size=p0.size)).astype(np.float32)
    reg.set_flat_params(theta)
    eps = rng.normal(size=reg.num_noise).astype(np.float32)
    loss, g = reg.loss_and_gradients(noise=eps)
    gz = reg.design_gradient().astype(np.float64)

    common = dict(W=W, sample_scales=ss, x_bias_loc0=np.log(1.0 / n), x_bias_scale0=12.0, use_distortion=use_distortion,
                  scale_penalty=pen, use_point_estimates=point)
    e = RR.unflatten(eps.astype(np.float64), RR.NOISE, S, Cdim, n, deg)
    pp = RR.unflatten(theta.astype(np.float64), RR.PARAMS, S, Cdim, n, deg)
    z64 = z.astype(np.float64)
    loss_o, draws = pca_loss(pp, e, z64, 1.0, lik=None if point else _lik(vars_), **common)
    print("loss", loss, "restatement", loss_o)
    assert abs(loss - loss_o) <= 1e-4 * abs(loss_o) + 1e-2, (loss, loss_o)

    # the analytic z-gradient of the restatement, cross-checked against central differences of pca_loss (the likelihood term does
    # not depend on z: left out of the differences)
    gz_o = pca_z_gradient(pp, draws, z64, 1.0, W, ss, use_distortion)
    scale_o = np.abs(gz_o).max()
    h = 1e-4
    for s_ in range(S):
        for f in range(Cdim):
            zp, zm = z64.copy(), z64.copy()
            zp[s_, f] += h
            zm[s_, f] -= h
            fd = (pca_loss(pp, e, zp, 1.0, **common)[0] - pca_loss(pp, e, zm, 1.0, **common)[0]) / (2 * h)
            assert abs(gz_o[s_, f] - fd) <= 1e-5 * (abs(fd) + scale_o), (s_, f, gz_o[s_, f], fd)
    gscale = np.abs(gz).max()
    err = np.abs(gz - gz_o) / (np.abs(gz_o) + 2e-3 * gscale)
    print("z gradient: worst relative error", err.max())
    assert err.max() < 1e-2, (err.max(), gz, gz_o)

    # the flat-parameter gradient is that of a handle WITHOUT a latent design given the same design; the losses differ by the prior
    plain = P.RNASeqTranscriptLinearRegression(None if point else vars_, x_init, z, ss, use_distortion, pen, point, **kw)
    plain.set_flat_params(theta)
    loss_p, g_p = plain.loss_and_gradients(noise=eps)
    # (the same arithmetic up to the order of the float32 atomic sums behind the shared coefficients: rtol 1e-4 of the scale)
    np.testing.assert_allclose(g, g_p, rtol=1e-4, atol=1e-4 * np.abs(g_p).max())
    assert abs((loss - loss_p) - prior_nlp(z64, 1.0)) <= 1e-4 * abs(loss_o) + 1e-2

    # another prior scale changes the loss and the gradient as the formula says
    reg.set_latent_design(z, 2.5)
    loss2, g2 = reg.loss_and_gradients(noise=eps)
    gz2 = reg.design_gradient().astype(np.float64)
    assert abs((loss2 - loss) - (prior_nlp(z64, 2.5) - prior_nlp(z64, 1.0))) <= 1e-4 * abs(loss_o) + 1e-2
    gz2_o = pca_z_gradient(pp, draws, z64, 2.5, W, ss, use_distortion)
    err2 = np.abs(gz2 - gz2_o) / (np.abs(gz2_o) + 2e-3 * np.abs(gz2).max())
    assert err2.max() < 1e-2, (err2.max(), gz2, gz2_o)
    np.testing.assert_allclose(g2, g, rtol=1e-4, atol=1e-4 * np.abs(g).max())


def test_fit_trajectory_matches_restatement_adam(P, ctx):
    """Adam steps with supplied noise: the flat parameters AND z follow RR.adam_step(lr = 1e-3) driven by a shadow handle's per-step
    gradients, then a second fit continues the same trajectory: z shares the step clock.  (Supplied noise is enqueued directly, never
    replayed from the graph: the captured step with the update is what the reproducibility and planted-structure tests run.)"""
    rng = np.random.default_rng(52)
    S, Cdim, n, deg = 3, 2, 60, 4
    vars_, x_init = _problem(rng, S, n)
    ss = np.zeros((S, 1), np.float32)
    z0 = rng.normal(0, 0.5, size=(S, Cdim)).astype(np.float32)

    def make():
        r = P.RNASeqTranscriptLinearRegression(vars_, x_init, np.zeros_like(z0), ss, True, 0.5, False, kernel_regression_degree=deg,
                                               ctx=ctx)
        r.set_latent_design(z0, 1.0)
        _set_lr(P, r, 1e-3)
        return r
    reg, shadow = make(), make()
    first, more = 4, 3
    noise = rng.normal(size=(first + more, reg.num_noise)).astype(np.float32)
    theta = reg.get_flat_params().astype(np.float64)
    z = z0.astype(np.float64)
    m, v, mz, vz = np.zeros_like(theta), np.zeros_like(theta), np.zeros_like(z), np.zeros_like(z)
    losses = []

    def shadow_steps(t0, count):
        for t in range(t0, t0 + count):
            shadow.set_flat_params(theta.astype(np.float32))
            shadow.set_design(z.astype(np.float32))
            l, g = shadow.loss_and_gradients(noise=noise[t - 1])
            gz = shadow.design_gradient()
            losses.append(l)
            RR.adam_step(theta, g.astype(np.float64), m, v, t, lr=1e-3)
            RR.adam_step(z, gz.astype(np.float64), mz, vz, t, lr=1e-3)

    shadow_steps(1, first)
    out = reg.fit(first, noise=noise[:first], return_trace=True)
    np.testing.assert_allclose(out[-1], losses, rtol=2e-5)
    np.testing.assert_allclose(reg.get_flat_params(), theta, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(reg.get_design(), z, rtol=2e-4, atol=2e-5)
    assert np.abs(reg.get_design() - z0).max() > 1e-3  # (z moved: about lr per step)
    shadow_steps(first + 1, more)
    out = reg.fit(more, noise=noise[first:], return_trace=True)
    np.testing.assert_allclose(out[-1], losses[first:], rtol=2e-5)
    np.testing.assert_allclose(reg.get_flat_params(), theta, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(reg.get_design(), z, rtol=2e-4, atol=2e-5)


def test_device_rng_fits_are_reproducible(P, ctx):
    """Two RNASeqPCA fits with the same seeds (the captured step, device RNG): equal traces and z within the tolerance of the
    atomic-order sums, rtol 1e-4; another seed differs."""
    rng = np.random.default_rng(53)
    S, n = 4, 150
    vars_, x_init = _problem(rng, S, n)
    ss = P.estimate_sample_scales(x_init, upper_quantile=0.8)
    lik = P.RNASeqApproxLikelihood(vars_, ctx=ctx)
    runs = []
    for seed in (7, 7, 8):
        pca = P.RNASeqPCA(lik, x_init, ss, False, ctx=ctx)
        z, w, trace = pca.fit(50, seed=seed, return_trace=True)
        assert z.shape == (S, 2) and w.shape == (2, n) and np.all(np.isfinite(trace))
        runs.append((z, trace))
    np.testing.assert_allclose(runs[1][1], runs[0][1], rtol=1e-4)
    print("z: worst relative difference", np.max(np.abs(runs[1][0] - runs[0][0]) / np.abs(runs[0][0])))
    np.testing.assert_allclose(runs[1][0], runs[0][0], rtol=1e-4, atol=0)
    assert np.abs(runs[0][0]).max() > 1e-3
    assert not np.allclose(runs[2][1], runs[0][1], rtol=1e-4)


@pytest.mark.parametrize("point", [True, False])
def test_fit_separates_planted_groups(P, ctx, point):
    """S = 8 in two groups of 4, n = 400, 100 transcripts shifted by +-3 in the second group, log-noise 0.05, 3000 steps: along the
    centred component of largest variance the gap between the group means is at least 10 x the larger within-group standard
    deviation.  (CPU check of this model in float64 with point estimates: gap 1.07 against 0.004 at step 3000.)"""
    rng = np.random.default_rng(54)
    S, n = 8, 400
    tree = random_tree(n, rng)
    li, ri, fi = O.make_inverse_ptt_params(*tree)
    to = O.PTT(*tree)
    base = rng.normal(0, 1.0, size=n)
    effect = np.zeros(n)
    planted = rng.choice(n, 100, replace=False)
    effect[planted] = rng.choice([-3.0, 3.0], size=100)
    group = (np.arange(S) >= S // 2).astype(np.float64)
    mus, x_init = [], []
    for s in range(S):
        logx = base + group[s] * effect + rng.normal(0, 0.05, size=n)
        x = np.exp(logx - logx.max())
        x /= x.sum()
        y = np.clip(to.inverse_transform(x.astype(np.float32))[0], 1e-6, 1 - 1e-6)
        mus.append(np.log(y) - np.log1p(-y))
        x_init.append(np.log(x))
    x_init = np.array(x_init, np.float32)
    vars_ = dict(efflen=np.full((S, n), 1000.0, np.float32), la_mu=np.array(mus, np.float32),
                 la_sigma=np.full((S, n - 1), 0.05, np.float32), la_alpha=np.zeros((S, n - 1), np.float32), left_index=li[None],
                 right_index=ri[None], leaf_index=fi[None])
    ss = P.estimate_sample_scales(x_init, upper_quantile=0.9)
    pca = P.RNASeqPCA(None if point else vars_, x_init, ss, point, ctx=ctx)
    z, w, trace = pca.fit(3000, seed=5, return_trace=True)
    assert np.all(np.isfinite(trace)) and np.all(np.isfinite(z))
    first, last = trace[:200].mean(), trace[-200:].mean()
    zc = z.astype(np.float64) - z.mean(axis=0)
    t = zc[:, np.argmax(zc.var(axis=0))]
    gap = abs(t[S // 2:].mean() - t[:S // 2].mean())
    within = max(t[:S // 2].std(), t[S // 2:].std())
    print("point" if point else "likelihood", "loss", first, "->", last, "gap", gap, "within", within)
    assert last < first
    assert gap >= 10.0 * within, (gap, within, z)


def test_latent_design_argument_errors(P, ctx):
    rng = np.random.default_rng(55)
    S, n = 3, 40
    vars_, x_init = _problem(rng, S, n)
    ss = np.zeros(S, np.float32)
    # more components than REG_MAXF: refused where F is fixed, at the handle's creation, with that call's status (UNSUPPORTED = 5)
    with pytest.raises(P.PoleeError, match="at most 16 factors") as e17:
        P.RNASeqPCA(None, x_init, ss, True, latent_dimensionality=17, ctx=ctx)
    assert e17.value.status == 5
    reg = P.RNASeqTranscriptLinearRegression(None, x_init, np.zeros((S, 2), np.float32), ss, True, 1.0, True, ctx=ctx,
                                             kernel_regression_degree=5)
    z = rng.normal(size=(S, 2)).astype(np.float32)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(P.PoleeError, match="prior_scale") as eb:
            reg.set_latent_design(z, bad)
        assert eb.value.status == 1  # BAD_ARG
    with pytest.raises(ValueError):
        reg.set_latent_design(np.zeros((S, 3), np.float32))
    lib = P.lib()
    st = lib.polee_regression_get_design(reg._h, None)
    assert st == 1 and b"null" in lib.polee_last_error(ctx._h)
    # a gene-level model has no latent design
    G = 12
    gene_of = np.concatenate([np.arange(G), rng.integers(0, G, n - G)])
    x_gene_init = rng.normal(-np.log(G), 1.0, size=(S, G)).astype(np.float32)
    gene = P.RNASeqGeneLinearRegression(vars_, gene_of + 1, np.arange(1, n + 1), x_gene_init,
                                        rng.normal(size=(S, n)).astype(np.float32), None, np.ones((S, 2), np.float32), ss, True, 1.0,
                                        False, kernel_regression_degree=5, ctx=ctx)
    with pytest.raises(P.PoleeError) as ei:
        gene.set_latent_design(np.zeros((S, 2), np.float32))
    assert ei.value.status == 5 and "transcript-level" in str(ei.value)
    # set_design on a latent handle moves z (and get_design returns it); without the mode get_design is the creation's matrix
    np.testing.assert_array_equal(reg.get_design(), np.zeros((S, 2), np.float32))
    reg.set_latent_design(z, 1.0)
    z2 = rng.normal(size=(S, 2)).astype(np.float32)
    reg.set_design(z2)
    np.testing.assert_array_equal(reg.get_design(), z2)

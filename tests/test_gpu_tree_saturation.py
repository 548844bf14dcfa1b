"""Forward tree transforms at saturated nodes: a stick fraction of exactly 0 or 1 -- what the sampler's Float32 logistic gives from
a logit of 16.64 on, and the HSB op's double from 36.8 on -- kills a child's whole subtree in the reference's products.  The device
path is a prefix sum over the Euler tour of signed edge logs (ptt_forward_device; FwdLoad / FwdEmit of csrc/ptt_internal.hpp), where
such an edge is a -inf on ENTER and a +inf on EXIT unless it is counted instead of summed.  Every entry point that goes through
that path is compared with the oracle function that mirrors it, on the placements of tests/tree_ops_restatement.py (whose own
float64 recursion tests/test_tree_ops_host.py holds against the same oracle).

With the scan that summed the infinities (the library before the dead-edge count) the leaf-child control passes and every case with
a dead internal child fails: in test_sampler_rand[random-1100-internal_cross_chunk] the oracle has 5 leaves at the floor and the
device every leaf behind the dead child's EXIT, and transform is refused for its non-finite ladj."""
import numpy as np
import pytest

import tree_ops_restatement as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FLOOR32 = np.float32(1e-16)
CASES = R.sat_cases()

@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def ctx(P):
    return P.Context(0)


@pytest.fixture(scope="module")
def handles(P, ctx):
    cache = {}

    def get(kind, n):
        if (kind, n) not in cache:
            t, _ = R.sat_tree(kind, n)
            cache[kind, n] = (P.PolyaTreeTransform(t.parents, t.js, ctx=ctx), O.PTT(t.parents, t.js))
        return cache[kind, n]
    return get


def _floor_set(x, floor=FLOOR32):
    return set(np.flatnonzero(np.asarray(x) == floor).tolist())


def check_leaves(got, ref, rtol, atol, floor=FLOOR32):
    """the set of leaves at the floor is the oracle's, the live leaves meet the bound, the draw sums to 1"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert not np.isnan(got).any()
    assert _floor_set(got, floor) == _floor_set(ref, floor)
    live = ref != floor
    assert live.any()
    err = np.abs(got[live].astype(np.float64) - ref[live]) / (atol + rtol * np.abs(ref[live].astype(np.float64)))
    print("live %d of %d, worst error / bound %.3g" % (live.sum(), live.size, err.max()))
    np.testing.assert_allclose(got[live], ref[live], rtol=rtol, atol=atol)


@pytest.mark.parametrize("kind,n,name", CASES)
def test_transform(P, handles, kind, n, name):
    t, to = handles(kind, n)
    _, _, where, ys = R.sat_inputs(kind, n, name)
    y = R.saturate(ys[0], where)
    xs, ladj = t.transform(y, compute_ladj=True)
    xo, lo = to.transform(y, True)
    check_leaves(xs, xo, 3e-7, 0)
    assert abs(float(xs.astype(np.float64).sum()) - 1) < 1e-4
    assert R.ladj_matches(ladj, lo), (ladj, lo)
    xs2, _ = t.transform(y)  # (no ladj: the partial sums are not taken)
    assert xs2.tobytes() == xs.tobytes()


@pytest.mark.parametrize("kind,n,name", CASES)
@pytest.mark.parametrize("big", [40.0, 100.0])
def test_hsb(P, ctx, kind, n, name, big):
    tr, _ = R.sat_tree(kind, n)
    l, r, f = tr.index_arrays()
    _, _, where, ys = R.sat_inputs(kind, n, name)
    logit = R.saturated_logits(ys[0], where, big)
    x = P.hsb(logit, P.PolyaTreeTransform(ctx=ctx, index=(l, r, f)))[0]
    check_leaves(x, O.hsb(logit, l, r, f)[0], 1e-6, 0, np.float32(0))
    assert abs(float(x.astype(np.float64).sum()) - 1) < 1e-4


@pytest.mark.parametrize("kind,n,name", CASES)
def test_sampler_rand(P, handles, kind, n, name):
    t, to = handles(kind, n)
    _, _, where, _ = R.sat_inputs(kind, n, name)
    mu, sigma, alpha, z0, _ = R.sampler_params(n - 1, where, np.random.default_rng(n))
    als = P.ApproxLikelihoodSampler()
    als.set_transform(t, mu, sigma, alpha)
    x = als.rand(1, z0=z0[None])[0]
    check_leaves(x, O.sampler_draw(to, mu, sigma, alpha, z0), 2e-5, 1e-30)
    assert abs(float(x.astype(np.float64).sum()) - 1) < 1e-4


@pytest.mark.parametrize("kind,n,name", CASES)
def test_sampler_summaries(P, handles, kind, n, name):
    """posterior_mean, quantile and initial_values over draws of which every one has dead subtrees"""
    t, to = handles(kind, n)
    _, _, where, _ = R.sat_inputs(kind, n, name)
    rng = np.random.default_rng(n + 1)
    mu, sigma, alpha, _, eff = R.sampler_params(n - 1, where, rng)
    N = 9
    z0 = rng.normal(size=(N, n - 1)).astype(np.float32)
    als = P.ApproxLikelihoodSampler()
    als.set_transform(t, mu, sigma, alpha)
    draws = np.stack([O.sampler_draw(to, mu, sigma, alpha, z0[d]) for d in range(N)])
    dead = (draws == FLOOR32).all(axis=0)
    qs = (0.0, 0.5, 1.0)
    q = als.quantile(qs, N, z0=z0)
    assert (q[:, dead] == FLOOR32).all()
    np.testing.assert_allclose(q, np.quantile(draws.astype(np.float64), qs, axis=0), rtol=3e-5, atol=1e-30)
    pm = als.posterior_mean(N, z0=z0)
    acc = np.zeros(n, np.float32)
    for d in range(N):
        acc += np.clip(draws[d], np.float32(1e-15), np.float32(0.9999999))
    np.testing.assert_allclose(pm, acc / np.float32(N), rtol=3e-5, atol=1e-30)
    x0 = als.initial_values(eff, N, z0=z0)
    ref = np.zeros(n)
    for d in range(N):  # (these draws clamp y to [1e-10, 1 - 1e-10]: nothing is dead, the saturated sides are tiny)
        ref += O.x0_draw(to, mu, sigma, alpha, eff, z0[d])
    assert not np.isnan(x0).any()
    np.testing.assert_allclose(x0, ref / N, rtol=2e-5, atol=1e-12)


@pytest.mark.parametrize("kind,n,name", CASES)
def test_approx_sample_one_saturated_sample_beside_a_clean_one(P, ctx, kind, n, name):
    tr, _ = R.sat_tree(kind, n)
    l, r, f = tr.index_arrays()
    _, _, where, _ = R.sat_inputs(kind, n, name)
    rng = np.random.default_rng(n + 2)
    mu_s, sigma, alpha, z0, eff = R.sampler_params(n - 1, where, rng, ones=(40.0, 100.0))
    mu_c = R.sampler_params(n - 1, {}, rng)[0]
    mu, sg, al = np.stack([mu_s, mu_c]), np.stack([sigma, sigma]), np.stack([alpha, alpha])
    ef, z = np.stack([eff, eff]), np.stack([z0, z0])
    ap = P.RNASeqApproxLikelihood(dict(efflen=ef, la_mu=mu, la_sigma=sg, la_alpha=al, left_index=l, right_index=r, leaf_index=f),
                                  ctx=ctx)
    x = ap.sample(z)
    xo = O.tf_sampler(z, ef, mu, sg, al, l, r, f)
    for s in range(2):
        check_leaves(x[s], xo[s], 1e-4, 1e-16)
        assert abs(float(x[s].astype(np.float64).sum()) - 1) < 1e-4
    if kind != "spine":  # (a spine's deep leaves lie at the floor in either sample)
        assert _floor_set(x[0]) and not _floor_set(x[1])
    # the clean sample is, bit for bit, what it is without the saturated one beside it
    alone = P.RNASeqApproxLikelihood(dict(efflen=ef[1:], la_mu=mu[1:], la_sigma=sg[1:], la_alpha=al[1:], left_index=l,
                                          right_index=r, leaf_index=f), ctx=ctx).sample(z[1:])
    assert alone[0].tobytes() == x[1].tobytes()


@pytest.mark.parametrize("kind,n,name", CASES)
def test_streamed_sampler(P, ctx, kind, n, name):
    """the handle behind `polee sample` (sample.hip -> sampler_block_device), raw draws with supplied noise"""
    from polee_amd.sample import ApproxSampleStream
    tr, _ = R.sat_tree(kind, n)
    t, to = P.PolyaTreeTransform(tr.parents, tr.js, ctx=ctx), O.PTT(tr.parents, tr.js)
    _, _, where, _ = R.sat_inputs(kind, n, name)
    rng = np.random.default_rng(n + 3)
    mu, sigma, alpha, _, eff = R.sampler_params(n - 1, where, rng)
    N = 5
    z0 = rng.normal(size=(N, n - 1)).astype(np.float32)
    st = ApproxSampleStream(t, mu, sigma, alpha, eff, 100000, 7)
    raw = np.concatenate([st.next(2, raw=True, z0=z0[:2])["raw"], st.next(3, raw=True, z0=z0[2:])["raw"]])
    for d in range(N):
        check_leaves(raw[d], O.sampler_draw(to, mu, sigma, alpha, z0[d]), 2e-5, 1e-30)


@pytest.mark.parametrize("kind,n,name", CASES)
def test_saturated_row_between_clean_rows(P, handles, kind, n, name):
    t, to = handles(kind, n)
    _, _, where, ys = R.sat_inputs(kind, n, name, B=3)
    ys = np.array(ys)
    ys[1] = R.saturate(ys[1], where)
    xs, ladj = t.transform(ys, compute_ladj=True)
    clean, ladj_clean = t.transform(ys[[0, 2]], compute_ladj=True)
    assert xs[[0, 2]].tobytes() == clean.tobytes() and ladj[[0, 2]].tobytes() == ladj_clean.tobytes()
    for b in range(3):
        xo, lo = to.transform(ys[b], True)
        check_leaves(xs[b], xo, 3e-7, 0)
        assert R.ladj_matches(ladj[b], lo)


@pytest.mark.parametrize("kind,n", R.SAT_TREES[:4])
def test_large_negative_logits_that_do_not_saturate_stay_live(P, handles, kind, n):
    """mu = -17 and -30 leave y > 0 in Float32 (4e-8 and 9e-14): the left side is tiny, not dead.  On two nodes whose left
    child is a leaf that stays above the floor (tests/test_tree_ops_host.py holds the inputs to that)."""
    t, to = handles(kind, n)
    mu, sigma, alpha, z0, tids = R.near_saturated_sampler(kind, n)
    N = len(z0)
    draws = np.stack([O.sampler_draw(to, mu, sigma, alpha, z0[d]) for d in range(N)])
    assert (draws[:, tids] > FLOOR32).all() and (draws[:, tids] < 1e-6).all()
    als = P.ApproxLikelihoodSampler()
    als.set_transform(t, mu, sigma, alpha)
    x = als.rand(N, z0=z0)
    assert (x[:, tids] > FLOOR32).all()
    np.testing.assert_allclose(x, draws, rtol=2e-5, atol=1e-30)
    q = als.quantile((0.0, 1.0), N, z0=z0)
    assert (q[:, tids] > FLOOR32).all()
    np.testing.assert_allclose(q, np.quantile(draws.astype(np.float64), (0.0, 1.0), axis=0), rtol=3e-5, atol=1e-30)


def test_fixture_with_the_saturated_mu_of_real_prepared_samples(P, ctx, prep_fixture):
    """mu[5] = 30, mu[40] = -120, mu[100] = 17 on the golden prepared sample: the draw sums to 1 and has exactly the oracle's
    leaves at the floor, a couple of dozen of them"""
    t = P.PolyaTreeTransform(prep_fixture["node_parent_idxs"], prep_fixture["node_js"], ctx=ctx)
    to = O.PTT(prep_fixture["node_parent_idxs"], prep_fixture["node_js"])
    mu, sigma, alpha = prep_fixture["mu"].copy(), np.exp(prep_fixture["omega"]), prep_fixture["alpha"]
    mu[[5, 40, 100]] = (30.0, -120.0, 17.0)
    als = P.ApproxLikelihoodSampler()
    als.set_transform(t, mu, sigma, alpha)
    z0 = np.stack([O.randn(t.n - 1, 70 + d) for d in range(3)])
    xs = als.rand(3, z0=z0)
    for d in range(3):
        xo = O.sampler_draw(to, mu, sigma, alpha, z0[d])
        assert len(_floor_set(xo)) >= 20
        check_leaves(xs[d], xo, 2e-5, 1e-30)
        assert abs(float(xs[d].astype(np.float64).sum()) - 1) < 1e-4

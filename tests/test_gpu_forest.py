"""-m gpu: the forest of `polee model random-forest` grown on the device (polee_amd/random_forest.py, csrc/forest.hip) against the
library's host builder (csrc/forest_host.cpp) and the NumPy restatement (tests/forest_restatement.py).

There are no tolerances: node arrays (thresholds included) and votes are compared for exact equality.  On the sampler path the host
builder is fed the device's own rows (log_draws), because device logf and host log differ by an ulp; log_draws itself is held
against the log of the sampler's draws to within one ulp of f32."""
import numpy as np
import pytest

import forest_restatement as R
from conftest import random_tree
from oracle import oracle as O
from test_forest_host import SHAPES, assert_same_forest, nsubfeatures_for, shape_data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def ctx(P):
    return P.Context(0)


def _device(ctx, x, y, k, seed, **opts):
    from polee_amd.random_forest import RNASeqRandomForest
    f = RNASeqRandomForest(k, x.shape[1], ctx=ctx, **opts)
    f.fit(x, y, seed=seed)
    return f


def _check(ctx, x, y, k, seed, restate=True, **opts):
    """device == host builder (== restatement), and the device's votes on the training rows == the host's"""
    from polee_amd.random_forest import build_forest_host, forest_votes_host
    f = _device(ctx, x, y, k, seed, **opts)
    d = f.nodes()
    h = build_forest_host(x, y, k, seed, **opts)
    assert_same_forest(d, h)
    if restate:
        assert_same_forest(d, R.build_forest(x, y, k, seed, **opts))
    xv = x[:64]
    np.testing.assert_array_equal(f.votes(xv), forest_votes_host(h, xv, k))
    return d


@pytest.mark.parametrize("shape", SHAPES)
def test_fit_points_equals_host_builder_and_restatement(ctx, shape):
    N, n, k, nsub = shape
    x, y, f = shape_data(shape)
    d = _check(ctx, x, y, k, 11, ntrees=7, nsubfeatures=f)
    assert len(d[1]) >= 21
    _check(ctx, x, y, k, 11, restate=False, ntrees=7, nsubfeatures=f, partial_sampling=0.7)


@pytest.mark.parametrize("Nb", [1, 2, 63, 64, 65, 100, 257, 1100])
def test_root_sizes_across_the_wave_and_workgroup_paths(ctx, Nb):
    x, y = R.planted_data(np.random.default_rng(Nb), Nb, 8, 3, signal=2, constant=1)
    _check(ctx, x, y, 3, 5, ntrees=1 if Nb > 300 else 3)


def test_the_largest_bootstrap_and_one_row_more(ctx, P):
    from polee_amd.random_forest import FOREST_MAX_ROWS
    x, y = R.planted_data(np.random.default_rng(3), FOREST_MAX_ROWS + 1, 8, 2, signal=2, constant=1)
    d = _check(ctx, x[:-1], y[:-1], 2, 9, ntrees=1, max_depth=1)
    assert d[1].tolist()[1:] == [-1, -1] and d[1][0] >= 0
    with pytest.raises(P.PoleeError) as ei:
        _device(ctx, x, y, 2, 9, ntrees=1, max_depth=1)
    assert ei.value.status == 5  # POLEE_ERR_UNSUPPORTED


@pytest.mark.parametrize("k", [2, 3, 16])
def test_class_counts(ctx, k):
    x, y = R.planted_data(np.random.default_rng(k), 96, 130, k)
    _check(ctx, x, y, k, 2, ntrees=3, nsubfeatures=nsubfeatures_for(130, 11))


@pytest.mark.parametrize("n,nsub", [(5, 1), (5, 3), (5, 5), (130, 1), (130, 37), (130, 130), (1100, 1), (1100, 333), (1100, 1100)])
def test_feature_counts_and_candidate_chunks(ctx, n, nsub):
    x, y = R.planted_data(np.random.default_rng(n + nsub), 70, n, 3, constant=min(4, n - 1))
    _check(ctx, x, y, 3, 4, restate=nsub <= 130, ntrees=2, nsubfeatures=nsubfeatures_for(n, nsub))


@pytest.mark.parametrize("max_depth", [0, 1, -1])
@pytest.mark.parametrize("min_samples_leaf", [1, 3])
def test_depth_and_leaf_limits(ctx, max_depth, min_samples_leaf):
    x, y = R.planted_data(np.random.default_rng(12), 100, 20, 3)
    _check(ctx, x, y, 3, 6, ntrees=3, max_depth=max_depth, min_samples_leaf=min_samples_leaf)


def test_rounded_values_and_constant_columns(ctx):
    rng = np.random.default_rng(14)
    x = np.round(rng.normal(size=(150, 6)), 1).astype(np.float32)  # equal values carry different labels
    x[:, 4:] = np.float32(-0.5)
    x[::7, 0] = np.float32(-0.0)  # ... and a negative zero next to positive ones
    y = rng.integers(0, 3, 150).astype(np.int32)
    _check(ctx, x, y, 3, 8, ntrees=4)
    _check(ctx, np.full((9, 3), 0.25, np.float32), np.array([2, 1, 1, 2, 0, 1, 2, 0, 2], np.int32), 3, 8, ntrees=4)


def test_many_trees_share_a_level(ctx):
    x, y, f = shape_data(SHAPES[0])
    d = _check(ctx, x, y, 3, 21, ntrees=200, nsubfeatures=f)
    assert len(d[0]) == 201


# ---- the sampler path
_PROBLEMS = {}


def _problem(P, ctx, S, n):
    """random trees, per-sample parameters (the construction of tests/test_gpu_classify.py); built once per shape"""
    if (S, n) not in _PROBLEMS:
        rng = np.random.default_rng(1000 * S + n)
        trees = [random_tree(n, rng) for _ in range(S)]
        idx = [O.make_inverse_ptt_params(*tr) for tr in trees]
        L_, R_, F_ = (np.stack([i[j] for i in idx]) for j in range(3))
        vars_ = dict(efflen=rng.uniform(200, 3000, size=(S, n)).astype(np.float32),
                     la_mu=rng.normal(0, 1, size=(S, n - 1)).astype(np.float32),
                     la_sigma=np.exp(rng.normal(-1, 0.3, size=(S, n - 1))).astype(np.float32),
                     la_alpha=rng.normal(0, 0.3, size=(S, n - 1)).astype(np.float32), left_index=L_, right_index=R_, leaf_index=F_)
        _PROBLEMS[(S, n)] = P.RNASeqApproxLikelihood(vars_, ctx=ctx)
    return _PROBLEMS[(S, n)]


@pytest.mark.parametrize("n", [150, 1100])
def test_sampler_path(P, ctx, n):
    from polee_amd.random_forest import RNASeqRandomForest, build_forest_host, forest_votes_host, log_draws
    S, D, k = 5, 4, 2
    ap, ap_test = _problem(P, ctx, S, n), _problem(P, ctx, 4, n)
    rng = np.random.default_rng(n)
    z0 = rng.normal(size=(D, S, n - 1)).astype(np.float32)
    z0t = rng.normal(size=(3, 4, n - 1)).astype(np.float32)
    labels = np.array([0, 1, 0, 1, 1], np.int32)
    rows = log_draws(ap, D, z0=z0)
    assert rows.shape == (D * S, n) and np.isfinite(rows).all()
    for d in range(D):  # draw d of log_draws = the log of the sampler's draw with that slice of z0, to one ulp of f32
        ref = np.log(ap.sample(z0=z0[d].copy()).astype(np.float64))
        got = rows[d * S:(d + 1) * S].astype(np.float64)
        ulps = np.abs(got - ref) / np.spacing(np.maximum(np.abs(got), np.abs(ref)).astype(np.float32))
        print("log_draws, draw %d: worst distance from the f64 log %.3f ulp of f32" % (d, ulps.max()))
        assert (ulps <= 1.0).all()
    opts = dict(ntrees=5, nsubfeatures=nsubfeatures_for(n, 33 if n > 1000 else 12))
    f = RNASeqRandomForest(k, n, ctx=ctx, **opts)
    f.fit_sample(ap, labels, D, seed=31, z0=z0)
    h = build_forest_host(rows, np.tile(labels, D), k, 31, **opts)
    assert_same_forest(f.nodes(), h)
    v = f.votes_sample(ap_test, 3, z0=z0t)
    hv = forest_votes_host(h, log_draws(ap_test, 3, z0=z0t), k).reshape(3, 4, k).sum(axis=0)
    np.testing.assert_array_equal(v, hv)
    assert (v.sum(axis=1) == 5 * 3).all()
    np.testing.assert_array_equal(f.predict_sample(ap_test, 3, z0=z0t), hv / 15.0)
    # without z0 the device RNG draws: the same seed gives the same rows, and fit_sample sees them
    r1, r2 = log_draws(ap, 2, seed=7), log_draws(ap, 2, seed=7)
    np.testing.assert_array_equal(r1, r2)
    assert not np.array_equal(r1[:S], r1[S:])
    f.fit_sample(ap, labels, 2, draw_seed=7, seed=31)
    assert_same_forest(f.nodes(), build_forest_host(r1, np.tile(labels, 2), k, 31, **opts))


def test_set_nodes_with_a_hand_made_forest(P, ctx):
    from polee_amd.random_forest import RNASeqRandomForest
    # tree 0: x0 < 0.5 ? class 0 : class 1;  tree 1: x1 < -1 ? class 2 : (x0 < 0.5 ? class 2 : class 0)
    nodes = (np.array([0, 3, 8]), np.array([0, -1, -1, 1, -1, 0, -1, -1]), np.array([0.5, 0, 0, -1.0, 0, 0.5, 0, 0]),
             np.array([1, -1, -1, 1, -1, 3, -1, -1]), np.array([2, -1, -1, 2, -1, 4, -1, -1]), np.array([0, 0, 1, 0, 2, 0, 2, 0]))
    f = RNASeqRandomForest(3, 2, ctx=ctx)
    f.set_nodes(nodes)
    x = np.array([[0.0, 0.0], [0.5, 0.0], [0.75, -2.0], [0.25, -1.0], [np.nextafter(np.float32(0.5), np.float32(0)), -1.5]], np.float32)
    want = np.array([[1, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 0, 1]], np.int32)  # x == thr goes right
    np.testing.assert_array_equal(f.votes(x), want)
    np.testing.assert_array_equal(R.votes(nodes, x, 3), want)
    assert_same_forest(f.nodes(), nodes)
    np.testing.assert_array_equal(f.predict(x), want / 2.0)
    bad = [a.copy() for a in nodes]
    bad[3][0] = 0  # a child that is its own parent
    with pytest.raises(P.PoleeError):
        f.set_nodes(tuple(bad))
    bad = [a.copy() for a in nodes]
    bad[1][3] = 2  # a feature the forest does not have
    with pytest.raises(P.PoleeError):
        f.set_nodes(tuple(bad))
    # a host-built forest predicts on the device
    from polee_amd.random_forest import build_forest_host, forest_votes_host
    xs, ys, fr = shape_data(SHAPES[0])
    h = build_forest_host(xs, ys, 3, 3, ntrees=7, nsubfeatures=fr)
    g = RNASeqRandomForest(3, xs.shape[1], ctx=ctx)
    g.set_nodes(h)
    np.testing.assert_array_equal(g.votes(xs), forest_votes_host(h, xs, 3))


def test_reproducible_and_seeded(ctx):
    x, y, f = shape_data(SHAPES[2])
    a = _device(ctx, x, y, 16, 5, ntrees=7, nsubfeatures=f)
    b = _device(ctx, x, y, 16, 5, ntrees=7, nsubfeatures=f)
    assert_same_forest(a.nodes(), b.nodes())
    np.testing.assert_array_equal(a.votes(x), b.votes(x))
    c = _device(ctx, x, y, 16, 6, ntrees=7, nsubfeatures=f)
    assert len(c.nodes()[1]) != len(a.nodes()[1]) or not np.array_equal(c.nodes()[1], a.nodes()[1])


def test_non_finite_points_are_refused(P, ctx):
    x, y, f = shape_data(SHAPES[0])
    x = x.copy()
    x[2, 3] = -np.inf
    with pytest.raises(P.NonFiniteError):
        _device(ctx, x, y, 3, 5, ntrees=2)

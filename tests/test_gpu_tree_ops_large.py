"""The standalone tree operations, element by element, against the float64 recursions of tests/tree_ops_restatement.py at the sizes
where the scans' spine kernel changes regime: each of its 256 threads takes ceil(nchunks / 256) chunk totals, so more than one from
131 072 scanned elements on -- tours (3n - 2 entries) from n = 43 692, leaf-order scans from n = 131 073.  The sizes sit on both
sides of either threshold, with and without a partial last chunk; tests/test_tree_ops_host.py shows that these cases see a spine
that loses a thread's first total, a leaf prefix without its low word and a dropped tail element, and that the float64 reference
is good to a tenth of every bound used here.  Each test prints its worst error in units of its bound.

Measured on an MI355X: worst error / bound per operation and case (a value up to 1 passes).  xs 0 = the reference's Float32,
bit for bit; inv_hsb_grad's 0.5 is the Float32 rounding of the output; inv_hsb's y equals inverse_transform's.

    case              xs     ladj     y_grad   y_grad    inverse  inverse ladj  inv_hsb   hsb    inv_hsb
                                               no ladj   y        (ptt.jl)      ladj             _grad
    random 342        0      2.7e-6   7.0e-7   1.2e-6    0        3.9e-3        1.0e-3    0.29   0.5
    random 43691      0      5.1e-6   5.1e-7   1.3e-6    3.0e-4   3.6e-3        3.7e-3    0.59   0.5
    random 43692      0.21   1.7e-5   2.0e-6   6.9e-6    2.7e-4   3.6e-3        1.1e-3    0.54   0.5
    random 43862      0      1.4e-5   9.3e-7   4.7e-6    2.2e-4   3.6e-3        1.9e-3    0.58   0.5
    random 131072     0      5.0e-5   3.3e-6   1.7e-5    3.5e-4   3.9e-3        3.4e-3    0.59   0.5
    random 131073     0      7.6e-6   5.2e-7   1.9e-6    3.9e-4   3.8e-3        3.9e-3    0.66   0.5
    balanced 43692    0      1.7e-5   4.3e-7   3.4e-6    2.3e-4   3.5e-3        2.1e-3    0.47   0.5
    spine 43692       0      3.7e-5   1.0e-5   2.8e-5    1.1e-3   3.3e-3        3.1e-3    0.24   0.5
    balanced 131073   0.39   3.5e-5   3.9e-7   4.2e-6    2.3e-4   3.9e-3        4.3e-3    0.56   0.5
    spine 131073      0      1.7e-4   2.4e-5   2.7e-5    2.0e-3   3.3e-3        2.8e-3    0.25   0.5
    sampler draw, random 131073: 0.07"""
import numpy as np
import pytest

import tree_ops_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def ctx(P):
    return P.Context(0)


def _report(kind, n, err):
    print("scaled errors", kind, n, {k: "%.3g" % v for k, v in err.items()})
    assert all(v <= 1 for v in err.values()), err


@pytest.mark.parametrize("kind,n", R.LARGE_CASES)
def test_transform_and_gradients(P, ctx, kind, n):
    tr, d = R.large_tree(kind, n), R.large_inputs(kind, n)
    t = P.PolyaTreeTransform(tr.parents, tr.js, ctx=ctx)
    xs, ladj = t.transform(d["ys"], compute_ladj=True)
    yg = t.transform_gradients(d["ys"], d["x_grad"])
    yg0 = t.transform_gradients_no_ladj(d["ys"], d["x_grad"])
    _report(kind, n, R.scaled_errors(kind, n, dict(xs=xs, ladj=ladj, yg=yg, yg0=yg0)))


@pytest.mark.parametrize("kind,n", R.LARGE_CASES)
def test_inverse_and_tf_ops(P, ctx, kind, n):
    tr, d, ref = R.large_tree(kind, n), R.large_inputs(kind, n), R.large_reference(kind, n)
    t = P.PolyaTreeTransform(tr.parents, tr.js, ctx=ctx)
    ys, ladj = t.inverse_transform(d["x"])
    t2 = P.PolyaTreeTransform(ctx=ctx, index=tr.index_arrays())
    y_tf, ladj_tf = P.inv_hsb(d["x"], t2)
    hx = P.hsb(d["logit"], t2)
    bp = P.inv_hsb_grad(d["y_grad"], d["ladj_grad"], ref["inv_y"], t2)
    err = R.scaled_errors(kind, n, dict(inv_y=ys, inv_ladj_jl=ladj, inv_ladj_tf=ladj_tf[:, 0].astype(np.float64), hsb=hx, bp=bp))
    err["inv_hsb_y"] = R.scaled_errors(kind, n, dict(inv_y=y_tf))["inv_y"]
    _report(kind, n, err)


def test_rows_do_not_depend_on_the_batches_a_handle_has_seen(P, ctx):
    """one handle called with B = 1, then 5, then 2 (its scratch grows to the largest batch and stays): every row equals, bit for
    bit, the same input run alone on a fresh handle"""
    n = 1100
    tr = R.Tree(*R.build_tree(n, np.random.default_rng(11), "random"))
    rng = np.random.default_rng(12)
    t = P.PolyaTreeTransform(tr.parents, tr.js, ctx=ctx)
    for B in (1, 5, 2):
        ys = rng.uniform(0.05, 0.95, size=(B, n - 1))
        xg = rng.normal(size=(B, n)) * 10
        x = np.maximum(rng.dirichlet(np.ones(n) * 0.5, size=B).astype(np.float32), np.float32(1e-12))
        xs, ladj = t.transform(ys, compute_ladj=True)
        yg = t.transform_gradients(ys, xg)
        yg0 = t.transform_gradients_no_ladj(ys, xg)
        iy, il = t.inverse_transform(x)
        for b in range(B):
            fresh = P.PolyaTreeTransform(tr.parents, tr.js, ctx=ctx)
            xs1, ladj1 = fresh.transform(ys[b], compute_ladj=True)
            assert xs1.tobytes() == xs[b].tobytes() and ladj1 == ladj[b], (B, b)
            assert fresh.transform_gradients(ys[b], xg[b]).tobytes() == yg[b].tobytes(), (B, b)
            assert fresh.transform_gradients_no_ladj(ys[b], xg[b]).tobytes() == yg0[b].tobytes(), (B, b)
            iy1, il1 = fresh.inverse_transform(x[b])
            # (the inverse's ladj is summed by atomic adds across workgroups: its last bits depend on their order, not on the batch)
            assert iy1.tobytes() == iy[b].tobytes() and abs(il1 - il[b]) <= 1e-12 * abs(il[b]), (B, b)


def test_sampler_rand_at_131073(P, ctx):
    kind, n = "random", 131073
    tr, d = R.large_tree(kind, n), R.large_inputs(kind, n)
    t = P.PolyaTreeTransform(tr.parents, tr.js, ctx=ctx)
    rng = np.random.default_rng(n)
    mu, sigma, alpha, _, _ = R.sampler_params(n - 1, {}, rng)
    z0 = rng.normal(size=(2, n - 1)).astype(np.float32)
    als = P.ApproxLikelihoodSampler()
    als.set_transform(t, mu, sigma, alpha)
    xs = als.rand(2, z0=z0)
    ref = np.stack([R.sampler_draw(tr, mu, sigma, alpha, z0[b]) for b in range(2)])
    err = np.abs(xs.astype(np.float64) - ref) / (1e-30 + 2e-5 * np.abs(ref.astype(np.float64)))
    print("scaled errors sampler", n, "%.3g" % err.max())
    np.testing.assert_allclose(xs, ref, rtol=2e-5, atol=1e-30)

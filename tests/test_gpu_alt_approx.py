"""The alternative likelihood approximations on the GPU (polee_altvi, csrc/altvi.hip) against the NumPy f64 restatement of the
reference (tests/alt_approx_restatement.py), fed with the same noise: logistic_normal, normal_ilr, normal_alr.  Run with
`pytest -m gpu` on an MI355X.

Shapes: the reference fixture (n = 313, the tree of the prep fixture); a synthetic sample of n = 700, m = 14 000, whose Euler tour of
3 n - 2 = 2 098 entries spans five 512-entry scan chunks and whose leaves span two, with a caterpillar, a random and a balanced
tree (the caterpillar is the one a wrong chunk offset breaks); n = 2."""
import os
import subprocess
import sys

import numpy as np
import pytest

import alt_approx_restatement as R
from conftest import random_tree
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
METHODS = R.METHODS


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def ctx(P):
    return P.Context(0)


_cache = {}


def _data(name, lm_fixture):
    """dict(m, n, colptr, rowval, nzval, effective_lengths) of a shape, built once"""
    if name not in _cache:
        if name == "fixture":
            _cache[name] = lm_fixture
        elif name == "n700":
            from tools import synth
            smp = synth.make_sample(700, 14000, 4.0, 17)
            colptr, rowval, nzval = synth.to_csc(smp)
            _cache[name] = dict(m=14000, n=700, colptr=colptr, rowval=rowval, nzval=nzval, effective_lengths=smp["effective_lengths"])
        elif name == "n2":
            # 30 fragments over two transcripts: some compatible with one of them, some with both (CSC, 1-based)
            rng = np.random.default_rng(2)
            rows0 = np.sort(rng.choice(30, 20, replace=False))
            rows1 = np.sort(np.concatenate([np.setdiff1d(np.arange(30), rows0), rows0[:8]]))
            rowval = (np.concatenate([rows0, rows1]) + 1).astype(np.uint32)
            colptr = np.array([1, 1 + len(rows0), 1 + len(rows0) + len(rows1)], np.uint32)
            nzval = (rng.random(len(rowval)) * 1e-3 + 1e-5).astype(np.float32)
            _cache[name] = dict(m=30, n=2, colptr=colptr, rowval=rowval, nzval=nzval, effective_lengths=np.array([900.0, 1500.0], np.float32))
    return _cache[name]


def _tree_arrays(shape, kind, prep_fixture, n):
    if shape == "fixture":
        return prep_fixture["node_parent_idxs"], prep_fixture["node_js"]
    return random_tree(n, np.random.default_rng(n + len(kind)), kind)


def _setup(P, ctx, lm_fixture, prep_fixture, method, shape, kind):
    f = _data(shape, lm_fixture)
    n = f["n"]
    s = P.RNASeqSample(f["m"], n, f["colptr"], f["rowval"], f["nzval"], f["effective_lengths"], ctx=ctx)
    so = O.Sample(f["m"], n, f["colptr"], f["rowval"], f["nzval"])
    t = rt = None
    if method == "normal_ilr":
        parents, js = _tree_arrays(shape, kind, prep_fixture, n)
        t = P.PolyaTreeTransform(parents, js, ctx=ctx)
        rt = R.Tree(parents, js)
    # (ALR away from the fixture: a reference element in the middle, so that both sides of the index shift are taken)
    refidx = n if shape == "fixture" else max(1, n // 3)
    approx = {"logistic_normal": P.LogisticNormalApprox(), "normal_ilr": P.NormalILRApprox(),
              "normal_alr": P.NormalALRApprox(refidx)}[method]
    return f, n, s, so, t, rt, refidx, approx


ONE_STEP = ([(m, "fixture", "-") for m in METHODS]
            + [("normal_ilr", "n700", k) for k in ("spine", "random", "balanced")] + [("normal_ilr", "n2", "random")]
            + [(m, shape, "-") for m in ("logistic_normal", "normal_alr") for shape in ("n700", "n2")])


@pytest.mark.parametrize("method,shape,kind", ONE_STEP)
def test_one_step_gradients_match_the_restatement(P, ctx, lm_fixture, prep_fixture, method, shape, kind):
    """eval_gradients at spread parameters (mu ~ N(0, 2), omega ~ N(-1.5, 0.3)), the device's own noise exported and fed to the
    restatement.  Bounds as test_vi_single_step_gradients_match_oracle sets them; T = the sum of the absolute values of the terms
    that are added into a y_grad (ILR: |a| sum_left |l| + |b| sum_right |l| over the leaf gradients l)."""
    f, n, s, so, t, rt, refidx, approx = _setup(P, ctx, lm_fixture, prep_fixture, method, shape, kind)
    K = 6
    rng = np.random.default_rng(41)
    mu = rng.normal(0, 2, n - 1).astype(np.float32)
    omega = rng.normal(-1.5, 0.3, n - 1).astype(np.float32)
    fit = P.AltLikelihoodApproximationFit(s, approx, t, num_steps=2, num_mc_samples=K, gradonly=False, seed=99)
    fit.set_params(mu, omega)
    z = fit.export_noise(1)
    if n > 100:
        assert abs(z.mean()) < 0.1 and abs(z.std() - 1) < 0.05
    out = fit.eval_gradients()
    ref = R.step_gradients(method, so.log_likelihood, mu, omega, z, tree=rt, refidx=refidx)
    sigma = np.exp(omega.astype(np.float64))
    noise_mu = np.zeros(n - 1)
    noise_om = np.zeros(n - 1)
    for d in range(K):
        r = ref["draws"][d]
        np.testing.assert_allclose(out["xs"][d], r["xs"], rtol=1e-5)
        assert abs(out["lp"][d] - r["lp"]) <= 1e-6 * abs(r["lp"])
        assert abs(out["ladj"][d] - r["ladj"]) <= 1e-5 * max(1, abs(r["ladj"]))
        np.testing.assert_allclose(out["x_grad"][d], r["x_grad"], rtol=1e-4, atol=1e-6 * np.abs(r["x_grad"]).max())
        err = np.abs(out["y_grad"][d] - r["y_grad"])
        print(method, shape, kind, "draw", d, "max y_grad error / (T + 1):", (err / (r["terms"] + 1)).max())
        assert (err <= 2e-5 * (r["terms"] + 1)).all()
        noise_mu += r["terms"]
        noise_om += np.abs(sigma * z[d]) * r["terms"]
    for name, noise in (("mu_grad", noise_mu), ("omega_grad", noise_om)):
        rg = ref[name]
        assert (np.abs(out[name] - rg) <= 1e-4 * np.abs(rg) + 1e-5 * (noise / K + 1)).all(), name
    # the hook updates nothing
    mu1, om1 = fit.params()
    np.testing.assert_array_equal(mu1, mu)
    np.testing.assert_array_equal(om1, omega)
    assert fit.stats()["steps_done"] == 0


TRAJECTORY_SEED = 3  # (tests/test_alt_approx_host.py runs the Float32 restatement on these inputs under these bounds)


@pytest.mark.parametrize("method", METHODS)
def test_trajectory_with_supplied_noise(P, ctx, lm_fixture, prep_fixture, method):
    """Five steps, K = 6, supplied noise, on the fixture: initial values, then the parameters (at least 99 % within
    2e-4 (1 + |ref|): ADAM's first steps are sign-sensitive where a gradient is ~ 0), lp_mean and elbo."""
    f, n, s, so, t, rt, refidx, approx = _setup(P, ctx, lm_fixture, prep_fixture, method, "fixture", "-")
    steps, K = 5, 6
    z0 = O.randn(steps * K * (n - 1), TRAJECTORY_SEED).reshape(steps, K, n - 1)
    fit0 = P.AltLikelihoodApproximationFit(s, approx, t, num_steps=steps, num_mc_samples=K, z0=z0)
    mu0, om0 = fit0.params()
    rmu0, rom0 = R.initial_params(method, n)
    np.testing.assert_array_equal(mu0, rmu0)
    np.testing.assert_allclose(om0, rom0, rtol=0, atol=1e-6)
    ref = R.fit(method, so.log_likelihood, n, z0, tree=rt, refidx=refidx)
    got = P.approximate_likelihood(approx, s, t, num_steps=steps, num_mc_samples=K, z0=z0, gradonly=False)
    for key in ("mu", "omega"):
        ok = np.abs(got[key] - ref[key]) <= 2e-4 * (1 + np.abs(ref[key]))
        print(method, key, "within bound:", ok.mean())
        assert ok.mean() >= 0.99, (key, ok.mean())
    np.testing.assert_allclose(got["lp_mean"], ref["lp_mean"], rtol=1e-5)
    np.testing.assert_allclose(got["elbo"], ref["elbo"], rtol=1e-5)
    # the reference's Dicts
    want = {"logistic_normal": {"mu", "omega"}, "normal_ilr": {"mu", "omega", "node_parent_idxs", "node_js"},
            "normal_alr": {"mu", "omega", "refidx"}}[method]
    assert set(got) - {"elbo", "lp_mean"} == want
    if method == "normal_alr":
        assert got["refidx"].tolist() == [n]
    if method == "normal_ilr":
        assert (got["node_parent_idxs"] == prep_fixture["node_parent_idxs"]).all()


@pytest.mark.parametrize("method,shape,kind", [(m, "fixture", "-") for m in METHODS] + [("normal_ilr", "n700", "spine"), ("normal_alr", "n2", "-")])
def test_draws_match_the_restatement(P, ctx, lm_fixture, prep_fixture, method, shape, kind, tmp_path):
    """sample_likap on a file with supplied noise equals the restatement of evaluate.jl's function, rtol 1e-5; rows sum to 1.
    11 draws: one full batch of 8 and a short one."""
    from polee_amd import h5io
    f, n, s, so, t, rt, refidx, approx = _setup(P, ctx, lm_fixture, prep_fixture, method, shape, kind)
    rng = np.random.default_rng(8)
    params = {"mu": rng.normal(0, 2, n - 1).astype(np.float32), "omega": rng.normal(-1.5, 0.3, n - 1).astype(np.float32)}
    if method == "normal_ilr":
        params["node_parent_idxs"], params["node_js"] = t.node_parent_idxs, t.node_js
    if method == "normal_alr":
        params["refidx"] = np.array([refidx], np.int32)
    fn = str(tmp_path / "alt.h5")
    h5io.write_approximation(fn, f["m"], n, f["effective_lengths"], params, approx_type="Polee." + type(approx).__name__)
    count = 11
    z = O.randn(count * (n - 1), 12).reshape(count, n - 1)
    got = P.sample_likap(fn, count, z0=z, ctx=ctx)
    ref = R.sample_likap(method, params["mu"], params["omega"], f["effective_lengths"], z, tree=rt, refidx=refidx)
    assert got.shape == (count, n) and got.dtype == np.float32
    np.testing.assert_allclose(got, ref, rtol=1e-5)
    np.testing.assert_allclose(got.sum(axis=1, dtype=np.float64), 1.0, atol=1e-5)
    # without supplied noise: finite, normalised, draws differ, and the seed decides them
    a, b = P.sample_likap(fn, 3, seed=5, ctx=ctx), P.sample_likap(fn, 3, seed=5, ctx=ctx)
    np.testing.assert_array_equal(a, b)
    assert np.isfinite(a).all() and (a[0] != a[1]).any() and (a != P.sample_likap(fn, 3, seed=6, ctx=ctx)).any()


@pytest.mark.parametrize("method", METHODS)
def test_two_fits_are_bitwise_equal(P, ctx, lm_fixture, prep_fixture, method):
    """20 steps with the likelihood handle in deterministic mode, device noise: no float atomics anywhere else in the step"""
    f, n, s, so, t, rt, refidx, approx = _setup(P, ctx, lm_fixture, prep_fixture, method, "fixture", "-")
    s.set_deterministic(True)
    runs = [P.approximate_likelihood(approx, s, t, num_steps=20, num_mc_samples=6, seed=4, gradonly=False) for _ in range(2)]
    for key in ("mu", "omega", "elbo", "lp_mean"):
        assert runs[0][key].tobytes() == runs[1][key].tobytes(), key
    assert np.abs(runs[0]["mu"]).max() > 0


@pytest.mark.parametrize("method", METHODS)
def test_a_fit_fits(P, ctx, lm_fixture, prep_fixture, method):
    """500 steps, K = 6, device noise, on the fixture: the mean log-likelihood over 64 fresh draws at the fitted parameters is
    finite and above that at the initial parameters.  A sanity check; it fixes no number."""
    f, n, s, so, t, rt, refidx, approx = _setup(P, ctx, lm_fixture, prep_fixture, method, "fixture", "-")

    def mean_lp(mu, omega):
        lps = []
        for seed in range(1000, 1008):  # 8 x 8 fresh draws
            probe = P.AltLikelihoodApproximationFit(s, approx, t, num_steps=1, num_mc_samples=8, gradonly=False, seed=seed)
            probe.set_params(mu, omega)
            lps.append(probe.eval_gradients()["lp"])
        return float(np.mean(lps))
    fit = P.AltLikelihoodApproximationFit(s, approx, t, num_steps=500, num_mc_samples=6, seed=31)
    before = mean_lp(*fit.params())
    fit.run(500)
    fit.sync()
    assert fit.stats()["steps_done"] == 500 and fit.stats()["nonfinite_step"] == 0
    after = mean_lp(*fit.params())
    print(method, "mean lp before", before, "after", after)
    assert np.isfinite(after) and after > before


def test_prep_to_sample_likap(P, ctx, tmp_path):
    """python -m polee_amd.prep <lm> --approx-method normal_ilr -o out.h5, then sample_likap(out.h5, 5)"""
    from polee_amd import h5io
    lm = os.path.join(GOLDEN, "mBr_M_6w_1.likelihood-matrix.h5")
    out = str(tmp_path / "out.h5")
    r = subprocess.run([sys.executable, "-m", "polee_amd.prep", lm, "--approx-method", "normal_ilr", "-o", out, "--no-efflen-jacobian"],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Using alternative approximation. Some features not supported." in r.stderr
    assert "--no-efflen-jacobian has no effect" in r.stderr
    ps = h5io.read_prepared_sample(out)
    assert ps["metadata"]["approximation"] == "Polee.NormalILRApprox" and "alpha" not in ps
    n = ps["n"]
    assert ps["mu"].shape == (n - 1,) and ps["node_js"].shape == (2 * n - 1,)
    xs = P.sample_likap(out, 5, ctx=ctx)
    assert xs.shape == (5, n) and np.isfinite(xs).all()
    np.testing.assert_allclose(xs.sum(axis=1, dtype=np.float64), 1.0, atol=1e-5)
    # the default type through the same entry: the existing sampler
    d = str(tmp_path / "default.h5")
    h5io.write_approximation(d, ps["m"], n, ps["effective_lengths"],
                             dict(mu=ps["mu"], omega=ps["omega"], alpha=np.zeros(n - 1, np.float32), node_parent_idxs=ps["node_parent_idxs"],
                                  node_js=ps["node_js"]))
    xd = P.sample_likap(d, 4, ctx=ctx)
    assert xd.shape == (4, n) and np.isfinite(xd).all()
    np.testing.assert_allclose(xd.sum(axis=1, dtype=np.float64), 1.0, atol=1e-5)
    with pytest.raises(ValueError, match="only LogitSkewNormalPTTApprox can be used here"):
        P.polee_sample(out, str(tmp_path / "x.csv"), num_samples=2, ctx=ctx)

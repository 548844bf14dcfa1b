"""The alternative likelihood approximations (prep --approx-method) without a GPU: the NumPy restatement that the GPU tests use as
their yardstick (tests/alt_approx_restatement.py) checked against finite differences, the Float32 noise floor of the reference's
own arithmetic under the GPU trajectory test's bounds, the host routines of the library, the sanitizer driver, the files and the
command line.  Built: logistic_normal, normal_ilr, normal_alr."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import alt_approx_restatement as R
from conftest import random_tree
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polee_amd", "csrc")


def _toy_likelihood(n, rng):
    """lp(x) = sum_i log(A x)_i in f64 for a small dense positive A"""
    A = rng.random((3 * n, n)) + 0.05

    def ll(x):
        x = np.asarray(x, np.float64)
        p = A @ x
        return float(np.log(p).sum()), A.T @ (1 / p)
    return ll


def _fd(f, y, h=1e-6):
    g = np.zeros_like(y)
    for i in range(len(y)):
        e = np.zeros_like(y); e[i] = h
        g[i] = (f(y + e) - f(y - e)) / (2 * h)
    return g


def _logdet(method, ys, **kw):
    """log |det d x[free] / d y| by central differences; the free coordinates leave out one element (the last, or the reference one)"""
    n = len(ys) + 1
    drop = kw.get("refidx", n) - 1 if method == "normal_alr" else n - 1
    keep = np.arange(n) != drop
    J = np.zeros((n - 1, n - 1))
    h = 1e-6
    for i in range(n - 1):
        e = np.zeros(n - 1); e[i] = h
        J[:, i] = (R.forward(method, ys + e, **kw)[0][keep] - R.forward(method, ys - e, **kw)[0][keep]) / (2 * h)
    return np.linalg.slogdet(J)[1]


@pytest.mark.parametrize("kind", ["random", "spine", "balanced"])
def test_ilr_ladj_is_the_log_determinant(kind):
    """ilr_ladj = sum log x + log sqrt(n) (isometric_log_ratios.jl:77-83) is log |det d x[1:n-1] / d y| of y -> x, n = 5, with
    x[n] the dependent coordinate: no constant is dropped, log sqrt(n) included."""
    rng = np.random.default_rng(5)
    n = 5
    t = R.Tree(*random_tree(n, rng, kind))
    for _ in range(4):
        ys = rng.normal(0, 1.5, n - 1)
        ladj = R.forward("normal_ilr", ys, tree=t)[1]
        assert abs(ladj - _logdet("normal_ilr", ys, tree=t)) < 1e-6


@pytest.mark.parametrize("refidx", [5, 1, 3])
def test_alr_ladj_as_written(refidx):
    """alr_ladj = sum(ys) - log(1 + sum(exp.(ys))) (additive_log_ratios.jl:27) is NOT log |det J| of the transform: that is
    sum_i log x_i over all n elements = sum(ys) - n log(1 + sum exp ys).  The reference's value lacks (n - 1) log(1 + sum exp ys),
    which is no constant.  The literal formula is pinned, and the relation to the true determinant stated, n = 5."""
    rng = np.random.default_rng(6)
    n = 5
    for _ in range(4):
        ys = rng.normal(0, 1.5, n - 1)
        xs, ladj = R.forward("normal_alr", ys, refidx=refidx)
        assert abs(ladj - (ys.sum() - np.log1p(np.exp(ys).sum()))) < 1e-12
        true = _logdet("normal_alr", ys, refidx=refidx)
        assert abs(true - np.log(xs).sum()) < 1e-6
        assert abs(ladj - (n - 1) * np.log1p(np.exp(ys).sum()) - true) < 1e-6
        # the reference element sits where refidx says
        assert abs(xs[refidx - 1] - 1 / (1 + np.exp(ys).sum())) < 1e-12


@pytest.mark.parametrize("kind,n", [("random", 9), ("spine", 7), ("balanced", 8), ("random", 2)])
def test_ilr_gradients_are_the_gradient_of_lp_plus_ladj(kind, n):
    """ilr_transform_gradients! (isometric_log_ratios.jl:91-128) with dladj_dxi = 1 / xs[i] is the true gradient of
    lp(x(y)) + ilr_ladj(y) (no clamp binds here)."""
    rng = np.random.default_rng(n)
    t = R.Tree(*random_tree(n, rng, kind))
    ll = _toy_likelihood(n, rng)
    ys = rng.normal(0, 1, n - 1)
    xs, ladj, state = R.ilr_transform(t, ys)
    lp, g = ll(xs)
    yg = R.ilr_transform_gradients(t, xs, g, state)
    fd = _fd(lambda y: ll(R.forward("normal_ilr", y, tree=t)[0])[0] + R.forward("normal_ilr", y, tree=t)[1], ys)
    np.testing.assert_allclose(yg, fd, rtol=1e-6, atol=1e-6)
    T = R.ilr_ygrad_terms(t, xs, g, state)
    assert (T >= np.abs(yg) - 1e-12).all()


@pytest.mark.parametrize("refidx,n", [(6, 6), (1, 6), (4, 7), (2, 2)])
def test_alr_gradients_are_the_gradient_of_lp_plus_ladj_as_written(refidx, n):
    """alr_transform_gradients! (additive_log_ratios.jl:49-71): `1 - xs[i]` is the gradient of the ladj AS WRITTEN (:27), so
    y_grad is the true gradient of lp + alr_ladj -- of the reference's objective, not of the change of variables."""
    rng = np.random.default_rng(n + refidx)
    ll = _toy_likelihood(n, rng)
    ys = rng.normal(0, 1, n - 1)
    xs, _ = R.alr_transform(refidx, ys)
    lp, g = ll(xs)
    yg = R.alr_transform_gradients(refidx, xs, g)
    fd = _fd(lambda y: ll(R.forward("normal_alr", y, refidx=refidx)[0])[0] + R.forward("normal_alr", y, refidx=refidx)[1], ys)
    np.testing.assert_allclose(yg, fd, rtol=1e-6, atol=1e-6)


def test_logistic_normal_gradients_pin_the_literal_formula():
    """likelihood-approximation-alt.jl:138-160.  The likelihood part, xs[i] x_grad[i] - xs[i] c, is the true gradient of lp(x(y)).
    The ladj part (:148-155) takes xsum AFTER normalisation (xsum = 1 - xs[n]), where one would expect the sum of exp(ys); with
    that xsum, ln_ladj = log(1 + xsum) + sum log xs[1:n-1] (:157-160) is what the fit adds to lp, and the formula of :154 as written
    turns out to be its gradient.  Both are pinned literally; the sum is the gradient of lp + ln_ladj."""
    rng = np.random.default_rng(11)
    n = 6
    ll = _toy_likelihood(n, rng)
    ys = rng.normal(0, 1, n - 1)
    xs = R.forward("logistic_normal", ys)[0]
    lp, g = ll(xs)
    yg, ladj = R.logistic_normal_gradients(xs, g)
    fd_lp = _fd(lambda y: ll(R.forward("logistic_normal", y)[0])[0], ys)
    xsum = xs[:-1].sum()
    literal = (1 / (1 + xsum)) * (xs[:-1] - xs[:-1] * xsum) + 1 - xs[:-1] * (n - 1)
    np.testing.assert_allclose(yg - literal, fd_lp, rtol=1e-6, atol=1e-6)
    assert abs(ladj - (np.log(1 + xsum) + np.log(xs[:-1]).sum())) < 1e-12
    fd_ladj = _fd(lambda y: R.forward("logistic_normal", y)[1], ys)
    np.testing.assert_allclose(literal, fd_ladj, rtol=1e-6, atol=1e-6)
    # it is not the log-determinant of y -> x[1:n-1], which is sum log x over all n elements
    assert abs(ladj - _logdet("logistic_normal", ys)) > 1e-2
    assert abs(np.log(xs).sum() - _logdet("logistic_normal", ys)) < 1e-6


def _trajectory_inputs(lm_fixture, prep_fixture, seed):
    f = lm_fixture
    so = O.Sample(f["m"], f["n"], f["colptr"], f["rowval"], f["nzval"])
    steps, K = 5, 6
    z0 = O.randn(steps * K * (f["n"] - 1), seed).reshape(steps, K, f["n"] - 1)
    tree = R.Tree(prep_fixture["node_parent_idxs"], prep_fixture["node_js"])
    return so, z0, tree


TRAJECTORY_SEED = 3


@pytest.mark.parametrize("method", R.METHODS)
def test_float32_noise_floor_meets_the_trajectory_bounds(method, lm_fixture, prep_fixture):
    """The restatement with Float32 where the reference keeps Float32 against itself in f64, on the GPU trajectory test's inputs
    (the fixture, five steps, K = 6, noise seed 3) and under that test's bounds: the cap can be met by the reference's own
    arithmetic."""
    so, z0, tree = _trajectory_inputs(lm_fixture, prep_fixture, TRAJECTORY_SEED)
    n = lm_fixture["n"]
    ref = R.fit(method, so.log_likelihood, n, z0, tree=tree, refidx=n)
    f32 = R.fit(method, so.log_likelihood, n, z0, tree=tree, refidx=n, f32=True)
    for key in ("mu", "omega"):
        ok = np.abs(f32[key] - ref[key]) <= 2e-4 * (1 + np.abs(ref[key]))
        print(method, key, "within bound:", ok.mean())
        assert ok.mean() >= 0.99, (key, ok.mean())
    np.testing.assert_allclose(f32["lp_mean"], ref["lp_mean"], rtol=1e-5)
    np.testing.assert_allclose(f32["elbo"], ref["elbo"], rtol=1e-5)


def test_initial_values_and_step_clamps():
    """mu = 0; omega = 0.1 for the logistic-normal (:79), log(0.1f0) for ILR and ALR (:536, 655); clamps 2e-2 / 2e-1"""
    mu, om = R.initial_params("logistic_normal", 4)
    assert (mu == 0).all() and (om == np.float32(0.1)).all() and R.max_step("logistic_normal") == 2e-2
    for m in ("normal_ilr", "normal_alr"):
        mu, om = R.initial_params(m, 4)
        assert (mu == 0).all() and (om == np.log(np.float32(0.1))).all() and R.max_step(m) == 2e-1


@pytest.mark.parametrize("kind,n", [("random", 300), ("spine", 60), ("balanced", 257), ("random", 2)])
def test_ilr_coefficient_table_matches_the_restatement(kind, n):
    import ctypes as C
    from polee_amd import _lib as L
    t = R.Tree(*random_tree(n, np.random.default_rng(n), kind))
    a, b, r, s = t.coefficients()
    r32, s32 = r.astype(np.int32), s.astype(np.int32)
    ab = np.zeros((n - 1, 2))
    L.check(L.lib().polee_ilr_coefficients(L.ptr(r32, L.i32p), L.ptr(s32, L.i32p), C.c_int64(n - 1), L.ptr(ab, L.f64p)))
    np.testing.assert_allclose(ab[:, 0], a, rtol=1e-15)
    np.testing.assert_allclose(ab[:, 1], b, rtol=1e-15)
    assert (r + s)[0] == n
    with pytest.raises(L.PoleeError):
        L.check(L.lib().polee_ilr_coefficients(L.ptr(np.zeros(1, np.int32), L.i32p), L.ptr(s32, L.i32p), C.c_int64(1), L.ptr(ab, L.f64p)))


def test_default_opts_are_the_references_constants():
    import ctypes as C
    from polee_amd import _lib as L
    for method, step in ((1, 2e-2), (4, 2e-1), (5, 2e-1)):
        o = L.AltViOpts()
        L.lib().polee_altvi_default_opts(C.c_int32(method), C.byref(o))
        assert (o.method, o.num_steps, o.num_mc_samples, o.gradonly, o.refidx) == (method, 500, 6, 1, -1)
        assert (o.max_step0, o.max_step1, o.eps, o.adam_rm, o.adam_rv) == (step, step, 1e-10, 0.7, 0.9)


def test_host_parts_clean_under_sanitizer():
    """tests/san/alt_approx_main.cpp: a stand-alone driver, built host-only with address,undefined and run on the CPU"""
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    subprocess.check_call(["make", "-s", "-C", CSRC, "_obj/san_address_undefined/alt_approx_check", "SAN=address,undefined"],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([os.path.join(CSRC, "_obj", "san_address_undefined", "alt_approx_check")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ok" in r.stdout


# ---- files -------------------------------------------------------------------------------------------------------------------------
def _params(typ, n, rng):
    p = {"mu": rng.normal(size=n - 1).astype(np.float32), "omega": rng.normal(size=n - 1).astype(np.float32)}
    if typ == "NormalILRApprox":
        p["node_parent_idxs"], p["node_js"] = random_tree(n, rng)
    if typ == "NormalALRApprox":
        p["refidx"] = np.array([n], np.int32)
    return p


@pytest.mark.parametrize("typ", ["LogisticNormalApprox", "NormalILRApprox", "NormalALRApprox"])
def test_alternative_fit_round_trips_through_the_file(typ, tmp_path):
    from polee_amd import h5io
    rng = np.random.default_rng(2)
    n = 7
    p = _params(typ, n, rng)
    eff = (rng.random(n) * 900 + 100).astype(np.float32)
    fn = str(tmp_path / "alt.h5")
    h5io.write_approximation(fn, 50, n, eff, p, approx_type="Polee." + typ)
    back = h5io.read_prepared_sample(fn)
    assert back["metadata"]["approximation"] == "Polee." + typ and back["n"] == n and back["m"] == 50
    assert "alpha" not in back and "beta" not in back
    for key, val in p.items():
        assert back[key].dtype == (np.float32 if key in ("mu", "omega") else np.int32)
        np.testing.assert_array_equal(back[key], val)
    if typ != "NormalILRApprox":
        assert back["node_parent_idxs"] is None and back["node_js"] is None
    if typ != "NormalALRApprox":
        assert "refidx" not in back


def test_default_file_is_byte_identical_to_the_golden_one(tmp_path, monkeypatch):
    """tests/golden/prepared_default_before_alt.h5 was written by write_approximation as it stood before it learnt the alternative
    types (mu / omega / alpha + tree, fixed arrays below, date attribute frozen): the same call gives the same bytes, the object headers'
    modification times aside."""
    import datetime
    from polee_amd import h5io
    golden = os.path.join(ROOT, "tests", "golden", "prepared_default_before_alt.h5")

    class Frozen(datetime.datetime):
        @classmethod
        def now(cls, tz=None):
            return cls(2020, 1, 2, 3, 4, 5, 678901)
    monkeypatch.setattr(h5io.datetime, "datetime", Frozen)
    rng = np.random.default_rng(1234)
    n = 9
    parents, js = random_tree(n, rng)
    p = {"mu": rng.normal(size=n - 1).astype(np.float32), "omega": rng.normal(size=n - 1).astype(np.float32),
         "alpha": rng.normal(size=n - 1).astype(np.float32), "node_parent_idxs": parents, "node_js": js}
    eff = (rng.random(n) * 900 + 100).astype(np.float32)
    fn = str(tmp_path / "default.h5")
    h5io.write_approximation(fn, 77, n, eff, p, gfffilename="a.gff3", gffhash=b"\x01\x02", fafilename="g.fa", fahash=b"\x03", args="x -o y")
    got, want = bytearray(open(fn, "rb").read()), open(golden, "rb").read()
    assert len(got) == len(want)
    # (HDF5 itself stamps every object header with the time of writing, 4 bytes each: the only bytes two runs of one writer differ in)
    for off in (932, 1532, 1812, 4236, 4508, 4780, 5044, 5492):
        got[off:off + 4] = want[off:off + 4]
    assert bytes(got) == want
    back = h5io.read_prepared_sample(fn)
    for key in ("mu", "omega", "alpha", "node_parent_idxs", "node_js"):
        np.testing.assert_array_equal(back[key], p[key])


def test_sample_command_refuses_an_alternative_file(tmp_path):
    from polee_amd import h5io
    rng = np.random.default_rng(3)
    fn = str(tmp_path / "ilr.h5")
    h5io.write_approximation(fn, 50, 7, np.ones(7, np.float32), _params("NormalILRApprox", 7, rng), approx_type="Polee.NormalILRApprox")
    r = subprocess.run([sys.executable, "-m", "polee_amd.sample", fn], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0
    assert ("%s holds a NormalILRApprox; only LogitSkewNormalPTTApprox can be used here (draw from it with polee_amd.sample_likap)" % fn) in r.stderr
    assert "Traceback" not in r.stderr
    # the model loaders say the same
    from polee_amd import estimate
    with pytest.raises(ValueError, match="holds a NormalILRApprox; only LogitSkewNormalPTTApprox can be used here"):
        estimate.load_samples_hdf5([fn], 7, using_device=False)


# ---- command line and exports ----------------------------------------------------------------------------------------------------
def test_approx_method_names_and_exports():
    import polee_amd as P
    from polee_amd import prep
    want = {"logit_skew_normal_ptt": P.LogitSkewNormalPTTApprox, "logistic_normal": P.LogisticNormalApprox,
            "kumaraswamy_ptt": P.KumaraswamyPTTApprox, "logit_normal_ptt": P.LogitNormalPTTApprox,
            "normal_ilr": P.NormalILRApprox, "normal_alr": P.NormalALRApprox}
    for name, typ in want.items():
        a = prep.select_approx_method(name, "sequential")
        assert type(a) is typ
        if hasattr(a, "treemethod"):
            assert a.treemethod == "sequential"
    assert prep.select_approx_method("normal_alr", "cluster").reference_idx == -1
    with pytest.raises(ValueError):
        prep.select_approx_method("normal_clr", "cluster")
    with pytest.raises(SystemExit):  # a seventh name is rejected by the parser
        prep.main(["x.h5", "--approx-method", "normal_clr"])
    for name in ("AltLikelihoodApproximationFit", "sample_likap", "approximation_type"):
        assert hasattr(P, name)
    # evaluate.jl:12-25: prefixes stripped, the old HSB names accepted
    assert P.approximation_type("Polee.NormalILRApprox") is P.NormalILRApprox
    assert P.approximation_type("Extruder.LogitNormalHSBApprox") is P.LogitNormalPTTApprox
    assert P.approximation_type("LogitSkewNormalHSBApprox") is P.LogitSkewNormalPTTApprox
    assert P.approximation_type("KumaraswamyHSBApprox") is P.KumaraswamyPTTApprox
    with pytest.raises(ValueError):
        P.approximation_type("Polee.Nothing")


def test_prep_messages_for_what_is_not_built(capsys):
    from polee_amd import prep
    for name in ("kumaraswamy_ptt", "logit_normal_ptt", "optimize"):
        with pytest.raises(SystemExit) as e:
            prep.main(["x.h5", "--approx-method", name])
        assert "not built" in str(e.value)
    with pytest.raises(SystemExit) as e:
        prep.main(["--salmon", "dir", "--ptt-tree", "t.h5", "--approx-method", "normal_ilr"])
    assert "--salmon" in str(e.value)
    assert "Using alternative approximation. Some features not supported." in capsys.readouterr().err

"""EM maximum-likelihood estimate on the GPU (csrc/em.hip, polee_amd.em; `polee debug-optimize`, src/em.jl) against the NumPy
restatement of tests/test_em_host.py.  The likelihood is flat near its maximum (the abundances of the f32 and the f64 restatement
differ by up to 3 % after 2 000 iterations), so results of several iterations are compared in LOG-LIKELIHOOD, always re-evaluated
in f64 NumPy (lp64), never component by component."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT  # noqa: F401
from test_em_host import Problem, expand_rows, reference_stop_iteration, run_em, subset_csc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def ctx(P):
    return P.Context(0)


@pytest.fixture(scope="module")
def prob(lm_fixture):
    return Problem.from_csc(lm_fixture)


@pytest.fixture(scope="module")
def runs(prob):
    """The f64 restatement over 3 000 iterations and the f32 one over 1 000: (y64, lps64, lps32)."""
    y64, l64 = run_em(prob, 3000)
    _, l32 = run_em(prob, 1000, np.float32)
    return y64, l64, l32


def _sample(P, ctx, lm, ks=None, deterministic=False):
    s = P.RNASeqSample(lm["m"], lm["n"], lm["colptr"], lm["rowval"], lm["nzval"], lm["effective_lengths"], ks=ks, ctx=ctx)
    if deterministic:
        s.set_deterministic(True)
    return s


def _em(P, ctx, lm, y0=None, **kw):
    from polee_amd.em import EM
    return EM(_sample(P, ctx, lm, **kw), y0)


def _delta(l64, l32, T):
    """How far below the f64 restatement a device result may fall after T iterations: ten times what NumPy's f32 loses (another
    summation order, float atomics, hardware reciprocal and log come on top), at least 1e-3 (0.4 iterations' worth at T = 200)."""
    return max(10.0 * abs(l64[T - 1] - l32[T - 1]), 1e-3)


def _norm64(y):
    y = np.asarray(y, np.float64)
    return y / y.sum()


# ---- 1. one step -----------------------------------------------------------------------------------------------------------------
def test_one_step_matches_the_restatement(P, ctx, lm_fixture, prob):
    em = _em(P, ctx, lm_fixture)
    info = em.run(1, -1.0)
    y = em.mixture()
    want, lps = run_em(prob, 1)
    assert info["iters"] == 1 and info["M"] == 19743 and not info["converged"]
    assert abs(float(y.astype(np.float64).sum()) - 1) <= 1e-6
    np.testing.assert_allclose(y, want, rtol=1e-4, atol=0)
    assert abs(info["lp_start"] - -364724.375) <= 1e-6 * 364724.375
    assert abs(info["last_lp"] - lps[0]) <= 1e-6 * abs(lps[0])


# ---- 2., 3. trajectory and reported lp -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [10, 200, 1000])
def test_trajectory_in_log_likelihood(P, ctx, lm_fixture, prob, runs, T):
    _, l64, l32 = runs
    em = _em(P, ctx, lm_fixture)
    info = em.run(T, -1.0)
    assert info["iters"] == T and not info["converged"]
    y = em.mixture()
    lp = prob.lp64(_norm64(y))
    delta = _delta(l64, l32, T)
    print("T = %d: lp64(device) - lp64(f64 restatement) = %.3g (f32 restatement: %.3g; allowed -%.3g)"
          % (T, lp - l64[T - 1], l32[T - 1] - l64[T - 1], delta))
    assert lp >= l64[T - 1] - delta, (lp, l64[T - 1], delta)
    assert lp <= l64[-1] + 1e-6, (lp, l64[-1])
    # the reported lp is the returned mixture's
    tr = em.trace()
    assert tr.size == T
    assert abs(tr[-1] - lp) <= 1e-6 * abs(lp), (tr[-1], lp)
    assert abs(tr[0] - l64[0]) <= 1e-6 * abs(l64[0])  # entry 0: the first iterate's
    assert info["last_lp"] == tr[-1]


# ---- 4. monotone -----------------------------------------------------------------------------------------------------------------
def test_first_hundred_increments_are_positive(P, ctx, lm_fixture):
    em = _em(P, ctx, lm_fixture)
    info = em.run(100, -1.0)
    inc = np.diff(np.concatenate([[info["lp_start"]], em.trace()]))
    assert inc.size == 100 and (inc > 0).all(), inc.min()  # (the restatement's smallest is 0.026; f32 noise is 1e-4)


# ---- 5. stop rule ----------------------------------------------------------------------------------------------------------------
def test_stop_rule(P, ctx, lm_fixture, prob):
    t_ref, y_ref = reference_stop_iteration(prob)
    em = _em(P, ctx, lm_fixture)
    info = em.run()  # tol 1e-6, max_iters 5000
    lp = prob.lp64(_norm64(em.mixture()))
    print("stopped after %d iterations at lp64 %.6f (last increase %.3g); em.jl's own rule stops the f32 restatement at %d, lp64 %.6f"
          % (info["iters"], lp, info["last_increase"], t_ref, prob.lp64(y_ref)))
    assert info["converged"] and info["iters"] < 5000
    assert info["last_increase"] < 1e-6
    assert info["iters"] >= t_ref
    assert lp >= prob.lp64(y_ref)
    assert em.trace().size == info["iters"]
    y = em.mixture()
    for _ in range(2):
        again = em.run(50, 1e-6, 7)
        assert again["iters"] == info["iters"] and again["converged"]
        assert np.array_equal(em.mixture().view(np.uint32), y.view(np.uint32))


# ---- 6. multiplicities -----------------------------------------------------------------------------------------------------------
def test_multiplicities_match_the_row_expanded_matrix(P, ctx, lm_fixture):
    rng = np.random.default_rng(7)
    ks = rng.integers(1, 5, lm_fixture["m"]).astype(np.int64)
    Px = expand_rows(lm_fixture, ks)
    T = 200
    _, l64 = run_em(Px, T)
    _, l32 = run_em(Px, T, np.float32)
    em = _em(P, ctx, lm_fixture, ks=ks)
    info = em.run(T, -1.0)
    assert info["M"] == int(ks.sum())
    lp = Px.lp64(_norm64(em.mixture()))
    y3000, _ = run_em(Px, 3000, trace=False)
    assert lp >= l64[-1] - _delta(l64, l32, T), (lp, l64[-1])
    assert lp <= Px.lp64(y3000) + 1e-6
    assert abs(em.trace()[-1] - lp) <= 1e-6 * abs(lp)
    got, want = em.info(kkt=True)["kkt_max"], _residual64(Px, em.mixture())
    assert abs(got - want) <= 1e-3 * want, (got, want)  # (the f64 gradient with multiplicities)


def test_multiplicities_with_the_host_built_layout(P, ctx, lm_fixture, tmp_path):
    """M and one iteration with the layout built by the host builder (POLEE_DEVICE_BUILD=0, read once per process: a child)."""
    import subprocess
    import sys
    rng = np.random.default_rng(7)
    ks = rng.integers(1, 5, lm_fixture["m"]).astype(np.int64)
    np.save(str(tmp_path / "ks.npy"), ks)
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import polee_amd as P; from polee_amd.em import EM\n"
            "a = np.load(%r); ks = np.load(%r)\n"
            "s = P.RNASeqSample(int(a['m'][0]), int(a['n'][0]), a['colptr'], a['rowval'], a['nzval'], a['effective_lengths'], ks=ks)\n"
            "assert not s.built_on_device\n"
            "em = EM(s); info = em.run(1, -1.0); np.save(%r, em.mixture()); print('M', info['M'])\n"
            % (ROOT, os.path.join(GOLDEN, "mBr_M_6w_1.likelihood-matrix.npz"), str(tmp_path / "ks.npy"), str(tmp_path / "y.npy")))
    out = subprocess.check_output([sys.executable, "-c", code], env=dict(os.environ, POLEE_DEVICE_BUILD="0"), cwd=ROOT, timeout=300)
    assert out.decode().split()[-2:] == ["M", str(int(ks.sum()))]
    want, _ = run_em(Problem.from_csc(lm_fixture, ks=ks), 1, trace=False)
    np.testing.assert_allclose(np.load(str(tmp_path / "y.npy")), want, rtol=1e-4, atol=0)


# ---- 7. empty rows and columns ---------------------------------------------------------------------------------------------------
def test_empty_rows_and_columns(P, ctx, lm_fixture):
    lm = lm_fixture
    rng = np.random.default_rng(3)
    rows = rng.choice(lm["m"], 500, replace=False)
    collen = np.diff(np.asarray(lm["colptr"], np.int64))
    cols = rng.choice(np.flatnonzero(collen > 0), 5, replace=False)
    colidx = np.repeat(np.arange(lm["n"]), collen)
    keep = ~np.isin(np.asarray(lm["rowval"], np.int64) - 1, rows) & ~np.isin(colidx, cols)
    sub = subset_csc(lm, keep)
    Ps = Problem.from_csc(sub)
    assert Ps.keep.size <= lm["m"] - 500
    s = _sample(P, ctx, sub)
    from polee_amd.em import EM
    em = EM(s)
    info = em.run(1, -1.0)
    assert s.info["num_empty_rows"] == lm["m"] - Ps.keep.size
    assert info["M"] == lm["m"] - s.info["num_empty_rows"]
    y1 = em.mixture()
    empty_cols = np.flatnonzero(np.bincount(Ps.col, minlength=lm["n"]) == 0)
    assert np.isin(cols, empty_cols).all() and (y1[empty_cols] == 0).all()
    np.testing.assert_allclose(y1, run_em(Ps, 1, trace=False)[0], rtol=1e-4, atol=0)
    info = em.run(1999, -1.0)
    y = em.mixture()
    assert info["iters"] == 2000 and not info["nonfinite"]
    assert np.isfinite(y).all() and (y >= 0).all() and (y[empty_cols] == 0).all()
    assert abs(float(y.astype(np.float64).sum()) - 1) <= 1e-6
    assert np.isfinite(em.trace()).all()


def test_zeros_and_subnormals_on_the_fixture(P, ctx, lm_fixture):
    """Transcripts without fragments are 0 after one iteration; more underflow on the way; nothing turns NaN or Inf."""
    em = _em(P, ctx, lm_fixture)
    em.run(2000, -1.0)
    y = em.mixture()
    assert np.isfinite(y).all() and (y >= 0).all()
    assert (y == 0).sum() >= 29 and np.isfinite(em.trace()).all()


# ---- 8. TPM ----------------------------------------------------------------------------------------------------------------------
def test_tpm(P, ctx, lm_fixture):
    em = _em(P, ctx, lm_fixture)
    em.run(50, -1.0)
    y = em.mixture().astype(np.float64)
    el = lm_fixture["effective_lengths"].astype(np.float64)
    tpm = em.tpm()
    want = 1e6 * (y / el) / (y / el).sum()
    np.testing.assert_allclose(tpm, want, rtol=1e-6, atol=0)
    assert abs(float(tpm.astype(np.float64).sum()) - 1e6) <= 1
    raw = em.tpm(use_efflen=False)
    np.testing.assert_allclose(raw, 1e6 * y, rtol=1e-6, atol=0)
    assert abs(float(raw.astype(np.float64).sum()) - 1e6) <= 1


# ---- 9. fixed point --------------------------------------------------------------------------------------------------------------
def _residual64(prob, y):
    yn = _norm64(y)
    return float(np.max(yn * np.abs(prob.gradient(yn) / prob.M - 1)))


def test_fixed_point_loses_nothing(P, ctx, lm_fixture, prob, runs):
    y64, l64, l32 = runs
    em = _em(P, ctx, lm_fixture, y0=y64.astype(np.float32))
    em.run(20, -1.0)
    y = em.mixture()
    lp = prob.lp64(_norm64(y))
    print("20 iterations from the f64 optimum: lp64 %.3g below it" % (l64[-1] - lp))
    assert lp >= l64[-1] - _delta(l64, l32, 1000)
    info = em.info(kkt=True)
    assert 0 <= info["kkt_max"] < 1e-6
    assert np.array_equal(em.mixture().view(np.uint32), y.view(np.uint32))  # (the extra pass leaves the iterate alone)
    assert em.run(1, -1.0)["iters"] == 21                                    # ... and the next pass finds g zeroed
    assert prob.lp64(_norm64(em.mixture())) >= l64[-1] - _delta(l64, l32, 1000)


@pytest.mark.parametrize("T", [1, 5, 50])
def test_residual_of_early_iterates(P, ctx, lm_fixture, prob, T):
    """Far from the fixed point the residual is large against the rounding of an f32 gradient (below)."""
    em = _em(P, ctx, lm_fixture)
    em.run(T, -1.0)
    got, want = em.info(kkt=True)["kkt_max"], _residual64(prob, em.mixture())
    print("T = %d: kkt_max device %.6g, NumPy %.6g" % (T, got, want))
    assert abs(got - want) <= 1e-3 * want, (got, want)


def test_residual_at_the_optimum(P, ctx, lm_fixture, prob, runs):
    """info.kkt_max against max_j y_j |g_j / M - 1| recomputed in f64 NumPy at the returned mixture, rtol 1e-3, after 20
    iterations from the f32 cast of the f64 optimum.  There |g_j / M - 1| is about 5e-8 on the transcript that attains the maximum
    (y_j = 0.005), one ulp of an f32: the residual of the f32 gradient the iterations use read 9.2e-9 where f64 gives 5.1e-9, so
    the residual is computed from an f64 gradient of its own (em.hip, em_g64_tiles_kernel), at the mixture handed out."""
    y64, _, _ = runs
    em = _em(P, ctx, lm_fixture, y0=y64.astype(np.float32))
    em.run(20, -1.0)
    got, want = em.info(kkt=True)["kkt_max"], _residual64(prob, em.mixture())
    print("kkt_max: device %.6g, NumPy on the returned mixture %.6g" % (got, want))
    assert abs(got - want) <= 1e-3 * want, (got, want)


# ---- 10. reproducible ------------------------------------------------------------------------------------------------------------
def test_bitwise_reproducible_in_deterministic_mode(P, ctx, lm_fixture):
    out = []
    for check_every in (64, 64, 1):
        em = _em(P, ctx, lm_fixture, deterministic=True)
        em.run(200, -1.0, check_every)
        out.append((em.mixture(), em.trace()))
    for y, tr in out[1:]:
        assert np.array_equal(y.view(np.uint32), out[0][0].view(np.uint32))
        assert np.array_equal(tr.view(np.uint64), out[0][1].view(np.uint64))
    # in two calls, and after a reset, the same again
    em = _em(P, ctx, lm_fixture, deterministic=True)
    em.run(120, -1.0)
    em.run(80, -1.0)
    assert np.array_equal(em.mixture().view(np.uint32), out[0][0].view(np.uint32))
    assert np.array_equal(em.trace().view(np.uint64), out[0][1].view(np.uint64))
    em.reset()
    assert em.info()["iters"] == 0 and em.trace().size == 0
    em.run(200, -1.0, 13)
    assert np.array_equal(em.mixture().view(np.uint32), out[0][0].view(np.uint32))


# ---- 11. C2 size -----------------------------------------------------------------------------------------------------------------
def test_c2_full_size(P, ctx):
    from oracle import oracle as O
    from tools import synth
    from polee_amd.em import EM
    N, M = 200_000, 30_000_000
    smp = synth.make_sample(N, M, 8.0, seed=123456789, literal=True)
    s = P.RNASeqSample(M, N, None, None, None, smp["effective_lengths"], ctx=ctx, xt=(smp["tcolptr"], smp["trowval"], smp["tnzval"]))
    em = EM(s)
    info = em.run(30, -1.0)
    Mfr = M - s.info["num_empty_rows"]
    assert info["M"] == Mfr and info["iters"] == 30
    y = em.mixture()
    assert np.isfinite(y).all() and (y >= 0).all()
    assert abs(float(y.astype(np.float64).sum()) - 1) <= 1e-5
    tr = em.trace()
    inc = np.diff(np.concatenate([[info["lp_start"]], tr]))
    print("C2 increments: first five %s, smallest %.6g, |lp| %.6g" % (np.array2string(inc[:5], precision=4), inc.min(), abs(tr[-1])))
    assert tr.size == 30 and (inc[:5] > 0).all()
    assert (inc >= -1e-6 * abs(tr[-1])).all(), inc.min()
    colptr, rowval, nzval = synth.to_csc(smp)
    so = O.Sample(M, N, colptr, rowval, nzval)
    del colptr, rowval, nzval
    O.set_num_threads(O.physical_cores())
    lpo, go = so.log_likelihood(y)
    print("C2: reported lp - f64 oracle at the returned mixture = %.4g (%.3g of |lp|)" % (tr[-1] - lpo, abs(tr[-1] - lpo) / abs(lpo)))
    assert abs(tr[-1] - lpo) <= 1e-6 * abs(lpo), (tr[-1], lpo)
    # the f64 gradient behind the residual, over every stream of a C2-size layout (the oracle multiplies in f32 and sums in f64)
    yn = y.astype(np.float64) / y.astype(np.float64).sum()
    got, want = em.info(kkt=True)["kkt_max"], float(np.max(yn * np.abs(go * y.astype(np.float64).sum() / Mfr - 1)))
    print("C2: kkt_max device %.6g, from the oracle's gradient %.6g" % (got, want))
    assert abs(got - want) <= 1e-3 * want, (got, want)
    em.run(1, -1.0)
    y1 = em.mixture()
    sel = y > 1e-9
    np.testing.assert_allclose(y1[sel], (y.astype(np.float64) * go / Mfr)[sel], rtol=1e-4, atol=0)


def test_start_with_zeros_at_scale(P, ctx):
    """The count behind the check of a start with zeros (two passes, lp(2y) - lp(y) = ln 2 x fragments counted) at 1.26e7
    fragments: a mixture with 18 531 exact zeros is accepted, one that leaves fragments without a transcript is not."""
    from tools import synth
    from polee_amd import PoleeError
    from polee_amd.em import EM
    smp = synth.tile_fixture(639)
    s = P.RNASeqSample(smp["m"], smp["n"], None, None, None, smp["effective_lengths"], ctx=ctx,
                       xt=(smp["tcolptr"], smp["trowval"], smp["tnzval"]))
    em = EM(s)
    info = em.run(5, -1.0)
    y = em.mixture()
    assert (y == 0).sum() >= 29 * 639
    em.reset(y)
    again = em.run(1, -1.0)
    assert abs(again["lp_start"] - info["last_lp"]) <= 1e-8 * abs(info["last_lp"])
    # the first fragment with several transcripts loses all of them
    tp = np.asarray(smp["tcolptr"], np.int64) - 1
    i = int(np.flatnonzero(np.diff(tp) >= 2)[0])
    cols = np.asarray(smp["trowval"][tp[i]:tp[i + 1]], np.int64) - 1
    y0 = np.where(y > 0, y, np.float32(1e-9)).astype(np.float32)
    y0[cols] = 0
    with pytest.raises(PoleeError, match="probability 0|only one") as e:
        em.reset(y0)
    assert e.value.status == 1


# ---- 12. rejections --------------------------------------------------------------------------------------------------------------
def test_argument_rejection(P, ctx, lm_fixture, prob):
    from polee_amd import PoleeError, _lib as L
    from polee_amd.em import EM
    lm, n = lm_fixture, lm_fixture["n"]
    lib = L.lib()
    h = C.c_void_p()
    assert lib.polee_em_create(None, None, C.byref(h)) == 1 and not h
    assert b"polee_em_create: null handle" in lib.polee_last_error(None)
    s = _sample(P, ctx, lm)
    good = np.full(n, 1.0, np.float32)
    for name, j, v in (("negative", 3, -1.0), ("NaN", 4, np.nan), ("infinite", 5, np.inf)):
        y0 = good.copy()
        y0[j] = v
        with pytest.raises(PoleeError, match=r"y0\[%d\]" % j) as e:
            EM(s, y0)
        assert e.value.status == 1, name
    with pytest.raises(PoleeError, match="sums to 0") as e:
        EM(s, np.zeros(n, np.float32))
    assert e.value.status == 1
    # 0 on the only transcript some fragment is compatible with: that fragment's probability would be 0
    lens = np.bincount(prob.row)
    j = int(prob.col[prob.starts[np.flatnonzero(lens == 1)[0]]])
    y0 = good.copy()
    y0[j] = 0
    with pytest.raises(PoleeError, match="only one") as e:
        EM(s, y0)
    assert e.value.status == 1
    em = EM(s)
    with pytest.raises(PoleeError, match="only one") as e:
        em.reset(y0)
    assert e.value.status == 1
    # ... and on every transcript of a fragment with several (none of them the case above): counted by two passes
    single = np.bincount(prob.col[prob.starts[lens == 1]], minlength=n) > 0
    i = next(int(r) for r in np.flatnonzero(lens >= 2) if not single[prob.col[prob.starts[r]:prob.starts[r] + lens[r]]].any())
    dead_cols = prob.col[prob.starts[i]:prob.starts[i] + lens[i]]
    y0 = good.copy()
    y0[dead_cols] = 0
    _, p = prob.frag_probs(y0)
    with pytest.raises(PoleeError, match="%d of the 19743 fragments have probability 0" % int((p == 0).sum())) as e:
        EM(s, y0)
    assert e.value.status == 1
    with pytest.raises(PoleeError, match="fragments have probability 0"):
        em.reset(y0)  # (a refused start leaves the handle as it was: the three iterations below start from 1 / n)
    # zeros that leave every fragment a transcript are a start like any other (and stay 0)
    y0 = good.copy()
    y0[dead_cols[0]] = 0
    y0[np.bincount(prob.col, minlength=n) == 0] = 0
    em3 = EM(s, y0)
    info = em3.run(30, -1.0)
    assert info["iters"] == 30 and not info["nonfinite"] and em3.mixture()[dead_cols[0]] == 0
    yr, lr = run_em(prob, 30, y0=y0)
    assert abs(info["last_lp"] - lr[-1]) <= 1e-6 * abs(lr[-1])
    with pytest.raises(PoleeError, match="max_iters < 0") as e:
        em.run(-1, 1e-6, 8)
    assert e.value.status == 1
    with pytest.raises(PoleeError, match="check_every < 1") as e:
        em.run(10, 1e-6, 0)
    assert e.value.status == 1
    k = C.c_int64()
    buf = np.zeros(4, np.float64)
    assert lib.polee_em_get_trace(em._h, L.ptr(buf, L.f64p), C.c_int64(-1), C.byref(k)) == 1
    assert b"capacity" in lib.polee_last_error(ctx._h)
    em.run(3, -1.0)
    assert lib.polee_em_get_trace(em._h, L.ptr(buf, L.f64p), C.c_int64(2), C.byref(k)) == 0
    assert k.value == 3 and buf[1] != 0 and buf[2] == 0
    assert abs(em.info()["lp_start"] - -364724.375) <= 1e-6 * 364724.375


# ---- 13. CLI ---------------------------------------------------------------------------------------------------------------------
def test_cli_writes_tpm_csv_and_trace(P, tmp_path):
    import subprocess
    import sys
    out, tr = str(tmp_path / "em.csv"), str(tmp_path / "trace.csv")
    lm = os.path.join(GOLDEN, "mBr_M_6w_1.likelihood-matrix.h5")
    subprocess.check_call([sys.executable, "-m", "polee_amd.em", lm, "-o", out, "--trace", tr, "--max-iters", "150", "--tol", "-1",
                           "--deterministic"], cwd=ROOT, timeout=300)
    lines = open(out).read().splitlines()
    assert lines[0] == "transcript_id,tpm" and len(lines) == 314
    ids = [ln.split(",")[0] for ln in lines[1:]]
    tpm = np.array([float(ln.split(",")[1]) for ln in lines[1:]])
    assert ids == [str(j) for j in range(1, 314)]
    assert abs(tpm.sum() - 1e6) <= 1 and (tpm >= 0).all()
    tlines = open(tr).read().splitlines()
    assert tlines[0] == "iteration,lp" and len(tlines) == 151
    assert -326995.495 < float(tlines[-1].split(",")[1]) < -326994.548  # (the restatement's lp at 100 and at 200 iterations)

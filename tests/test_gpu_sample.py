"""`polee sample` on the GPU (csrc/sample.hip, csrc/binomial.hpp, polee_amd.sample): the streaming handle against
polee_sampler_draw (bit for bit), against the NumPy restatement of tests/test_sample_host.py and against the oracle's draws; the
exact multinomial sampler against scipy's binomial pmf and the multinomial's moments; the command end to end.

The statistical tests use fixed seeds, so their outcome does not vary from run to run; their limits are set so that a correct
sampler fails with probability below 1e-8."""
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import stats

from conftest import ROOT
from oracle import oracle as O
from test_sample_host import (FIXTURE_M, PREP_H5, check_multinomial, heavy_tailed_shares, pooled_chi2, restate_expected_counts,
                              restate_posterior_mean, restate_props)

pytestmark = pytest.mark.gpu

SEED = 20260117
RT22 = 2.0 ** -22


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def ctx(P):
    return P.Context(0)


def _params(prep):
    return prep["mu"], np.exp(prep["omega"]), prep["alpha"], prep["effective_lengths"]


def _stream(P, ctx, prep, seed=SEED, m=FIXTURE_M):
    from polee_amd.sample import ApproxSampleStream
    t = P.PolyaTreeTransform(prep["node_parent_idxs"], prep["node_js"], ctx=ctx)
    mu, sigma, alpha, l = _params(prep)
    return ApproxSampleStream(t, mu, sigma, alpha, l, m, seed)


def _plain_draws(P, ctx, prep, ndraws, seed=SEED, z0=None):
    """polee_sampler_draw, what the parent commit offers"""
    t = P.PolyaTreeTransform(prep["node_parent_idxs"], prep["node_js"], ctx=ctx)
    mu, sigma, alpha, _ = _params(prep)
    als = P.ApproxLikelihoodSampler()
    als.set_transform(t, mu, sigma, alpha)
    als.seed(seed)
    return als.rand(ndraws, z0=z0)


def _run_split(P, ctx, prep, sizes, z0=None):
    """All outputs of a stream whose draws are asked for in calls of the given sizes: expected counts from one stream, sampled
    counts from a second one with the same seed."""
    a, b = _stream(P, ctx, prep), _stream(P, ctx, prep)
    raw, props, ce, cs = [], [], [], []
    k = 0
    for c in sizes:
        z = None if z0 is None else z0[k:k + c]
        o = a.next(c, props=True, counts=True, raw=True, z0=z)
        raw.append(o["raw"]); props.append(o["props"]); ce.append(o["counts"])
        cs.append(b.next(c, props=False, counts=True, sample_counts=True, z0=z)["counts"])
        k += c
    assert a.num_draws == k and b.num_draws == k
    pm, ec = a.mean()
    pm2, ecs = b.mean(sample_counts=True)
    np.testing.assert_array_equal(pm, pm2)
    return dict(raw=np.concatenate(raw), props=np.concatenate(props), expected=np.concatenate(ce), sampled=np.concatenate(cs), pm=pm,
                ec=ec, ecs=ecs)


@pytest.mark.parametrize("noise", ["device", "supplied"])
def test_draw_identity_and_independence_of_the_split(P, ctx, prep_fixture, noise):
    n, N = 313, 64
    z0 = O.randn(N * (n - 1), 41).reshape(N, n - 1).astype(np.float32) if noise == "supplied" else None
    plain = _plain_draws(P, ctx, prep_fixture, N, z0=z0)
    whole = _run_split(P, ctx, prep_fixture, [N], z0)
    assert whole["raw"].tobytes() == plain.tobytes()  # draw d of the handle is row d of polee_sampler_draw, bit for bit
    if noise == "device":  # ... and of a longer polee_sampler_draw: a draw depends on (seed, d) alone
        assert _plain_draws(P, ctx, prep_fixture, N + 13)[:N].tobytes() == plain.tobytes()
    for sizes in ([16] * 4, [1] * N, [5, 11, 3, 45]):
        part = _run_split(P, ctx, prep_fixture, sizes, z0)
        for key in whole:
            assert part[key].tobytes() == whole[key].tobytes(), (sizes, key)


def test_props_counts_and_mean_match_the_restatement_and_the_oracle(P, ctx, prep_fixture):
    n, N, m = 313, 40, FIXTURE_M
    mu, sigma, alpha, l = _params(prep_fixture)
    z0 = O.randn(N * (n - 1), 43).reshape(N, n - 1).astype(np.float32)
    got = _run_split(P, ctx, prep_fixture, [N], z0)
    props = restate_props(got["raw"], l)
    # the only freedom: the order of the f64 sum and one f32 rounding
    np.testing.assert_allclose(got["props"], props, rtol=RT22, atol=0)
    # counts and the mean from the DEVICE's props: their own arithmetic is f64 (or one f32 rounding of an f64 mean)
    np.testing.assert_allclose(got["expected"], restate_expected_counts(got["props"], l, m), rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["pm"], restate_posterior_mean(got["props"]), rtol=RT22, atol=0)
    np.testing.assert_allclose(got["pm"], restate_posterior_mean(props), rtol=RT22, atol=0)
    np.testing.assert_allclose(got["ec"], restate_expected_counts(got["pm"], l, m), rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["expected"].sum(axis=1), m, rtol=1e-12)
    # against the oracle's draws from the same noise: twice the sampler's own tolerance (a prop divides by a sum with the same error)
    to = O.PTT(prep_fixture["node_parent_idxs"], prep_fixture["node_js"])
    oracle_raw = np.stack([O.sampler_draw(to, mu, sigma, alpha, z0[d]) for d in range(N)])
    np.testing.assert_allclose(got["props"], restate_props(oracle_raw, l), rtol=4e-5, atol=1e-30)


def test_sampled_counts_structure(P, ctx, prep_fixture):
    from polee_amd.sample import multinomial_counts
    m = FIXTURE_M
    got = _run_split(P, ctx, prep_fixture, [24])
    for c in (got["sampled"], got["ecs"][None, :]):
        assert c.dtype == np.float64 and (c == np.floor(c)).all() and (c >= 0).all()
        assert (c.sum(axis=1) == m).all()
    assert len({r.tobytes() for r in got["sampled"]}) == 24  # different across draws
    other = _stream(P, ctx, prep_fixture, seed=SEED + 1).next(8, props=False, counts=True, sample_counts=True)["counts"]
    assert (other.sum(axis=1) == m).all() and not (other == got["sampled"][:8]).all()
    assert _stream(P, ctx, prep_fixture, m=0).next(3, props=False, counts=True, sample_counts=True)["counts"].max() == 0
    # the public sampler: zeros where the share is 0, rows are functions of (shares, m, seed, draw index)
    rng = np.random.default_rng(2)
    p = rng.gamma(0.3, size=(9, 1000))
    p[:, rng.random(1000) < 0.3] = 0.0
    p[3, :500] = 0.0
    c = multinomial_counts(p, 123457, seed=5, ctx=ctx)
    assert c.dtype == np.uint32 and c.shape == p.shape
    assert (c.sum(axis=1, dtype=np.int64) == 123457).all() and (c[p == 0] == 0).all()
    np.testing.assert_array_equal(c, multinomial_counts(p, 123457, seed=5, ctx=ctx))
    np.testing.assert_array_equal(c[3:6], multinomial_counts(p[3:6], 123457, seed=5, first_draw=3, ctx=ctx))
    np.testing.assert_array_equal(c[7], multinomial_counts(p[7], 123457, seed=5, first_draw=7, ctx=ctx))
    assert not (multinomial_counts(p, 123457, seed=6, ctx=ctx) == c).all()
    same = np.repeat(p[:1], 4, axis=0)
    cs = multinomial_counts(same, 123457, seed=5, ctx=ctx)
    assert len({r.tobytes() for r in cs}) == 4  # the same shares under four draw indexes
    assert multinomial_counts(p, 0, seed=5, ctx=ctx).max() == 0
    assert multinomial_counts(np.array([[2.5]]), 77, ctx=ctx).tolist() == [[77]]
    assert multinomial_counts(np.array([0.0, 3.0, 0.0]), 2 ** 31 - 1, ctx=ctx).tolist() == [0, 2 ** 31 - 1, 0]


BINOMIAL_CASES = [(5, .5), (40, .2), (1000, .004), (1000, .3), (1000, .97), (30_000_000, 1e-7), (30_000_000, .37), (2 ** 31 - 1, .5),
                  (2 ** 31 - 1, 1e-9)]


@pytest.mark.parametrize("N,p", BINOMIAL_CASES)
def test_binomial_goodness_of_fit(ctx, N, p):
    from polee_amd.sample import debug_binomial
    cnt = 1 << 20
    x = debug_binomial(np.full(cnt, N, np.int64), np.full(cnt, p), seed=SEED + BINOMIAL_CASES.index((N, p)), ctx=ctx)
    assert x.min() >= 0 and x.max() <= N
    sd = np.sqrt(N * p * (1 - p))
    lo, hi = max(0, int(N * p - 12 * sd - 30)), min(N, int(N * p + 12 * sd + 30))
    assert x.min() >= lo and x.max() <= hi  # (12 standard deviations: beyond it lies less than 1e-30)
    ks = np.arange(lo, hi + 1)
    expect = stats.binom.pmf(ks, N, p) * cnt
    obs = np.bincount(x - lo, minlength=ks.size).astype(np.float64)
    eb, ob, ae, ao = [], [], 0.0, 0.0
    for e, o in zip(expect.tolist(), obs.tolist()):  # pooled from the left to an expected count >= 10; the rest joins the last bin
        ae += e
        ao += o
        if ae >= 10.0:
            eb.append(ae); ob.append(ao)
            ae = ao = 0.0
    eb[-1] += ae + (cnt - expect.sum())
    ob[-1] += ao
    eb, ob = np.array(eb), np.array(ob)
    chi, df = float(((ob - eb) ** 2 / eb).sum()), len(eb) - 1
    limit = float(stats.chi2.isf(1e-9 / len(BINOMIAL_CASES), df))
    z = (x.mean() - N * p) / (sd / np.sqrt(cnt))
    print("Binomial(%d, %g): chi2 %.1f, df %d, limit %.1f; mean off by %.2f standard errors" % (N, p, chi, df, limit, z))
    assert df >= 4 and chi < limit, (chi, df, limit)
    assert abs(z) < 7.0, z


def test_binomial_closed_forms(ctx):
    from polee_amd.sample import debug_binomial
    N = np.array([0, 0, 0, 17, 17, 2 ** 31 - 1, 2 ** 31 - 1, 1, 1], np.int64)
    p = np.array([0.0, 0.3, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0])
    assert debug_binomial(N, p, ctx=ctx).tolist() == [0, 0, 0, 0, 17, 0, 2 ** 31 - 1, 0, 1]
    one = debug_binomial(np.ones(100000, np.int64), np.full(100000, 0.25), ctx=ctx)
    assert set(one.tolist()) == {0, 1} and abs(one.mean() - 0.25) < 7 * np.sqrt(0.1875 / 100000)


@pytest.mark.parametrize("m,min_categories", [(FIXTURE_M, 10), (30_000_000, 150)])
def test_multinomial_goodness_of_fit(ctx, m, min_categories):
    from polee_amd.sample import multinomial_counts
    p, D = heavy_tailed_shares(), 1024
    c = multinomial_counts(np.repeat(p[None, :], D, axis=0), m, seed=SEED, ctx=ctx).astype(np.int64)
    check_multinomial(c, p, m, min_categories)


def test_multinomial_at_full_size(ctx):
    from polee_amd.sample import multinomial_counts
    n, m, D = 200_000, 30_000_000, 8
    p = np.random.default_rng(7).lognormal(0.0, 3.0, n)
    p[::97] = 0.0
    rows = np.repeat(p[None, :], D, axis=0)
    c = multinomial_counts(rows, m, seed=SEED, ctx=ctx)
    assert (c.sum(axis=1, dtype=np.int64) == m).all() and (c[:, ::97] == 0).all()
    chi, df, limit = pooled_chi2(c.astype(np.int64), p, m)
    print("n = 200 000, m = 30 M, D = 8: pooled chi2 %.1f, df %d, limit %.1f" % (chi, df, limit))
    assert df > 50_000 and chi < limit, (chi, df, limit)
    np.testing.assert_array_equal(c, multinomial_counts(rows, m, seed=SEED, ctx=ctx))
    np.testing.assert_array_equal(c[5], multinomial_counts(p, m, seed=SEED, first_draw=5, ctx=ctx))


def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "polee_amd.sample"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def _read_kallisto(fn, n, N):
    from polee_amd import h5io
    with h5io.File(fn) as f:
        assert f.dataset_kind("est_counts") == ("float", 8, (n,))
        assert f.dataset_kind("aux/eff_lengths") == ("float", 8, (n,)) and f.dataset_kind("aux/lengths") == ("integer", 8, (n,))
        assert f.dataset_kind("aux/ids")[0] == "string" and f.dataset_kind("aux/ids")[2] == (n,)
        assert f.dataset_kind("aux/call")[0] == "string" and f.dataset_kind("aux/start_time")[0] == "string"
        assert f.read("aux/num_bootstrap", np.int64).tolist() == [N] and f.read("aux/index_version", np.int64).tolist() == [-1]
        assert f.read_strings("aux/kallisto_version") == "polee sample"
        assert not f.exists("bootstrap/bs%d" % N)
        return dict(est=f.read("est_counts", np.float64), ids=f.read_strings("aux/ids"), lens=f.read("aux/lengths", np.int64),
                    eff=f.read("aux/eff_lengths", np.float64),
                    bs=np.stack([f.read("bootstrap/bs%d" % k, np.float64) for k in range(N)]))


def test_command_end_to_end(P, ctx, prep_fixture, tmp_path):
    from polee_amd import h5io
    n, N, m = 313, 24, FIXTURE_M
    l = prep_fixture["effective_lengths"]
    d = str(tmp_path)
    base = [PREP_H5, "--num-samples", str(N), "--batch", "7"]
    # the same draws through polee_sampler_draw (the command's default seed), restated
    from polee_amd.sample import DEFAULT_SEED
    props = restate_props(_plain_draws(P, ctx, prep_fixture, N, seed=DEFAULT_SEED), l)
    pm = restate_posterior_mean(props)
    # a transformation file holding the fixture's own tree, and the default ids
    tf = os.path.join(d, "tree.h5")
    with h5io.File(tf, "w") as f:
        f.write("node_parent_idxs", prep_fixture["node_parent_idxs"])
        f.write("node_js", prep_fixture["node_js"])
        f.write_strings("transcript_ids", [str(j) for j in range(1, n + 1)])

    _cli(base + ["--kallisto", "-o", os.path.join(d, "e.h5")], d)
    e = _read_kallisto(os.path.join(d, "e.h5"), n, N)
    assert e["ids"] == [str(j) for j in range(1, n + 1)] and (e["lens"] == -1).all()
    np.testing.assert_array_equal(e["eff"], l.astype(np.float64))
    np.testing.assert_allclose(e["est"].sum(), m, rtol=1e-9)
    np.testing.assert_allclose(e["bs"].sum(axis=1), m, rtol=1e-9)
    # (counts = e / sum(e) * m: e and sum(e) each carry at most the 2^-22 of the props they come from, the rest is f64)
    np.testing.assert_allclose(e["bs"], restate_expected_counts(props, l, m), rtol=2.5 * RT22)
    np.testing.assert_allclose(e["est"], restate_expected_counts(pm, l, m), rtol=2.5 * RT22)

    _cli(base + ["--kallisto", "--sample-counts", "-o", os.path.join(d, "s.h5")], d)
    s = _read_kallisto(os.path.join(d, "s.h5"), n, N)
    assert s["est"].sum() == m and (s["bs"].sum(axis=1) == m).all() and (s["bs"] == np.floor(s["bs"])).all()
    # sampled counts scatter around the expected ones like a multinomial: sum over draws of the Pearson statistic
    big = e["bs"] >= 10.0
    pearson = ((s["bs"] - e["bs"]) ** 2 / e["bs"])[big].sum()
    assert pearson < stats.chi2.isf(1e-9, int(big.sum())), (pearson, big.sum())

    _cli(base + ["-o", os.path.join(d, "e.csv")], d)
    _cli(base + ["--sample-counts", "-o", os.path.join(d, "s.csv")], d)
    lines = open(os.path.join(d, "e.csv")).read().split("\n")
    assert lines[0] == "transcript_id,tpm" and len(lines) == n + 2 and lines[-1] == ""
    assert [ln.split(",")[0] for ln in lines[1:-1]] == [str(j) for j in range(1, n + 1)]
    tpm = np.array([float(ln.split(",")[1]) for ln in lines[1:-1]])
    np.testing.assert_allclose(tpm, 1e6 * pm.astype(np.float64), rtol=RT22, atol=0)
    assert open(os.path.join(d, "s.csv")).read() == open(os.path.join(d, "e.csv")).read()  # the TPMs do not depend on the counts' mode

    # --transformation with the same tree: the same contents; default output names in the working directory
    _cli(base + ["--kallisto", "--transformation", tf], d)
    t = _read_kallisto(os.path.join(d, "polee-sample.h5"), n, N)
    for key in ("est", "bs", "eff", "lens"):
        np.testing.assert_array_equal(t[key], e[key])
    assert t["ids"] == e["ids"]
    _cli(base + ["--transformation", tf, "--trim-prefix", "3"], d)
    lines_t = open(os.path.join(d, "polee-sample.csv")).read().split("\n")
    assert [ln.split(",")[1] for ln in lines_t[1:-1]] == [ln.split(",")[1] for ln in lines[1:-1]]
    assert [ln.split(",")[0] for ln in lines_t[1:-1]] == [str(j).replace("3", "") for j in range(1, n + 1)]


def test_memory_returns_and_bad_arguments(P, prep_fixture):
    from polee_amd import _lib as L
    from polee_amd.sample import ApproxSampleStream, debug_binomial, multinomial_counts
    probe = P.Context(0)

    def free_bytes():
        gc.collect()
        probe.synchronize()
        return probe.mem_info()[0]

    def cycle():
        c = P.Context(0)
        s = _stream(P, c, prep_fixture)
        s.next(20, props=True, counts=True, sample_counts=True, raw=True)
        s.next(3, props=True, counts=True)
        s.mean(sample_counts=True)
        multinomial_counts(np.ones((5, 4000)), 1000, ctx=c)
        del c, s

    cycle()
    cycle()
    base = free_bytes()
    for _ in range(5):
        cycle()
    assert base - free_bytes() < 8 << 20, (base, free_bytes())

    ctx = probe
    mu, sigma, alpha, l = _params(prep_fixture)
    t = P.PolyaTreeTransform(prep_fixture["node_parent_idxs"], prep_fixture["node_js"], ctx=ctx)

    def bad(f, *a, **kw):
        with pytest.raises(P.PoleeError) as e:
            f(*a, **kw)
        assert e.value.status == 1 and len(str(e.value)) > 30, str(e.value)  # POLEE_ERR_BAD_ARG with a message

    for m in (-1, 2 ** 31, 2 ** 40):
        bad(ApproxSampleStream, t, mu, sigma, alpha, l, m)
        bad(multinomial_counts, np.ones((2, 5)), m, ctx=ctx)
    for v in (0.0, -1.0, np.inf, np.nan):
        l2 = l.copy(); l2[7] = v
        bad(ApproxSampleStream, t, mu, sigma, alpha, l2, 100)
    s = ApproxSampleStream(t, mu, sigma, alpha, l, 100)
    bad(s.next, 0)
    bad(s.next, -3, props=False)
    bad(s.mean)  # no draws yet
    lib = L.lib()
    out = np.empty((1, 313), np.float64)
    with pytest.raises(P.PoleeError) as e:
        L.check(lib.polee_sampler_next(s._h, C.c_int32(1), C.c_int32(2), None, None, None, L.ptr(out, L.f64p)), ctx._h)
    assert e.value.status == 1
    assert s.num_draws == 0
    for v in (-1e-300, -1.0, np.inf, -np.inf, np.nan):
        p = np.ones((3, 50)); p[1, 17] = v
        bad(multinomial_counts, p, 10, ctx=ctx)
    p = np.ones((3, 50)); p[2] = 0.0
    bad(multinomial_counts, p, 10, ctx=ctx)
    assert multinomial_counts(p, 0, ctx=ctx).max() == 0  # (m = 0: nothing to place, a row without mass is fine)
    cnt = np.empty((1, 4), np.uint32)
    pp = np.ones((1, 4))
    for D, n in ((0, 4), (-1, 4), (1, 0), (1, -5), (1, 2 ** 31)):
        with pytest.raises(P.PoleeError) as e:
            L.check(lib.polee_multinomial_counts(ctx._h, L.ptr(pp, L.f64p), C.c_int32(D), C.c_int64(n), C.c_int64(5), C.c_uint64(1),
                                                 C.c_uint64(0), L.ptr(cnt, L.u32p)), ctx._h)
        assert e.value.status == 1
    bad(debug_binomial, [-1], [0.5], ctx=ctx)
    bad(debug_binomial, [2 ** 31], [0.5], ctx=ctx)
    bad(debug_binomial, [5], [1.5], ctx=ctx)
    bad(debug_binomial, [5], [np.nan], ctx=ctx)

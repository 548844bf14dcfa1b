"""-m gpu: the isoform effect sizes of the gene-isoform regression (polee_effects_*, csrc/effects.hip, polee_amd/regression.py
IsoformEffects) against tests/isoform_effects_restatement.py, the float64 restatement of src/regression.jl:761-945 in the reference's
own exp / normalise / log form, on SUPPLIED noise.

Tolerances.  Values derived from e or a (min, mean, both Aitchison arrays): absolute 1e-5 = 8 x the 1.2e-6 between an f32 log-space
evaluation and the f64 reference form on these shapes; the device works in f64 around f32 exponentials, so it has margin to spare
(printed: MARGIN lines; measured on an MI355X: at most 2.4e-7 on min and mean, 5.9e-8 on the Aitchison mean, 0 on the Aitchison min).
The counts behind prob_de: a draw within the value tolerance D of the threshold may fall either side, so
count_ref(e > es + D) <= niter prob_de <= count_ref(e > es - D) for every entry, and the same for the Aitchison distances.

Device noise: the mean over 1000 device draws against the restatement's mean over its own 1000 NumPy draws, within 5 standard errors
s / sqrt(niter) of the restatement's mean, s its standard deviation over its draws (measured on an MI355X: 4.22 for e and 3.29 for the
Aitchison mean at the worst entry; a wrong noise scale, a shared stream or a wrong counter moves entries by many more).
"""
import numpy as np
import pytest

import isoform_effects_restatement as T

pytestmark = pytest.mark.gpu

TOL = 1e-5
ES, AES = float(np.log(1.5)), 0.5

# (n, G, F, niter)
CASES = [(70, 9, 2, 40),      # base
         (300, 40, 3, 64),    # base, three factors
         (1100, 60, 1, 33),   # niter no multiple of the wave
         (257, 1, 2, 24),     # one gene of 257 isoforms: far more than the waves of a workgroup, every wave loops
         (64, 64, 2, 25),     # every gene a single isoform: exact zeros; k = round(2.5) = 2
         (70, 9, 2, 1),       # a single draw
         (70, 9, 2, 5),       # round(0.5) = 0, clamped to 1
         (70, 9, 2, 1000),    # the default niter, k = 100
         (70, 9, 2, 2048)]    # 56 KB of LDS: past the 48 KB a launch gets without asking, the attribute path (niter <= 4096 is built)


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def ctx(P):
    return P.Context(0)


def _inputs(n, G, F, seed=5):
    """gene_of: every gene at least one transcript, the rest at random, then a random permutation (not sorted); bias loc ~ N(-2, 3),
    scales ~ exp N(-1.5, 0.7), qw_loc ~ N(0, 1): the reference form stays finite on these"""
    rng = np.random.default_rng(seed + 1000 * n + G)
    gene_of = rng.permutation(np.concatenate([np.arange(G), rng.integers(0, G, size=n - G)])).astype(np.int32)
    return dict(gene_of=gene_of, qw_loc=rng.normal(0, 1, size=(F, n)).astype(np.float32),
                qw_scale=np.exp(rng.normal(-1.5, 0.7, size=(F, n))).astype(np.float32),
                bias_loc=rng.normal(-2, 3, size=n).astype(np.float32),
                bias_scale=np.exp(rng.normal(-1.5, 0.7, size=n)).astype(np.float32))


_REF = {}


def _reference(n, G, F, niter):
    """the restatement on fixed noise, computed once per case and shared"""
    key = (n, G, F, niter)
    if key not in _REF:
        inp = _inputs(n, G, F)
        rng = np.random.default_rng(17 + niter)
        zx = rng.normal(size=(niter, n)).astype(np.float32)
        zw = rng.normal(size=(niter, F, n)).astype(np.float32)
        ref = T.estimate_isoform_effect_sizes(inp["gene_of"], G, ES, AES, inp["qw_loc"], inp["qw_scale"], inp["bias_loc"], inp["bias_scale"],
                                              zx, zw, target_coverage=0.1, return_samples=True)
        assert all(np.isfinite(r).all() for r in ref)
        for r in ref:
            r.setflags(write=False)
        _REF[key] = (inp, zx, zw, ref)
    return _REF[key]


def _run(P, ctx, inp, G, F, niter, **kw):
    fx = P.IsoformEffects(inp["gene_of"], G, F, ctx=ctx)
    return fx.run(inp["qw_loc"], inp["qw_scale"], inp["bias_loc"], inp["bias_scale"], niter=niter, **kw)


@pytest.mark.parametrize("n,G,F,niter", CASES)
def test_supplied_noise_matches_the_restatement(P, ctx, n, G, F, niter):
    inp, zx, zw, ref = _reference(n, G, F, niter)
    min_r, mean_r, prob_r, amin_r, amean_r, aprob_r, e, a = ref
    got = _run(P, ctx, inp, G, F, niter, target_coverage=0.1, effect_size=ES, aitchison_effect_size=AES, zx=zx, zw=zw)
    min_d, mean_d, prob_d, amin_d, amean_d, aprob_d = got
    assert min_d.shape == (F, n) and amin_d.shape == (F, G) and all(g.dtype == np.float32 for g in got)
    worst = [float(np.abs(d.astype(np.float64) - r).max()) for d, r in ((min_d, min_r), (mean_d, mean_r), (amin_d, amin_r), (amean_d, amean_r))]
    print("MARGIN (%d, %d, %d, %d) max |dev - ref|: min %.3g mean %.3g aitchison min %.3g aitchison mean %.3g (bound %.0e)"
          % ((n, G, F, niter) + tuple(worst) + (TOL,)))
    for name, w in zip(("min_effect_sizes", "mean_effect_sizes", "aitchison_min", "aitchison_mean"), worst):
        assert w <= TOL, (name, w)
    # the counts, bracketed: no entry is left unchecked
    for name, dev, samples in (("prob_de", prob_d, e.astype(np.float64)), ("aitchison_prob_de", aprob_d, np.abs(a.astype(np.float64)))):
        thr = ES if name == "prob_de" else AES
        cnt = dev.astype(np.float64) * niter
        assert np.abs(cnt - np.rint(cnt)).max() < 1e-3, name
        lo, hi = (samples > thr + TOL).sum(axis=2), (samples > thr - TOL).sum(axis=2)
        cnt = np.rint(cnt)
        assert (lo <= cnt).all() and (cnt <= hi).all(), (name, int((cnt < lo).sum()), int((cnt > hi).sum()))
    if G == n:  # single-isoform genes: log 1 - log 1, exactly
        for d in (min_d, mean_d, amin_d, amean_d):
            assert not d.any()
        assert not prob_d.any() and not aprob_d.any()  # (0 > log 1.5 and 0 > 0.5 are false)
        assert T.order_statistic_index(niter, 0.1) == 2


def test_thresholds_of_none_give_no_probabilities_and_negative_ones_count_the_exact_zeros(P, ctx):
    n, G, F, niter = CASES[0]
    inp, zx, zw, ref = _reference(n, G, F, niter)
    got = _run(P, ctx, inp, G, F, niter, zx=zx, zw=zw)
    assert got[2] is None and got[5] is None
    np.testing.assert_array_equal(got[0], _run(P, ctx, inp, G, F, niter, effect_size=ES, aitchison_effect_size=AES, zx=zx, zw=zw)[0])
    inp1, zx1, zw1, _ = _reference(64, 64, 2, 25)
    got = _run(P, ctx, inp1, 64, 2, 25, effect_size=-0.1, aitchison_effect_size=-0.1, zx=zx1, zw=zw1)
    assert (got[2] == 1.0).all() and (got[5] == 1.0).all()  # (e = 0 > -0.1 in every draw)


def test_device_noise_is_reproducible_and_seeded(P, ctx):
    n, G, F, niter = 300, 40, 3, 64
    inp = _inputs(n, G, F)
    kw = dict(target_coverage=0.1, effect_size=ES, aitchison_effect_size=AES)
    fx = P.IsoformEffects(inp["gene_of"], G, F, ctx=ctx)
    args = (inp["qw_loc"], inp["qw_scale"], inp["bias_loc"], inp["bias_scale"])
    a = fx.run(*args, niter=niter, seed=11, **kw)
    b = fx.run(*args, niter=niter, seed=11, **kw)
    c = _run(P, ctx, inp, G, F, niter, seed=11, **kw)  # (another handle)
    d = fx.run(*args, niter=niter, seed=12, **kw)
    for x, y, z, w in zip(a, b, c, d):
        assert np.isfinite(x).all()
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, z)
    assert (a[1] != d[1]).mean() > 0.5 and (a[4] != d[4]).mean() > 0.5
    assert fx.kernel_ms is not None and fx.kernel_ms > 0


def test_device_noise_has_the_statistics_of_the_restatement(P, ctx):
    n, G, F, niter = 300, 40, 2, 1000
    inp = _inputs(n, G, F)
    rng = np.random.default_rng(23)
    zx, zw = rng.normal(size=(niter, n)), rng.normal(size=(niter, F, n))
    e, a = T.effect_size_samples(inp["gene_of"], G, inp["qw_loc"], inp["qw_scale"], inp["bias_loc"], inp["bias_scale"], zx, zw)
    got = _run(P, ctx, inp, G, F, niter, seed=2024)
    worst = []
    for name, dev, s in (("mean_effect_sizes", got[1], e.astype(np.float64)), ("aitchison_mean", got[4], a.astype(np.float64))):
        se = s.std(axis=2, ddof=1) / np.sqrt(niter)
        diff = np.abs(dev - s.mean(axis=2))
        worst.append(float((diff / (se + 1e-12))[se > 0].max()))
        assert (diff <= 5.0 * se).all(), (name, worst[-1])
    print("MARGIN device noise: largest |mean_dev - mean_ref| in standard errors of the restatement's mean: e %.2f, aitchison %.2f" % tuple(worst))


def test_bad_arguments_are_refused_with_a_message(P, ctx):
    n, G, F, niter = CASES[0]
    inp, zx, zw, _ = _reference(n, G, F, niter)
    for bad in (G, -1):
        g = inp["gene_of"].copy()
        g[3] = bad
        with pytest.raises(P.PoleeError) as ei:
            P.IsoformEffects(g, G, F, ctx=ctx)
        assert ei.value.status == 1 and "gene_of[3]" in str(ei.value)
    fx = P.IsoformEffects(inp["gene_of"], G, F, ctx=ctx)
    args = (inp["qw_loc"], inp["qw_scale"], inp["bias_loc"], inp["bias_scale"])
    for kw, word in ((dict(niter=0), "niter"), (dict(niter=niter, target_coverage=0.0), "target_coverage"),
                     (dict(niter=niter, target_coverage=1.5), "target_coverage"), (dict(niter=niter, target_coverage=float("nan")), "target_coverage"),
                     (dict(niter=niter, zx=zx[:-1], zw=zw), "noise"), (dict(niter=niter, zx=zx, zw=zw[:, :1]), "noise"),
                     (dict(niter=niter, zx=zx), "zx and zw")):
        with pytest.raises(P.PoleeError) as ei:
            fx.run(*args, **kw)
        assert ei.value.status == 1 and word in str(ei.value), (kw.keys(), str(ei.value))
    assert fx.run(*args, niter=niter, target_coverage=1.0, zx=zx, zw=zw)[0].shape == (F, n)  # (the handle still works; coverage 1 is in range)

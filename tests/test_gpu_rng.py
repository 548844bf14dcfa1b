"""The device normal generator (csrc/rng.hpp) against its NumPy restatement (tests/rng_restatement.py).  Run with `pytest -m gpu` on an
MI355X.

a. words: polee_debug_philox equals the restated rounds bit for bit, the high key word included.
b. Box-Muller: polee_debug_box_muller over every value of the u1 word and every value of the u2 word, against f64 Box-Muller on the
   device's own f32 uniforms.
c. consumers: the VI loop, the alternative approximations, the samplers and the approximation density's sampler draw, bit for bit,
   what the two hooks give for their counter layouts.
d. the battery of distribution statistics of tests/test_rng_host.py on the VI loop's exported noise."""
import ctypes as C

import numpy as np
import pytest

import rng_restatement as R
from conftest import random_tree
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEEDS = (123456789, 0xDEADBEEF00000007)
# Worst absolute error of a draw against f64 Box-Muller on the same f32 uniforms, MEASURED over the twelve sweeps of
# test_box_muller_sweep (see its docstring), and the bounds the tests hold the device to: twice the measurement, rounded up to one
# significant digit (the sweeps are exhaustive and deterministic: the margin is for a later compiler or libm).
E0_BOUND, E1_BOUND = 2e-6, 5e-6  # measured: E0 = 9.216e-7 (which = 0), E1 = 2.284e-6 (which = 1)


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def ctx(P):
    return P.Context(0)


def device_philox(ctx, seed, counters):
    """polee_debug_philox: counters uint32 [..., 4] -> words uint32 [..., 4]"""
    from polee_amd import _lib as L
    c = np.ascontiguousarray(counters, np.uint32)
    w = np.empty_like(c)
    L.check(L.lib().polee_debug_philox(ctx._h, C.c_uint64(int(seed)), c.ctypes.data_as(L.u32p), C.c_int64(c.size // 4),
                                       w.ctypes.data_as(L.u32p)), ctx._h)
    return w


def device_box_muller(ctx, which, words):
    """polee_debug_box_muller: words uint32 [..., 4] -> z f32 [..., 4]"""
    from polee_amd import _lib as L
    w = np.ascontiguousarray(words, np.uint32)
    z = np.empty(w.shape, np.float32)
    L.check(L.lib().polee_debug_box_muller(ctx._h, C.c_int32(which), w.ctypes.data_as(L.u32p), C.c_int64(w.size // 4),
                                           z.ctypes.data_as(L.f32p)), ctx._h)
    return z


def hook_noise(ctx, seed, step, K, nm1):
    """[K][nm1] f32: the which = 0 hook on the RESTATED words of the VI layout"""
    return R.blocks_to_draws(device_box_muller(ctx, 0, R.vi_words(seed, step, K, nm1)), K)


# ---- a. words ------------------------------------------------------------------------------------------------------------------
def test_device_philox_matches_the_published_vectors(ctx):
    c = np.array([[0, 0, 0, 0]], np.uint32)
    assert [int(x) for x in device_philox(ctx, 0, c)[0]] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    c = np.array([[0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], np.uint32)
    assert [int(x) for x in device_philox(ctx, (0x299F31D0 << 32) | 0xA4093822, c)[0]] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    c = np.full((1, 4), 0xFFFFFFFF, np.uint32)
    assert [int(x) for x in device_philox(ctx, 2 ** 64 - 1, c)[0]] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


@pytest.mark.parametrize("seed", [0, 123456789, 0xFEDCBA9876543210])
def test_device_philox_matches_the_restatement(ctx, seed):
    """4 096 random counters, and the library's layouts with their tag words, under a zero key, a key with an empty high word and a
    key with all of bits 32..63 in play."""
    rng = np.random.default_rng(5)
    c = rng.integers(0, 2 ** 32, size=(4096, 4), dtype=np.uint64).astype(np.uint32)
    c = np.concatenate([c, R.vi_counters(6, 300, 2).reshape(-1, 4), R.approx_counters(3, 257).reshape(-1, 4)])
    want = R.philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], seed)
    got = device_philox(ctx, seed, c)
    assert got.tobytes() == want.tobytes(), np.flatnonzero((got != want).any(axis=1))[:5]
    if seed >> 32:  # the high word reaches the key: the same counters under the low word alone give other words
        assert (device_philox(ctx, seed & 0xFFFFFFFF, c) != got).any(axis=1).all()


# ---- b. Box-Muller, exhaustively in each argument ------------------------------------------------------------------------------
SWEEPS = [("u1", w) for w in (0, (1 << 22) << 8, 0xFFFFFF00)] + [("u2", w) for w in (0, 0x80000000, 0xFFFFFF00)]
CHUNK = 1 << 22  # blocks per call: 64 MB of words up, 64 MB of normals down
_worst = {}


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("swept,fixed", SWEEPS)
def test_box_muller_sweep(ctx, which, swept, fixed):
    """All 2^24 values of one uniform's word (its upper 24 bits; the low 8 are zero) with the other word fixed: u1 swept at the u2
    words 0, 2^22 << 8 (a quarter revolution) and 0xFFFFFF00 (u2 = 1.0f); u2 swept at the u1 words 0 (the largest radius, 5.887),
    0x80000000 and 0xFFFFFF00 (the clamped one: the smallest radius, 3.45e-4).  which = 0 (rng.hpp's hardware log2 / sqrt / sin /
    cos): a block carries two pairs, 2^23 blocks cover a sweep; which = 1 (approx.hip's libm variant): one normal per block, 2^24
    blocks, and the other three outputs are 0.

    Every value is finite, |z| <= 5.8871, no pair is (0, 0), z^2 + z'^2 of a pair is r^2 within 2 sqrt(2) r E + 2 E^2 (each of z, z'
    within E of a point on the circle of radius r), and every value is within E of f64 Box-Muller on the same f32 uniforms.

    Measured on an MI355X, the worst absolute error over the six sweeps of each variant:
      which = 0: E0 = 9.216e-7 at the words (u1, u2) = (0x00000000, 0x81FD6B00): the largest radius, device -5.8800292, f64 -5.8800301.
                 Per sweep: u1 swept 4.771e-7 (u1 word 0x00127400, at each of the three u2 words); u2 swept 9.216e-7, 2.192e-7 and
                 5.3e-11 at the u1 words 0, 0x80000000, 0xFFFFFF00 -- the error follows the radius.
      which = 1: E1 = 2.284e-6 at the words (0x00000000, 0xC8D41500): the largest radius again, device 1.2656674, f64 1.2656652; the f32
                 product 2 pi u2 rounds the angle by up to 2.4e-7 before cosf sees it.  Per sweep: u1 swept 5.877e-7, 5.585e-7, 5.877e-7;
                 u2 swept 2.284e-6, 4.533e-7, 1.3e-10.
    The bounds are twice that, rounded up to one significant digit: 2e-6 and 5e-6.  E0 is below the 4e-6 at which it would be a finding."""
    E = (E0_BOUND, E1_BOUND)[which]
    per_block = 2 if which == 0 else 1
    nblocks = (1 << 24) // per_block
    worst = (0.0, None)
    for b0 in range(0, nblocks, CHUNK):
        k = np.arange(b0, b0 + CHUNK, dtype=np.uint32)
        words = np.empty((CHUNK, 4), np.uint32)
        for h in range(2):
            # pair h of block i holds value i + h * nblocks of the sweep (which = 1 reads pair 0 alone)
            v = (k + np.uint32(h * nblocks if which == 0 else 0)) << np.uint32(8)
            words[:, 2 * h] = v if swept == "u1" else fixed
            words[:, 2 * h + 1] = fixed if swept == "u1" else v
        z = device_box_muller(ctx, which, words)
        assert np.isfinite(z).all()
        assert np.abs(z).max() <= R.R_MAX
        if which == 0:
            ref = R.box_muller(words)
            pairs = z.reshape(-1, 2).astype(np.float64)
            r = R.radius(words[:, 0::2]).reshape(-1)
            zero = (pairs == 0).all(axis=1)
            assert not zero.any(), ("a pair of exact zeros at words", words.reshape(-1, 2)[np.flatnonzero(zero)[:3]])
            circle = np.abs((pairs ** 2).sum(axis=1) - r * r) - (2 * np.sqrt(2.0) * r * E + 2 * E * E)
            assert circle.max() <= 0, ("z^2 + z'^2 off r^2 at words", words.reshape(-1, 2)[circle.argmax()])
        else:
            assert not z[:, 1:].any()  # the three outputs the libm variant does not produce
            if swept == "u1":  # (the three fixed angles have a cosine other than 0 in f32: a zero here is a radius of 0)
                zero = z[:, 0] == 0
                assert not zero.any(), ("an exact zero at words", words[np.flatnonzero(zero)[:3], :2])
            ref = np.zeros(z.shape)
            ref[:, 0] = R.box_muller_libm(words)
        err = np.abs(z.astype(np.float64) - ref)
        i = int(err.argmax())
        if err.flat[i] > worst[0]:
            blk, e = divmod(i, 4)
            worst = (float(err.flat[i]), [hex(int(x)) for x in words[blk, 2 * (e // 2):2 * (e // 2) + 2]], float(z.flat[i]), float(ref.flat[i]))
    print("which = %d, %s swept, other word %#x: worst |error| %.4g at words (u1, u2) = %s (device %r, f64 %r)"
          % (which, swept, fixed, worst[0], worst[1], worst[2], worst[3]))
    _worst[(which, swept, fixed)] = worst
    assert worst[0] <= E, worst


def test_box_muller_pair_at_the_clamped_word(ctx):
    """u1 word 0xFFFFFF00 and above: (k + 1/2) 2^-24 rounds to 1.0f in f32, where the radius, and with it both normals of the pair,
    would be exactly 0.  With the clamp the radius is sqrt(-2 ln(1 - 2^-24)) = 3.4527e-4, in both variants."""
    words = np.array([[0xFFFFFF00, 0, 0xFFFFFFFF, 1 << 30], [0xFFFFFFFF, 3 << 30, 0xFFFFFF7F, 1 << 31]], np.uint32)
    z = device_box_muller(ctx, 0, words).astype(np.float64)
    r = 3.4526698e-4
    assert np.allclose(z, [[r, 0, 0, r], [0, -r, -r, 0]], rtol=0, atol=1e-9), z
    assert abs(float(device_box_muller(ctx, 1, words)[0, 0]) - r) < 1e-9


# ---- c. every consumer draws what the generator defines ------------------------------------------------------------------------
_samples = {}


def _sample(P, ctx, n):
    """The smallest sample a fit accepts: 4 n fragments over n transcripts, two in three compatible with two transcripts.  Only the
    noise of a fit is read.  -> (RNASeqSample, PolyaTreeTransform)"""
    if n not in _samples:
        m = 4 * n
        i = np.arange(m)
        a, b = i % n, (7 * i + 3) % n
        keep_b = (i % 3 != 0) & (a != b)
        rows = np.concatenate([i, i[keep_b]])
        cols = np.concatenate([a, b[keep_b]])
        order = np.lexsort((rows, cols))
        rows, cols = rows[order], cols[order]
        colptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(cols, minlength=n), out=colptr[1:])
        rng = np.random.default_rng(n)
        nzval = (rng.random(rows.size) * 1e-3 + 1e-5).astype(np.float32)
        efflens = rng.uniform(200, 3000, n).astype(np.float32)
        s = P.RNASeqSample(m, n, (colptr + 1).astype(np.uint32), (rows + 1).astype(np.uint32), nzval, efflens, ctx=ctx)
        parents, js = random_tree(n, rng, "balanced" if n > 5000 else "random")
        _samples[n] = (s, P.PolyaTreeTransform(parents, js, ctx=ctx))
    return _samples[n]


@pytest.mark.parametrize("nm1", [1, 255, 256, 257, 1100])
def test_vi_and_alt_fits_export_the_generators_noise(P, ctx, nm1):
    """polee_vi_export_noise for K in {1, 4, 6, 8} (draws 4, 5 are the second block of a node), steps 1, 2, 500 and both seeds: the bytes
    of the which = 0 hook on the restated words {k, d / 4, step, 'pole'}, and within E0 of the f64 restatement.
    polee_altvi_export_noise: the same bytes."""
    s, t = _sample(P, ctx, nm1 + 1)
    for seed in SEEDS:
        for K in (1, 4, 6, 8):
            fit = P.LikelihoodApproximationFit(s, t, num_steps=2, num_mc_samples=K, seed=seed)
            alt = P.AltLikelihoodApproximationFit(s, P.LogisticNormalApprox(), None, num_steps=2, num_mc_samples=K, seed=seed)
            for step in (1, 2, 500):
                z = fit.export_noise(step)
                assert z.shape == (K, nm1) and z.dtype == np.float32
                want = hook_noise(ctx, seed, step, K, nm1)
                assert z.tobytes() == want.tobytes(), (seed, K, step, np.argwhere(z != want)[:3])
                err = np.abs(z.astype(np.float64) - R.randn(seed, step, K, nm1))
                assert err.max() <= E0_BOUND, (seed, K, step, err.max(), np.unravel_index(err.argmax(), err.shape))
                assert alt.export_noise(step).tobytes() == z.tobytes(), (seed, K, step)


def _sampler_params(n, rng):
    return (rng.normal(0, 1, n - 1).astype(np.float32), np.exp(rng.normal(-1, 0.3, n - 1)).astype(np.float32),
            rng.normal(0, 0.3, n - 1).astype(np.float32))


def _sampler_noise(ctx, call_seed, ndraws, nm1):
    """[ndraws][nm1]: blocks of 8 draws, block b0 under sampler_block_seed(call_seed, b0), draw d its draw d - b0 of step 1"""
    return np.concatenate([hook_noise(ctx, R.sampler_block_seed(call_seed, b0), 1, min(8, ndraws - b0), nm1) for b0 in range(0, ndraws, 8)])


@pytest.mark.parametrize("seed", [123456789, 2 ** 64 - 5])
def test_samplers_draw_from_the_generators_noise(P, ctx, seed):
    """polee_sampler_draw (two calls of an ApproxLikelihoodSampler: the second one's seed is seed + 0x632BE59BD9B4E019) and the
    streaming ApproxSampleStream, 11 draws = a full block of 8 and a short one: the device-RNG draws are the bytes of the draws from
    supplied noise z0 = the hook's noise of every block's seed.  2^64 - 5: the block seed and the call seed wrap."""
    from polee_amd.sample import ApproxSampleStream
    n, N = 258, 11
    rng = np.random.default_rng(7)
    parents, js = random_tree(n, rng)
    t = P.PolyaTreeTransform(parents, js, ctx=ctx)
    mu, sigma, alpha = _sampler_params(n, rng)
    dev, sup = P.ApproxLikelihoodSampler(), P.ApproxLikelihoodSampler()
    for a in (dev, sup):
        a.set_transform(t, mu, sigma, alpha)
        a.seed(seed)
    first = None
    for call in range(2):
        z0 = _sampler_noise(ctx, R.sampler_call_seed(seed, call), N, n - 1)
        assert z0.shape == (N, n - 1)
        x = dev.rand(N)
        assert x.tobytes() == sup.rand(N, z0=z0).tobytes(), (seed, call)
        if call == 0:
            first = x
            z0_first = z0
        else:
            assert (x != first).any()
    l = rng.uniform(200, 3000, n).astype(np.float32)
    raw = ApproxSampleStream(t, mu, sigma, alpha, l, 10000, seed).next(N, props=False, raw=True)["raw"]
    assert raw.tobytes() == ApproxSampleStream(t, mu, sigma, alpha, l, 10000, seed).next(N, props=False, raw=True, z0=z0_first)["raw"].tobytes()
    assert raw.tobytes() == first.tobytes()


@pytest.mark.parametrize("seed", SEEDS)
def test_approx_density_sampler_draws_from_the_libm_variant(P, ctx, seed):
    """polee_approx_sample (RNASeqApproxLikelihood.sample), S = 3, n - 1 = 257: z0 = None with a seed gives the bytes of z0 = the
    which = 1 hook on the restated words of the counters {k, s, 1, 'appx'}."""
    S, n = 3, 258
    rng = np.random.default_rng(11)
    idx = [O.make_inverse_ptt_params(*random_tree(n, rng)) for _ in range(S)]
    L_, R_, F_ = (np.stack([i[j] for i in idx]) for j in range(3))
    ap = P.RNASeqApproxLikelihood(dict(efflen=rng.uniform(200, 3000, size=(S, n)).astype(np.float32),
                                       la_mu=rng.normal(0, 1, size=(S, n - 1)).astype(np.float32),
                                       la_sigma=np.exp(rng.normal(-1, 0.3, size=(S, n - 1))).astype(np.float32),
                                       la_alpha=rng.normal(0, 0.3, size=(S, n - 1)).astype(np.float32),
                                       left_index=L_, right_index=R_, leaf_index=F_), ctx=ctx)
    words = R.approx_words(seed, S, n - 1)
    z0 = np.ascontiguousarray(device_box_muller(ctx, 1, words)[..., 0])
    err = np.abs(z0.astype(np.float64) - R.approx_randn(seed, S, n - 1))
    assert err.max() <= E1_BOUND, err.max()
    x = ap.sample(seed=seed)
    assert x.tobytes() == ap.sample(z0=z0, seed=seed).tobytes()
    assert x.tobytes() != ap.sample(seed=seed ^ (1 << 32)).tobytes()


# ---- d. the battery on the device's own export ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_exported_noise_passes_the_battery(P, ctx, seed):
    """The statistics and caps of tests/test_rng_host.py on polee_vi_export_noise itself, K = 8, n - 1 = 131 072 (2^20 draws): given
    b and c this is redundant; it is the check that stands without the hooks."""
    K, nm1 = 8, 131072
    s, t = _sample(P, ctx, nm1 + 1)

    def fit(sd):
        return P.LikelihoodApproximationFit(s, t, num_steps=2, num_mc_samples=K, seed=sd)
    f = fit(seed)
    stats = R.battery(f.export_noise(1), f.export_noise(2), fit((seed + 1) % 2 ** 64).export_noise(1), fit(seed ^ (1 << 32)).export_noise(1))
    for name, (v, cap) in stats.items():
        print("%-40s %.4g (cap %.4g)" % (name, v, cap))
    assert len(stats) == 15
    assert not R.battery_failures(stats), R.battery_failures(stats)

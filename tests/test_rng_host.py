"""CPU tests of the normal generator's restatement (tests/rng_restatement.py; no GPU): the Philox rounds against the published vectors,
the facts of the f32 uniform over all 2^24 words, and the battery of distribution statistics on 2^20 restated draws of two seeds, one
of them with the key's high word in play.  tests/test_gpu_rng.py holds the device to the same restatement and the same battery."""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401
import rng_restatement as R

SEEDS = (123456789, 0xDEADBEEF00000007)


def test_philox_restatement_matches_the_published_vectors():
    """Random123's known-answer vectors for Philox4x32-10; the key is (low word, high word) of the seed."""
    w = R.philox4x32_10(0, 0, 0, 0, 0)
    assert [int(x) for x in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    w = R.philox4x32_10(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, (0xFFFFFFFF << 32) | 0xFFFFFFFF)
    assert [int(x) for x in w] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    w = R.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, (0x299F31D0 << 32) | 0xA4093822)
    assert [int(x) for x in w] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    # vectorised over counters: rows are the single calls
    c = np.array([[0, 0, 0, 0], [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], np.uint32)
    w = R.philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], (0x299F31D0 << 32) | 0xA4093822)
    assert w.shape == (2, 4) and w.dtype == np.uint32 and [int(x) for x in w[1]] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_block_and_call_seeds_wrap_modulo_two_to_the_64():
    assert R.sampler_block_seed(123456789, 0) == 123456789
    assert R.sampler_block_seed(123456789, 8) == (123456789 + 8 * 0x9E3779B97F4A7C15) % 2 ** 64
    assert R.sampler_block_seed(2 ** 64 - 5, 8) == (8 * 0x9E3779B97F4A7C15 - 5) % 2 ** 64 < 2 ** 64
    assert R.sampler_call_seed(2 ** 64 - 5, 1) == (0x632BE59BD9B4E019 - 5) % 2 ** 64


def test_facts_of_the_f32_uniform_over_all_words():
    """All 2^24 values of a word's upper 24 bits.  The f32 sum k + 1/2 is inexact from k = 2^23 on (half of the values, each off by
    2^-25 on the 2^-23 grid) and reaches 1.0f at the last k; the clamped uniform stays below 1, so the radius is never 0."""
    k = np.arange(1 << 24, dtype=np.uint32)
    w = k << np.uint32(8)
    raw, u, ideal = R.u01f_raw(w), R.u01f(w), R.u01d(w)
    assert raw.dtype == np.float32 and u.dtype == np.float32
    inexact = np.flatnonzero(raw.astype(np.float64) != ideal)
    assert inexact.size == 8388608 and inexact[0] == 1 << 23
    assert np.abs(raw.astype(np.float64) - ideal).max() == 2.0 ** -25
    assert raw[-1] == np.float32(1.0) and np.count_nonzero(raw == np.float32(1.0)) == 1
    # the clamp moves that one value and no other
    assert np.count_nonzero(u != raw) == 1 and u[-1] == np.nextafter(np.float32(1.0), np.float32(0.0))
    assert u.max() < 1.0 and u.min() == np.float32(2.0 ** -25) and raw.min() == np.float32(2.0 ** -25)
    assert np.all(np.diff(u.astype(np.float64)) >= 0)
    # the low 8 bits of a word are not read
    assert np.array_equal(R.u01f(w[::4097] | np.uint32(0xFF)), u[::4097])
    r = R.radius(w)
    assert R.R_MIN <= r.min() and r.max() <= R.R_MAX and r.min() > 0
    assert r.argmax() == 0 and r.argmin() >= (1 << 24) - 2
    # the order within a block and the one place where the pair would be (0, 0) without the clamp
    z = R.box_muller(np.array([[0xFFFFFF00, 0, 0, 1 << 30]], np.uint32))[0]
    assert 0 < z[0] and abs(z[0] - r[-1]) < 1e-15 and abs(z[1]) < 1e-9  # angle (1/2) / 2^24 revolutions: cos = 1 - 2e-14
    # a quarter revolution + 2^-25: (-r 2 pi 2^-25, r) = (-1.1e-6, 5.887)
    assert -2e-6 < z[2] < 0 and abs(z[3] - r[0]) < 1e-12
    assert R.box_muller_libm(np.array([[0xFFFFFF00, 0, 7, 7]], np.uint32))[0] == z[0]


def test_draw_order_of_the_restated_noise():
    """randn [K][nm1]: draw d of node k is element d % 4 of the block with counter {k, d / 4, step, 'pole'}."""
    seed, step, K, nm1 = SEEDS[1], 3, 6, 5
    z = R.randn(seed, step, K, nm1)
    assert z.shape == (K, nm1)
    for d in range(K):
        for k in range(nm1):
            w = R.philox4x32_10(k, d // 4, step, 0x706F6C65, seed)
            assert z[d, k] == R.box_muller(w)[d % 4]
    a = R.approx_randn(seed, 3, 5)
    assert a.shape == (3, 5) and a[2, 4] == R.box_muller_libm(R.philox4x32_10(4, 2, 1, 0x61707078, seed))


@pytest.mark.parametrize("seed", SEEDS)
def test_restated_noise_passes_the_battery(seed):
    """2^20 draws (K = 8, n - 1 = 131072) of step 1: moments, Kolmogorov-Smirnov, the tail beyond 4, and the correlations between
    neighbouring nodes, within a pair, within a block, across blocks, steps and seeds (low and high key word).  Each cap is 5 standard
    errors of the statistic under N(0,1) (KS: 2.6): a condition on the generator, not a record of what it gives -- the restatement
    stays below 2 standard errors in every line for both seeds."""
    K, nm1 = 8, 131072
    stats = R.battery(R.randn(seed, 1, K, nm1), R.randn(seed, 2, K, nm1), R.randn((seed + 1) % 2 ** 64, 1, K, nm1),
                      R.randn(seed ^ (1 << 32), 1, K, nm1))
    for name, (v, cap) in stats.items():
        print("%-40s %.4g (cap %.4g)" % (name, v, cap))
    assert len(stats) == 15
    assert not R.battery_failures(stats), R.battery_failures(stats)


def test_the_battery_notices_a_broken_generator():
    """The battery on deliberately wrong noise: a dropped high key word (seed ^ 2^32 repeats seed), cos used for both halves of a pair, a
    tail cut at 3."""
    K, nm1 = 8, 32768
    seed = SEEDS[1]
    z, s2, p1 = R.randn(seed, 1, K, nm1), R.randn(seed, 2, K, nm1), R.randn(seed + 1, 1, K, nm1)
    bad = R.battery_failures(R.battery(z, s2, p1, z.copy()))
    assert list(bad) == ["corr seed, seed ^ 2^32"]
    zz = z.copy()
    zz[1] = zz[0]
    assert "corr draws 0, 1 (cos, sin of a pair)" in R.battery_failures(R.battery(zz, s2, p1, R.randn(seed ^ (1 << 32), 1, K, nm1)))
    clipped = np.clip(z, -3.0, 3.0)  # (excess kurtosis -0.1 against a cap of 0.048 at this N)
    assert "excess kurtosis" in R.battery_failures(R.battery(clipped, s2, p1, R.randn(seed ^ (1 << 32), 1, K, nm1)))

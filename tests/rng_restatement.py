"""NumPy restatement of the device normal generator (polee_amd/csrc/rng.hpp) and of the counter layouts its consumers use.  Nothing
here imports the library: tests/test_rng_host.py holds the restatement to published vectors and to N(0,1), tests/test_gpu_rng.py
holds the device to the restatement.

A block is Philox4x32-10 of a counter (c0, c1, c2, c3) under the key (seed & 0xFFFFFFFF, seed >> 32).  A word's upper 24 bits k give
the uniform (k + 1/2) / 2^24.  The device forms it in f32: k + 1/2 is not a float from k = 2^23 on, the sum rounds to even, and
k = 2^24 - 1 gives exactly 1.0f.  The radius takes the uniform clamped to the largest float below 1 (u01f), the angle takes it as it
is (u01f_raw: one revolution is the angle 0).  Box-Muller here is f64 arithmetic on those f32 uniforms."""
import math

import numpy as np

MASK = np.uint64(0xFFFFFFFF)
M64 = (1 << 64) - 1
TAG_VI = 0x706F6C65      # 'pole': VI loop, alternative approximations, samplers, regression
TAG_APPROX = 0x61707078  # 'appx': polee_approx_sample
BELOW_ONE = np.float32(1.0) - np.float32(2.0 ** -24)  # 0x1.fffffep-1f
R_MIN, R_MAX = 3.45e-4, 5.8871  # sqrt(-2 ln(1 - 2^-24)) = 3.4527e-4, sqrt(-2 ln 2^-25) = 5.88706


def philox4x32_10(c0, c1, c2, c3, seed):
    """Four uint32 counter words (broadcast against each other) -> words uint32 [..., 4]."""
    c = [np.asarray(x).astype(np.uint64) & MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([x.astype(np.uint32) for x in c], axis=-1)


def u01f_raw(w):
    """The f32 uniform as the device's additions and product round it: in [2^-25, 1]."""
    w = np.asarray(w, np.uint32)
    return ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def u01f(w):
    """... clamped to the largest float below 1: what the radius is taken from."""
    return np.minimum(u01f_raw(w), BELOW_ONE)


def u01d(w):
    """The ideal (k + 1/2) / 2^24, exact in f64."""
    w = np.asarray(w, np.uint32)
    return ((w >> np.uint32(8)).astype(np.float64) + 0.5) * (1.0 / 16777216.0)


def radius(w):
    return np.sqrt(-2.0 * np.log(u01f(w).astype(np.float64)))


def box_muller(words):
    """words uint32 [..., 4] -> f64 [..., 4]: z[0], z[1] = r(word 0) (cos, sin)(2 pi u(word 1)), z[2], z[3] from words 2, 3."""
    words = np.asarray(words, np.uint32)
    z = np.empty(words.shape, np.float64)
    for h in (0, 1):
        r = radius(words[..., 2 * h])
        a = (2.0 * math.pi) * u01f_raw(words[..., 2 * h + 1]).astype(np.float64)
        z[..., 2 * h] = r * np.cos(a)
        z[..., 2 * h + 1] = r * np.sin(a)
    return z


def box_muller_libm(words):
    """The one normal per block of approx.hip: the cosine half of words 0, 1.  words [..., 4] -> f64 [...]."""
    words = np.asarray(words, np.uint32)
    return radius(words[..., 0]) * np.cos((2.0 * math.pi) * u01f_raw(words[..., 1]).astype(np.float64))


def vi_counters(K, nm1, step):
    """Counters {k, draw / 4, step, 'pole'} of a step's noise: uint32 [ceil(K / 4)][nm1][4]."""
    G = (K + 3) // 4
    c = np.empty((G, nm1, 4), np.uint32)
    c[..., 0] = np.arange(nm1, dtype=np.uint32)[None, :]
    c[..., 1] = np.arange(G, dtype=np.uint32)[:, None]
    c[..., 2] = step
    c[..., 3] = TAG_VI
    return c


def vi_words(seed, step, K, nm1):
    c = vi_counters(K, nm1, step)
    return philox4x32_10(c[..., 0], c[..., 1], c[..., 2], c[..., 3], seed)


def blocks_to_draws(z, K):
    """[G][nm1][4] of the blocks -> [K][nm1]: draw d is element d % 4 of group d / 4."""
    G, nm1 = z.shape[:2]
    return np.ascontiguousarray(np.moveaxis(z, 2, 1).reshape(4 * G, nm1)[:K])


def randn(seed, step, K, nm1):
    """[K][nm1] f64 of philox_randn(seed, step, d, k)."""
    return blocks_to_draws(box_muller(vi_words(seed, step, K, nm1)), K)


def sampler_block_seed(seed, b0):
    """Seed of the sampler's block of draws that starts at draw b0 (sampler_internal.hpp), modulo 2^64."""
    return (int(seed) + int(b0) * 0x9E3779B97F4A7C15) & M64


def sampler_call_seed(seed, count):
    """Seed of the count-th call (from 0) of an ApproxLikelihoodSampler seeded with `seed` (core.py)."""
    return (int(seed) + 0x632BE59BD9B4E019 * int(count)) & M64


def approx_counters(S, nm1):
    """Counters {k, s, 1, 'appx'} of polee_approx_sample: uint32 [S][nm1][4]."""
    c = np.empty((S, nm1, 4), np.uint32)
    c[..., 0] = np.arange(nm1, dtype=np.uint32)[None, :]
    c[..., 1] = np.arange(S, dtype=np.uint32)[:, None]
    c[..., 2] = 1
    c[..., 3] = TAG_APPROX
    return c


def approx_words(seed, S, nm1):
    c = approx_counters(S, nm1)
    return philox4x32_10(c[..., 0], c[..., 1], c[..., 2], c[..., 3], seed)


def approx_randn(seed, S, nm1):
    return box_muller_libm(approx_words(seed, S, nm1))


# ---- the battery ---------------------------------------------------------------------------------------------------------------
_erf = np.frompyfunc(math.erf, 1, 1)


def normal_cdf(x):
    return 0.5 * (1.0 + _erf(np.asarray(x, np.float64) / math.sqrt(2.0)).astype(np.float64))


def corr_stat(a, b):
    """sqrt(M) |corr(a, b)| over the M pairs: the correlation in units of its own standard error under independence."""
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    a = a - a.mean()
    b = b - b.mean()
    return math.sqrt(a.size) * abs(float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum())))


def battery(z, step2, seed_plus_1, seed_xor_hi):
    """z [8][nm1]: the noise of (seed, step 1); step2, seed_plus_1, seed_xor_hi: the same shape for (seed, step 2), (seed + 1, step 1)
    and (seed ^ 2^32, step 1).  -> {name: (statistic, cap)}; every cap is 5 standard errors of the statistic under N(0,1), but for
    the Kolmogorov-Smirnov sqrt(N) D <= 2.6 (P < 3e-6)."""
    z = np.asarray(z, np.float64)
    assert z.ndim == 2 and z.shape[0] == 8
    N = z.size
    m = z.mean()
    c = z - m
    var = (c * c).mean()
    out = {
        "mean": (abs(m) * math.sqrt(N), 5.0),
        "variance": (abs(var - 1.0), 5.0 * math.sqrt(2.0 / N)),
        "skewness": (abs((c ** 3).mean() / var ** 1.5), 5.0 * math.sqrt(6.0 / N)),
        "excess kurtosis": (abs((c ** 4).mean() / var ** 2 - 3.0), 5.0 * math.sqrt(24.0 / N)),
    }
    s = np.sort(z.ravel())
    F = normal_cdf(s)
    i = np.arange(N, dtype=np.float64)
    D = max(float(((i + 1.0) / N - F).max()), float((F - i / N).max()))
    out["KS"] = (math.sqrt(N) * D, 2.6)
    E = N * math.erfc(4.0 / math.sqrt(2.0))  # 2 N Phi(-4)
    out["count of |z| > 4"] = (abs(float((np.abs(z) > 4.0).sum()) - E), 5.0 * math.sqrt(E))
    pairs = {
        "nodes k, k + 1": (z[:, :-1], z[:, 1:]),
        "draws 0, 1 (cos, sin of a pair)": (z[0], z[1]),
        "draws 0, 2 (the pairs of a block)": (z[0], z[2]),
        "draws 3, 4 (two blocks)": (z[3], z[4]),
        "step 1, step 2": (z, step2),
        "seed, seed + 1": (z, seed_plus_1),
        "seed, seed ^ 2^32": (z, seed_xor_hi),
        "squares of draws 0, 1": (z[0] ** 2, z[1] ** 2),
        "squares of draws 0, 2": (z[0] ** 2, z[2] ** 2),
    }
    for name, (a, b) in pairs.items():
        out["corr " + name] = (corr_stat(a, b), 5.0)
    return out


def battery_failures(stats):
    return {k: v for k, v in stats.items() if not v[0] <= v[1]}

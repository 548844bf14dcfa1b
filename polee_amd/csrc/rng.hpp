// Counter-based normal noise shared by the VI loop (vi.hip), the alternative approximations (altvi.hip), the regression model
// (regression.hip), the isoform effects (effects.hip) and the approximation density's sampler (approx.hip).  Every Philox counter
// layout of the library and its tag word: DESIGN.md §3.17.  tests/rng_restatement.py restates this file in NumPy;
// tests/test_rng_host.py and tests/test_gpu_rng.py hold it to that restatement through polee_debug_philox / polee_debug_box_muller.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace polee {

// ---- counter-based RNG: Philox4x32-10, one N(0,1) per (seed, step, draw, k) -------------
__host__ __device__ inline void philox_round(uint32_t (&c)[4], const uint32_t (&k)[2])
{
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k[0];
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k[1];
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0;
    c[1] = n1;
    c[2] = n2;
    c[3] = n3;
}
// One Philox4x32-10 block of a caller-chosen counter under the key `seed`: key = (low word, high word) of the seed.
__host__ __device__ inline void philox4x32_10(uint32_t (&c)[4], uint64_t seed)
{
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, key);
        key[0] += 0x9E3779B9u;
        key[1] += 0xBB67AE85u;
    }
}

// The uniforms of a word's upper 24 bits k: (k + 1/2) / 2^24.
//   f64: exact, in (0, 1).
//   f32: exact for k < 2^23.  From 2^23 on k + 1/2 is not a float: the sum rounds to even, so the upper half of the values lies on the
//   2^-23 grid (8 388 608 of the 2^24 values are inexact, each by 2^-25) and k = 2^24 - 1 gives exactly 1.0f.
//   philox_u01f_raw is that value, in [2^-25, 1]; philox_u01f clamps it to the largest float below 1, in [2^-25, 1 - 2^-24]: closed
//   at neither 0 nor 1.  Box-Muller takes its radius from philox_u01f (at 1.0f the radius, and with it both normals of the pair,
//   would be exactly 0) and its angle, in revolutions, from philox_u01f_raw (1.0 is the angle 0: harmless).
__host__ __device__ inline float philox_u01f_raw(uint32_t w) { return ((float)(w >> 8) + 0.5f) * (1.0f / 16777216.0f); }
__host__ __device__ inline float philox_u01f(uint32_t w) { return fminf(philox_u01f_raw(w), 0x1.fffffep-1f); }
__host__ __device__ inline double philox_u01d(uint32_t w) { return ((double)(w >> 8) + 0.5) * (1.0 / 16777216.0); }

// Box-Muller on the uniforms of two words, on the hardware's transcendental units: v_log_f32 (log2), v_sqrt_f32 and
// v_sin_f32 / v_cos_f32, which take their argument in revolutions -- sin(2 pi u2) is v_sin_f32(u2), no range reduction.
// (noise, not arithmetic the reference defines; libm's logf + sincosf were ~250 instructions per node of the VI update, a tenth of
// the kernel).  The radius lies in [3.45e-4, 5.8871] (u1 = 1 - 2^-24 and 2^-25).  Measured against Box-Muller in f64 on the same f32
// uniforms, over every u1 word at three u2 words and every u2 word at three u1 words (tests/test_gpu_rng.py): the worst absolute
// error of a draw is E0 = 9.216e-7, at the largest radius (words u1 = 0, u2 = 0x81FD6B00: -5.8800292 for -5.8800301) -- the units'
// error is absolute in sin / cos and is multiplied by the radius; over the u1 words alone it is 4.771e-7 (word 0x00127400).
__device__ inline void philox_box_muller(uint32_t w1, uint32_t w2, float &zc, float &zs)
{
    const float u1 = philox_u01f(w1);
    const float u2 = philox_u01f_raw(w2);
    const float r = __builtin_amdgcn_sqrtf(-1.38629436111989061883f * __log2f(u1));  // sqrt(-2 ln u1)
    zc = r * __builtin_amdgcn_cosf(u2);
    zs = r * __builtin_amdgcn_sinf(u2);
}
// The four N(0,1) of a block's words: z[0], z[1] from words 0, 1 and z[2], z[3] from words 2, 3.
__device__ inline void philox_box_muller4(const uint32_t (&w)[4], float (&z)[4])
{
    philox_box_muller(w[0], w[1], z[0], z[1]);
    philox_box_muller(w[2], w[3], z[2], z[3]);
}
// The libm variant of the approximation density's sampler (approx.hip): one N(0,1) per block, the cosine half of words 0, 1.
// Worst absolute error against f64 on the same uniforms, measured as above: E1 = 2.284e-6 (words u1 = 0, u2 = 0xC8D41500; the f32
// product 2 pi u2 rounds the angle by up to 2.4e-7 and the radius 5.887 multiplies that).
__device__ inline float philox_box_muller_libm(uint32_t w1, uint32_t w2)
{
    const float u1 = philox_u01f(w1);
    const float u2 = philox_u01f_raw(w2);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// Four N(0,1) per Philox block: counter (k, draw / 4, step, 'pole'), two Box-Muller pairs.
__device__ inline void philox_randn4(uint64_t seed, uint32_t step, uint32_t group, uint32_t k, float (&z)[4])
{
    uint32_t c[4] = {k, group, step, 0x706f6c65u};
    philox4x32_10(c, seed);
    philox_box_muller4(c, z);
}
__device__ inline float philox_randn(uint64_t seed, uint32_t step, uint32_t draw, uint32_t k)
{
    float z[4];
    philox_randn4(seed, step, draw >> 2, k, z);
    return z[draw & 3];
}

}  // namespace polee
